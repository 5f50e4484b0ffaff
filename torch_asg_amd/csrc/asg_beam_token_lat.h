// torch_asg_amd/csrc/asg_beam_token_lat.h -- TokenLat: how the lattice passes of the token-graph family walk the outgoing edges
// of a product state.  One text for the backward of the beam-pruned loss (asg_beam_loss.hip: beam_loss_bwd<R, TL, TokenLat<R>>)
// and for the beta pull of the token confidences (asg_beam_conf.hip), so an edge of the one is an edge of the other.
#pragma once
#include "asg_common.h"
#include "asg_kernels.h"

namespace asg {

namespace {

template <typename R>
struct TokenLat {
    using Key = int;
    struct Args { GraphArgs g; BeamGraphArgs bg; BeamLossLayout lay; };
    const int *lab, *orow;
    const int2 *oarc;
    const R *ow, *fw;
    __device__ void bind(const Args &a) {
        lab = a.g.label; orow = a.bg.orow; oarc = (const int2 *) a.bg.oarc; ow = (const R *) a.bg.ow; fw = (const R *) a.g.final_w;
    }
    __device__ int label(int q) const { return lab[q]; }
    __device__ void end(int q, R &e) const { e = fw[q]; }
    template <typename F> __device__ void for_each_out(int q, int lg, int G, F fn) const {
        const int e1 = orow[q + 1];
        for (int e = orow[q] + lg; e < e1; e += G) {
            const int2 a = oarc[e];
            fn(a.x, [&]() -> R { return ow[e]; }, a.y);
        }
    }
};

// TokenLat with the end term of a prefix: a path may end in any kept state of the last set with weight 0 (the lattice-keeping
// streams, asg_beam_stream_conf.hip and asg_beam_conf_window.hip).
template <typename R>
struct PrefixLat : TokenLat<R> {
    struct Args : TokenLat<R>::Args { int fin; };
    int fin;
    __device__ void bind(const Args &a) { TokenLat<R>::bind(a); fin = a.fin; }
    __device__ void end(int q, R &e) const { e = fin ? this->fw[q] : R(0); }
};

}  // namespace

}  // namespace asg
