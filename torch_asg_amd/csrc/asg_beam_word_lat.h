// torch_asg_amd/csrc/asg_beam_word_lat.h -- how the passes behind the word search walk a PAIR's edges: bind_walk (the read-only
// part of a BeamWordFrame) and WordLat, the policy that asg_beam_lattice.h's backward takes.  Two units compile this text: the
// loss over pairs (asg_beam_word_loss.hip: beam_loss_bwd<R, TL, WordLat<R>>) and the word confidences
// (asg_beam_word_conf.hip: the beta pull with a word-event sink), so an edge of the one is an edge of the other.
#pragma once
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"  // the frame of the search, the LM walk and the end of a pair

namespace asg {

namespace {

// the alpha push (asg_beam_word_alpha.inc)
constexpr double kBSumScale = 281474976710656.0;              // 2^48: a target's sum of exp(c - max) over < 2^14 candidates

// The read-only part of a BeamWordFrame for the kernels that only walk the graph and the LM.
template <typename R>
__device__ __forceinline__ void bind_walk(BeamWordFrame<R> &f, const GraphArgs &g, const BeamGraphArgs &bg, const WordLmArgs &lm) {
    bind_graph<R, false>(f, g, bg, lm, 1, 1, 1);
}

// beta PULLS: a pair's own outgoing row is a gather against U_{t+1} in LDS; a separator edge walks the LM.
template <typename R>
struct WordLat {
    using Key = unsigned long long;
    struct Args { GraphArgs g; BeamGraphArgs bg; WordLmArgs lm; BeamWordLossLayout lay; };
    BeamWordFrame<R> f;
    const R *fw;
    Key qmask;
    __device__ void bind(const Args &a) {
        bind_walk<R>(f, a.g, a.bg, a.lm);
        fw = (const R *) a.g.final_w;
        qmask = (1ull << f.qbits) - 1ull;
    }
    __device__ int label(Key p) const { return f.label[(int) (p & qmask)]; }
    __device__ void end(Key p, R &e) const {
        int w;
        if (!word_end<R>(f, fw, (int) (p >> f.qbits), (int) (p & qmask), (R) 0, e, w)) e = Num<R>::ninf();
    }
    // whether an end in a word-end node completes its word at frame len (the event of the final step)
    __device__ constexpr bool end_event() const { return true; }
    template <typename F> __device__ void for_each_out(Key p, int lg, int G, F fn) const {
        const int q = (int) (p & qmask), h = (int) (p >> f.qbits);
        const int e1 = f.orow[q + 1];
        for (int e = f.orow[q] + lg; e < e1; e += G) {
            const int2 arc = f.oarc[e];
            int th = h;
            R w = f.ow[e];
            if (arc.y == f.sep) {                                             // a word ends: the LM moves
                R add;
                int h2;
                if (!f.step(h, f.wos[f.state[q]], h2, add)) continue;
                th = h2;
                w = w + add;
            }
            fn(f.pair(th, arc.x), [&]() -> R { return w; }, arc.y);
        }
    }
};

}  // namespace

}  // namespace asg
