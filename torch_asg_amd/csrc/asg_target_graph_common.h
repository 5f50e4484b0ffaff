// torch_asg_amd/csrc/asg_target_graph_common.h -- what the kernels over per-utterance target graphs share (asg_target_graph.hip:
// the score and its gradients; asg_target_graph_viterbi.hip: the best path): the view of one utterance's arrays, its clamped
// length, the workgroup reduction in a fixed tree and the LDS budget of one workgroup.
#pragma once
#include "asg_common.h"
#include "asg_kernels.h"

namespace asg {

namespace {

constexpr int kTgRed = 256;                     // LDS bytes in front of the vectors (reduction slots, 16 of either dtype)
// what one workgroup may ask for: the resident route of asg_graph_loss.hip (128 KiB of vectors + its scratch)
constexpr size_t kTgLds = 128 * 1024 + 256;

template <typename R> __device__ __forceinline__ R tmax(R a, R b) { return b > a ? b : a; }

__device__ __forceinline__ int tg_len(const int64_t *in_len, int b, int T) {
    if (!in_len) return T;
    const int64_t l = in_len[b];
    return (int) (l < 0 ? 0 : (l > T ? T : l));
}

// Workgroup max / sum over W threads in a fixed tree (butterfly in the wavefront, then the wavefronts ascending); the result
// in every thread.  One wavefront needs neither LDS nor a barrier.
template <typename R, int W, bool MAX>
__device__ __forceinline__ R tg_reduce(R v, R *red) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const R u = (R) __shfl_xor(v, o);
        v = MAX ? tmax(v, u) : v + u;
    }
    if (W == 64) return v;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int s = 1; s < W / 64; ++s) v = MAX ? tmax(v, red[s]) : v + red[s];
    __syncthreads();
    return v;
}

// The arrays of utterance b.
struct TgView {
    const int *label, *row, *src, *tgt, *orow, *oedge, *lab, *lrow, *lnode;
    int K, E, nlab;
};
__device__ __forceinline__ TgView tg_view(const TargetGraphArgs &G, int b) {
    TgView v;
    const int64_t k0 = (int64_t) b * G.Kmax, r0 = (int64_t) b * (G.Kmax + 1), e0 = (int64_t) b * G.Emax;
    v.label = G.label + k0; v.row = G.row + r0; v.src = G.src + e0; v.tgt = G.tgt + e0;
    v.orow = G.orow + r0; v.oedge = G.oedge + e0; v.lab = G.lab + k0; v.lrow = G.lrow + r0; v.lnode = G.lnode + k0;
    v.K = G.nk[b]; v.nlab = G.nlab[b];
    v.E = v.K > 0 ? v.row[v.K] : 0;
    return v;
}

inline size_t tg_fwd_lds(int elem, int Kmax, int64_t Emax) { return kTgRed + 2 * (size_t) Kmax * elem + (size_t) Emax * (elem + 4); }

inline void tg_set_lds(const void *fn, size_t dyn) {
    if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);
}

}  // namespace

}  // namespace asg
