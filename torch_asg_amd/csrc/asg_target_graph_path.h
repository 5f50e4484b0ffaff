// torch_asg_amd/csrc/asg_target_graph_path.h -- what the three path kernels over per-utterance target graphs share
// (asg_target_graph_viterbi.hip: the best path; asg_target_graph_nbest.hip: the best path into every final node, ranked;
// asg_target_graph_hard.hip: the best path's score as a training criterion): the max-plus forward with its back-pointer rows,
// written ONCE, and the staging of those rows into LDS for the walk back.
#pragma once
#include "asg_target_graph_common.h"

namespace asg {

namespace {

// frames per staged block, and the 16-byte granules one thread moves per block: F * Kmax elements + up to 7 in front of
// them (the block need not start on a 16-byte boundary) + the tail
template <int W> struct Tgv {
    static constexpr int F = W == 1024 ? 16 : 64;
    static constexpr int NG = ((F * W + 14) / 8 + W - 1) / W;
};
inline int tgv_frames(int Kmax) { return Kmax <= 256 ? 64 : 16; }
inline size_t tgv_granules(int Kmax) { return ((size_t) tgv_frames(Kmax) * Kmax + 14) / 8; }
// LDS of a workgroup that runs the forward and then walks one path: [reduction slots 256 B] then the larger of the forward's
// [v 2*Kmax R][f Emax R][src Emax int] and the backtrace's [stage 2 x granules x 16 B][line 2 x F int]
inline size_t tgv_lds(int elem, int Kmax, int64_t Emax) {
    const size_t back = kTgRed + 2 * tgv_granules(Kmax) * 16 + 2 * (size_t) tgv_frames(Kmax) * 4;
    const size_t fwd = tg_fwd_lds(elem, Kmax, Emax);
    return fwd > back ? fwd : back;
}

// n elements from `rows` into registers: granule g of the enclosing 16-byte-aligned range belongs to thread g mod W.
template <int W>
__device__ __forceinline__ void tgv_fetch(const uint16_t *rows, int n, uint4 (&r)[Tgv<W>::NG]) {
    const int mis = (int) (((uintptr_t) rows & 15) >> 1), total = (mis + n + 7) >> 3;
#pragma unroll
    for (int q = 0; q < Tgv<W>::NG; ++q) {
        const int g = (int) threadIdx.x + q * W, lo = g * 8 - mis;
        if (g >= total) continue;
        if (lo >= 0 && lo + 8 <= n) {
            r[q] = *(const uint4 *) (rows + lo);
        } else {                                      // the first or the last granule: nothing outside the block is read
            unsigned h[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = (lo + j >= 0 && lo + j < n) ? rows[lo + j] : 0u;
            r[q] = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
        }
    }
}

template <int W>
__device__ __forceinline__ void tgv_put(const uint16_t *rows, int n, const uint4 (&r)[Tgv<W>::NG], uint4 *stage) {
    const int mis = (int) (((uintptr_t) rows & 15) >> 1), total = (mis + n + 7) >> 3;
#pragma unroll
    for (int q = 0; q < Tgv<W>::NG; ++q) {
        const int g = (int) threadIdx.x + q * W;
        if (g < total) stage[g] = r[q];
    }
}

// The forward of utterance b over len >= 1 frames (uniform over the workgroup), thread k = node k: the score's prologue (f_e
// and the sources folded into LDS behind the reduction slots, tr[l_k][l_k] in a register), v ping-pongs between two LDS
// vectors, the next emission is loaded before the barrier.  ONE pass over the incoming edges carries (best value, best
// source) in registers, and the winning source goes to bpb[t][k] as 16 bits, a frame's row one coalesced store.  Returns
// end[k] = v[len-1][k] + final_w[k] (-inf for k >= K); every thread is behind the last frame's barrier, so the LDS is free.
// BP = false (a score that nobody walks back: asg_target_graph_hard.hip without a gradient) drops the stores; bpb is not read.
template <typename R, bool BP = true>
__device__ __forceinline__ R tgv_forward(const Problem &P, const TargetGraphArgs &G, const TgView &g, int b, int len,
                                         unsigned char *lds, uint16_t *bpb) {
    const int k = threadIdx.x, Kmax = G.Kmax;
    R *av = (R *) (lds + kTgRed);
    R *fe = av + 2 * (size_t) Kmax;
    int *se = (int *) (fe + G.Emax);
    const R NINF = Num<R>::ninf();
    const bool mine = k < g.K;
    const R *trm = (const R *) P.transition;
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    int e0 = 0, e1 = 0;
    R trs = R(0), fin = NINF, em = R(0), x = NINF;
    if (mine) {
        const int lk = g.label[k];
        in += (int64_t) lk * P.is2;
        e0 = g.row[k]; e1 = g.row[k + 1];
        const R *ew = (const R *) G.edge_w + (int64_t) b * G.Emax;
        for (int e = e0; e < e1; ++e) {               // the fold: one gather per edge per utterance
            const int s = g.src[e];
            fe[e] = trm[(int64_t) lk * P.ts0 + (int64_t) g.label[s] * P.ts1] + ew[e];
            se[e] = s;
        }
        trs = trm[(int64_t) lk * (P.ts0 + P.ts1)];
        fin = ((const R *) G.final_w)[(int64_t) b * Kmax + k];
        x = ((const R *) G.start_w)[(int64_t) b * Kmax + k] + in[0];
        if (len > 1) em = in[P.is0];
        av[k] = x;
        if (BP) bpb[k] = (uint16_t) k;                // (row 0 is never followed; written so that a staged block holds no stale bytes)
    }
    __syncthreads();
    for (int t = 1; t < len; ++t) {
        const R *vp = av + (size_t) ((t - 1) & 1) * Kmax;
        if (mine) {
            const R emt = em;
            if (t + 1 < len) em = in[(int64_t) (t + 1) * P.is0];         // next frame's emission: in flight across the barrier
            R best = vp[k] + trs;                     // stay wins ties
            int from = k;
            for (int e = e0; e < e1; ++e) {
                const int s = se[e];
                const R c = vp[s] + fe[e];
                if (c > best) { best = c; from = s; }
            }
            x = best + emt;
            av[(size_t) (t & 1) * Kmax + k] = x;
            if (BP) bpb[(int64_t) t * Kmax + k] = (uint16_t) from;
        }
        __syncthreads();
    }
    return mine ? x + fin : NINF;                     // x = v[len-1][k]
}

}  // namespace

}  // namespace asg
