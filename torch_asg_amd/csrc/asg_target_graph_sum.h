// torch_asg_amd/csrc/asg_target_graph_sum.h -- what the two log-sum units over per-utterance target graphs share
// (asg_target_graph.hip: the score of a graph and its gradients; asg_target_graph_final.hip: the score of every final node and
// their gradients): the alpha frame loop, written ONCE, and the two grad_transition kernels.
#pragma once
#include "asg_target_graph_common.h"

namespace asg {

namespace {

constexpr int kTgF = 256;                       // workgroup of the two grad_transition kernels

template <typename R> __device__ __forceinline__ R texp(R x);
template <> __device__ __forceinline__ float texp<float>(float x) { return expf(x); }
template <> __device__ __forceinline__ double texp<double>(double x) { return ::exp(x); }
template <typename R> __device__ __forceinline__ R tlog(R x);
template <> __device__ __forceinline__ float tlog<float>(float x) { return logf(x); }
template <> __device__ __forceinline__ double tlog<double>(double x) { return ::log(x); }

// The forward of utterance b over len >= 1 frames (uniform over the workgroup), thread k = node k.  Dynamic LDS behind the
// reduction slots: [alpha 2*Kmax R][f Emax R][src Emax int] (tg_fwd_lds).  The prologue gathers f_e into LDS (one gather per
// edge per utterance) and keeps tr[l_k][l_k] in a register; alpha ping-pongs between two LDS vectors; the emission of the NEXT
// frame is loaded before the barrier of this one.  With A, alpha[t][k] goes to A[b][t][k].  Returns alpha[len-1][k] +
// final_w[k] (-inf for k >= K); every thread is behind the last frame's barrier.
template <typename R>
__device__ __forceinline__ R tg_alpha_forward(const Problem &P, const TargetGraphArgs &G, const TgView &g, int b, int len,
                                              unsigned char *lds, R *A) {
    R *av = (R *) (lds + kTgRed);
    R *fe = av + 2 * (size_t) G.Kmax;
    int *se = (int *) (fe + G.Emax);
    const R NINF = Num<R>::ninf();
    const int k = threadIdx.x, T = P.T, Kmax = G.Kmax;
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
    }
    R *Ab = A ? A + (int64_t) b * T * Kmax : nullptr;
    if (mine && Ab) Ab[k] = x;
    __syncthreads();
    for (int t = 1; t < len; ++t) {
        const R *vp = av + (size_t) ((t - 1) & 1) * Kmax;
        if (mine) {
            const R emt = em;
            if (t + 1 < len) em = in[(int64_t) (t + 1) * P.is0];     // next frame's emission: in flight across the barrier
            const R stay = vp[k] + trs;
            R m = stay;
            for (int e = e0; e < e1; ++e) m = tmax(m, vp[se[e]] + fe[e]);
            x = NINF;
            if (m > NINF) {
                R s = texp(stay - m);
                for (int e = e0; e < e1; ++e) s += texp((vp[se[e]] + fe[e]) - m);
                x = (m + tlog(s)) + emt;
            }
            av[(size_t) (t & 1) * Kmax + k] = x;
            if (Ab) Ab[(int64_t) t * Kmax + k] = x;
        }
        __syncthreads();
    }
    return mine ? x + fin : NINF;                     // x = alpha[len-1][k]
}

// ---------------------------------------------------------------------------------------------------------------------
// grad_transition: zeros everywhere, then a wavefront per label pair that some graph of the batch uses; the lanes stride
// the pair's segment of the batch-wide list in list order and end in a fixed butterfly.  WEIGHT: each entry times gs[b]
// (the score of a graph); without it the per-utterance weights are already inside acc (the scores of the final nodes).
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kTgF) target_graph_tr_zero(R *gtr, int64_t n) {
    const int64_t x = (int64_t) blockIdx.x * kTgF + threadIdx.x;
    if (x < n) gtr[x] = R(0);
}

template <typename R, bool WEIGHT>
__global__ void __launch_bounds__(kTgF) target_graph_tr_reduce(TargetGraphArgs G, const R *acc, const R *gs, R *gtr) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t pair = (int64_t) blockIdx.x * (kTgF / 64) + w;
    if (pair >= G.npairs) return;
    const int slots = G.Kmax + G.Emax;
    R s = R(0);
    for (int x = G.pseg[pair] + lane, x1 = G.pseg[pair + 1]; x < x1; x += 64) {
        const int at = G.pslot[x];                    // b * (Kmax + Emax) + slot
        s += WEIGHT ? gs[at / slots] * acc[at] : acc[at];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += (R) __shfl_xor(s, o);
    if (lane == 0) gtr[G.pkey[pair]] = s;
}

// the zero-fill of grad_transition [N,N] and the reduction of acc [B][Kmax + Emax] into it
template <typename R, bool WEIGHT>
hipError_t tg_grad_transition(const Problem &P, const TargetGraphArgs &G, const R *acc, const R *gs, R *gtr, hipStream_t stream) {
    const int64_t NN = (int64_t) P.N * P.N;
    hipLaunchKernelGGL((target_graph_tr_zero<R>), dim3((unsigned) ((NN + kTgF - 1) / kTgF)), dim3(kTgF), 0, stream, gtr, NN);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || G.npairs == 0) return e;
    hipLaunchKernelGGL((target_graph_tr_reduce<R, WEIGHT>), dim3((unsigned) ((G.npairs + kTgF / 64 - 1) / (kTgF / 64))),
                       dim3(kTgF), 0, stream, G, acc, gs, gtr);
    return hipGetLastError();
}

inline size_t tg_bwd_lds(int elem, int Kmax, int64_t Emax) {
    return kTgRed + (size_t) Kmax * (5 * elem + 4) + (size_t) Emax * (2 * elem + 4);
}

}  // namespace

}  // namespace asg
