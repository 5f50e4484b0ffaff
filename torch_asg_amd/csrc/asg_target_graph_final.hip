// torch_asg_amd/csrc/asg_target_graph_final.hip -- the score of EVERY FINAL NODE of a per-utterance target graph, each summed
// over all alignments, and the gradient of any signed combination of them: what a sequence-discriminative criterion over an
// n-best list needs (minimum word error rate / minimum Bayes risk, pairwise ranking), where asg_target_graph.hip collapses the
// finals into one log-sum.  alpha, f_e and len are asg_target_graph.hip's, bit for bit (ONE frame loop: asg_target_graph_sum.h):
//   final_scores[b][k] = alpha[len-1][k] + final_w[k]          (-inf, never NaN: k >= K_b, final_w -inf, len 0, no path to k)
// Backward, with g = grad_final_scores [B][Kmax] (entries where final_scores is -inf are ignored, NaN included): reverse mode
// through the alpha recursion in the LINEAR domain -- a log-semiring beta pass cannot carry signed weights.  d[t][k] is the
// derivative of sum_k g_k * final_scores_k by alpha[t][k]:
//   d[len-1][k] = g[b][k] where final_scores[b][k] > -inf, else 0
//   q[t][k]     = I[t][l_k] - alpha[t][k]                                 (-inf where alpha[t][k] is -inf: every weight into k is 0)
//   w_stay      = exp((alpha[t-1][j] + q[t][j]) + tr[l_j][l_j])
//   w_e         = exp((alpha[t-1][j] + q[t][k]) + f_e)                     (edge e: j -> k)
//   d[t-1][j]   = d[t][j] * w_stay + sum over the edges out of j, ascending by target, of d[t][k] * w_e
//   acc_stay[j] += d[t][j] * w_stay,   acc_e += d[t][k] * w_e
//   grad_inputs[t][b][i]  = sum_{k of label i, ascending} d[t][k]          (0 for t >= len)
//   grad_transition[i][j] = sum over the batch-wide list pslot of label pair (i, j), in list order, of acc (no further factor)
// The order inside the exponent: alpha[t-1][j] + q[t][k] first.  The two are large and of opposite sign, their sum is small and
// carries (almost) no rounding of its own; the small f_e comes last.  What is left is the rounding of q (half an ulp of
// alpha) beside the rounding that the stored alpha itself carries: the weights into a node sum to 1 only to that precision.
//
// Forward: the shared frame loop, then every thread k < Kmax writes its own score (no workgroup log-sum, no memset).
// Backward: ONE workgroup per utterance, ONE thread per node, 64 / 256 / 1024 wide.  Dynamic LDS: [256 B][d 2*Kmax R]
// [q 2*Kmax R][acc Emax R][f Emax R][target Emax int][lnode Kmax int]; f, target and acc in OUTGOING order, f folded once per
// utterance.  256 + Kmax (4 e + 4) + Emax (2 e + 4) bytes: under asg_target_graph.hip's backward layout, whose bound
// (target_graph_max_edges) therefore holds here too.  Thread k publishes d[t][k] and q[t][k]; thread j pulls over its outgoing
// CSR: ONE exp per edge and frame and no log.  The stay's sum lives in a register of its thread, the edges' sums in LDS for
// the whole utterance; both are written once.  ONE barrier per frame: d and q ping-pong, so frame t - 1 publishes into the
// buffer that nobody has read since frame t + 1, and every thread has passed frame t's barrier -- which lies behind its reads
// of frame t + 1 -- before any thread writes that buffer again.  alpha[t-1][k] and the next emission are loaded before the
// barrier.  Label rows: one thread per distinct label in lnode order.  No float atomics, every output element written by a
// kernel (no memset), nothing synchronises: bit-identical run to run and capturable.
#include "asg_target_graph_sum.h"

namespace asg {

namespace {

template <typename R, int W>
__global__ void __launch_bounds__(W) target_graph_final_fwd(Problem P, TargetGraphArgs G, R *A, R *fs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int k = threadIdx.x, b = blockIdx.x;
    const TgView g = tg_view(G, b);
    const int len = g.K > 0 ? tg_len(P.in_len, b, P.T) : 0;
    R c = Num<R>::ninf();
    if (len >= 1) c = tg_alpha_forward<R>(P, G, g, b, len, lds, A);      // (uniform over the workgroup)
    if (k < G.Kmax) fs[(int64_t) b * G.Kmax + k] = c;
}

inline size_t tgf_bwd_lds(int elem, int Kmax, int64_t Emax) {
    return kTgRed + (size_t) Kmax * (4 * elem + 4) + (size_t) Emax * (2 * elem + 4);
}

template <typename R, int W>
__global__ void __launch_bounds__(W) target_graph_final_bwd(Problem P, TargetGraphArgs G, const R *A, const R *fs, const R *gf,
                                                            R *gin, R *acc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int Kmax = G.Kmax, Emax = G.Emax;
    R *dv = (R *) (lds + kTgRed);
    R *qv = dv + 2 * (size_t) Kmax;
    R *ac = qv + 2 * (size_t) Kmax;
    R *fo = ac + Emax;
    int *to = (int *) (fo + Emax);
    int *ln = to + Emax;
    const R NINF = Num<R>::ninf();
    const int k = threadIdx.x, b = blockIdx.x, T = P.T, N = P.N;
    const int64_t B = P.B;
    const TgView g = tg_view(G, b);
    const int len = g.K > 0 ? tg_len(P.in_len, b, T) : 0;
    const bool mine = k < g.K;
    R *accb = acc + (int64_t) b * (Kmax + Emax);
    for (int64_t x = k; x < (int64_t) (T - len) * N; x += W) gin[((int64_t) (len + x / N) * B + b) * N + x % N] = R(0);
    if (len < 1) {                                    // (uniform) this utterance adds zeros to grad_transition
        if (mine) accb[k] = R(0);
        for (int e = k; e < g.E; e += W) accb[Kmax + e] = R(0);
        return;
    }
    const R *trm = (const R *) P.transition;
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *Ab = A + (int64_t) b * T * Kmax;
    int o0 = 0, o1 = 0, l0 = 0, l1 = 0, li = 0;
    R trs = R(0), a = NINF, em = R(0), d = R(0), sacc = R(0);
    if (mine) {
        const int lk = g.label[k];
        in += (int64_t) lk * P.is2;
        o0 = g.orow[k]; o1 = g.orow[k + 1];
        const R *ew = (const R *) G.edge_w + (int64_t) b * Emax;
        for (int j = o0; j < o1; ++j) {               // the fold, through the outgoing CSR
            const int e = g.oedge[j], q = g.tgt[e];
            fo[j] = trm[(int64_t) g.label[q] * P.ts0 + (int64_t) lk * P.ts1] + ew[e];
            to[j] = q;
            ac[j] = R(0);
        }
        ln[k] = g.lnode[k];
        trs = trm[(int64_t) lk * (P.ts0 + P.ts1)];
        if (fs[(int64_t) b * Kmax + k] > NINF) d = gf[(int64_t) b * Kmax + k];      // g is ignored where the score is -inf
        a = Ab[(int64_t) (len - 1) * Kmax + k];
        em = in[(int64_t) (len - 1) * P.is0];
    }
    if (k < g.nlab) { l0 = g.lrow[k]; l1 = g.lrow[k + 1]; li = g.lab[k]; }
    for (int t = len - 1; t >= 0; --t) {
        R *dt = dv + (size_t) (t & 1) * Kmax, *qt = qv + (size_t) (t & 1) * Kmax;
        R ap = NINF;                                  // alpha[t-1][k] and I[t-1][l_k]: in flight across the barrier
        const R qk = a > NINF ? em - a : NINF;
        if (mine) {
            if (t >= 1) {
                ap = Ab[(int64_t) (t - 1) * Kmax + k];
                em = in[(int64_t) (t - 1) * P.is0];
            }
            dt[k] = d;
            qt[k] = qk;
        }
        R *row = gin + ((int64_t) t * B + b) * N;
        for (int i = k; i < N; i += W) row[i] = R(0);
        __syncthreads();                              // the only barrier of the frame (the prologue's LDS is behind it too)
        if (k < g.nlab) {                             // one thread per distinct label of the graph
            R s = R(0);
            for (int n = l0; n < l1; ++n) s += dt[ln[n]];
            row[li] = s;
        }
        if (mine && t >= 1) {
            R c = d * texp((ap + qk) + trs);
            sacc += c;
            R nd = c;
            for (int j = o0; j < o1; ++j) {
                c = dt[to[j]] * texp((ap + qt[to[j]]) + fo[j]);
                ac[j] += c;
                nd += c;
            }
            d = nd;
        }
        a = ap;
    }
    if (mine) {
        accb[k] = sacc;
        for (int j = o0; j < o1; ++j) accb[Kmax + g.oedge[j]] = ac[j];
    }
}

template <typename R, int W>
hipError_t tgf_forward(const Problem &P, const TargetGraphArgs &G, R *A, R *fs, hipStream_t stream) {
    const size_t dyn = tg_fwd_lds(sizeof(R), G.Kmax, G.Emax);
    tg_set_lds((const void *) target_graph_final_fwd<R, W>, dyn);
    hipLaunchKernelGGL((target_graph_final_fwd<R, W>), dim3(P.B), dim3(W), dyn, stream, P, G, A, fs);
    return hipGetLastError();
}

template <typename R, int W>
hipError_t tgf_backward(const Problem &P, const TargetGraphArgs &G, const R *A, const R *fs, const R *gf, R *gin, R *acc,
                        hipStream_t stream) {
    const size_t dyn = tgf_bwd_lds(sizeof(R), G.Kmax, G.Emax);
    tg_set_lds((const void *) target_graph_final_bwd<R, W>, dyn);
    hipLaunchKernelGGL((target_graph_final_bwd<R, W>), dim3(P.B), dim3(W), dyn, stream, P, G, A, fs, gf, gin, acc);
    return hipGetLastError();
}

}  // namespace

template <typename R>
hipError_t launch_target_graph_final_forward(const Problem &P, const TargetGraphArgs &G, bool store, void *work,
                                             void *final_scores, hipStream_t stream) {
    R *A = store ? (R *) work : nullptr, *fs = (R *) final_scores;
    if (G.Kmax == 0) return hipSuccess;               // [B,0]: nothing to write
    if (G.Kmax <= 64) return tgf_forward<R, 64>(P, G, A, fs, stream);
    if (G.Kmax <= 256) return tgf_forward<R, 256>(P, G, A, fs, stream);
    return tgf_forward<R, 1024>(P, G, A, fs, stream);
}

template <typename R>
hipError_t launch_target_graph_final_backward(const Problem &P, const TargetGraphArgs &G, const void *work,
                                              const void *final_scores, const void *grad_final_scores, void *grad_inputs,
                                              void *grad_transition, void *scratch, hipStream_t stream) {
    static_assert(sizeof(R) == 4 || sizeof(R) == 8, "float or double");
    const R *A = (const R *) work, *fs = (const R *) final_scores, *gf = (const R *) grad_final_scores;
    R *gin = (R *) grad_inputs, *gtr = (R *) grad_transition, *acc = (R *) scratch;
    hipError_t e;
    if (G.Kmax <= 64) e = tgf_backward<R, 64>(P, G, A, fs, gf, gin, acc, stream);
    else if (G.Kmax <= 256) e = tgf_backward<R, 256>(P, G, A, fs, gf, gin, acc, stream);
    else e = tgf_backward<R, 1024>(P, G, A, fs, gf, gin, acc, stream);
    if (e != hipSuccess) return e;
    return tg_grad_transition<R, false>(P, G, (const R *) acc, (const R *) nullptr, gtr, stream);
}

template hipError_t launch_target_graph_final_forward<float>(const Problem &, const TargetGraphArgs &, bool, void *, void *,
                                                             hipStream_t);
template hipError_t launch_target_graph_final_forward<double>(const Problem &, const TargetGraphArgs &, bool, void *, void *,
                                                              hipStream_t);
template hipError_t launch_target_graph_final_backward<float>(const Problem &, const TargetGraphArgs &, const void *, const void *,
                                                              const void *, void *, void *, void *, hipStream_t);
template hipError_t launch_target_graph_final_backward<double>(const Problem &, const TargetGraphArgs &, const void *, const void *,
                                                               const void *, void *, void *, void *, hipStream_t);

}  // namespace asg
