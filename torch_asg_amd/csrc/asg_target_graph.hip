// torch_asg_amd/csrc/asg_target_graph.hip -- the numerator of an ASG loss whose transcript is "one of these": the log-sum over
// all alignments of all label paths of a small node-labelled TARGET GRAPH that belongs to the utterance (alternative spellings,
// several word-piece segmentations, optional fillers), and its gradients.  asg_graph_loss.hip's recursion with a graph per
// utterance in place of the one product graph of the batch; TargetGraphs.compile (torch_asg_amd/target_graph.py) packs the
// batch into padded arrays [B][Kmax] / [B][Emax] (include/asg_hip.h::asg_target_graphs).  Utterance b, node k of label l_k:
//   f_e            = tr[l_k][l_src_e] + edge_w[e]                 (folded ONCE per utterance, rounded in the dtype)
//   alpha[0][k]    = start_w[k] + I[0][l_k]
//   alpha[t][k]    = lse(stay: alpha[t-1][k] + tr[l_k][l_k];  edge e into k, ascending: alpha[t-1][src_e] + f_e) + I[t][l_k]
//   Z              = lse_k(alpha[len-1][k] + final_w[k])
//   beta[len-1][k] = final_w[k]
//   beta[t-1][k']  = lse(stay: (beta[t][k'] + tr[l_k'][l_k']) + I[t][l_k'];  edge e to k, ascending: (beta[t][k] + f_e) + I[t][l_k])
// Every lse is max-then-sum in that order, -inf (never NaN) when every candidate is -inf.  With g = grad_scores[b]:
//   grad_inputs[t][b][i]  = g * sum_{k of label i, ascending} exp((alpha[t][k] + beta[t][k]) - Z)     (0 for t >= len)
//   grad_transition[i][j] = sum over the batch-wide list of the stays and edges of label pair (i, j), in list order, of
//                           g_b * acc,  acc = sum_{t >= 1} exp((alpha[t-1][src] + candidate) - Z)
//
// Forward and backward: ONE workgroup per utterance, ONE thread per node, the workgroup as wide as the largest graph of the
// batch needs (64, 256 or 1024 threads: a 30-node chain runs in one wavefront, whose barriers cost nothing).  The transition
// matrix is not read in the frame loop: a prologue gathers f_e into LDS (one gather per edge per utterance, not per edge per
// frame) and keeps tr[l_k][l_k] in a register.  alpha / beta ping-pong between two LDS vectors; the emission of the NEXT frame
// is loaded before the barrier of this one, so the global gather sits under the LDS work.  The posterior sums of a node's
// stay and of its outgoing edges are owned by the thread that pulls beta into that node, live in LDS for the whole utterance
// and are written once.  No float atomics, every output element written by a kernel (no memset): bit-identical run to run and
// capturable.  grad_transition: a zero-fill, then one wavefront per label pair that any graph uses.
#include "asg_target_graph_sum.h"

namespace asg {

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Forward.  Dynamic LDS: [reduction slots 256 B][alpha 2*Kmax R][f Emax R][src Emax int].
// ---------------------------------------------------------------------------------------------------------------------
template <typename R, int W>
__global__ void __launch_bounds__(W) target_graph_fwd(Problem P, TargetGraphArgs G, R *A, R *scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    R *red = (R *) lds;
    const R NINF = Num<R>::ninf();
    const int k = threadIdx.x, b = blockIdx.x;
    const TgView g = tg_view(G, b);
    const int len = g.K > 0 ? tg_len(P.in_len, b, P.T) : 0;
    if (len < 1) {                                    // (uniform over the workgroup)
        if (k == 0) scores[b] = NINF;
        return;
    }
    const bool mine = k < g.K;
    const R c = tg_alpha_forward<R>(P, G, g, b, len, lds, A);     // alpha[len-1][k] + final_w[k] (asg_target_graph_sum.h)
    const R m = tg_reduce<R, W, true>(c, red);
    R Z = NINF;
    if (m > NINF) Z = m + tlog(tg_reduce<R, W, false>(mine ? texp(c - m) : R(0), red));
    if (k == 0) scores[b] = Z;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward.  Dynamic LDS: [256 B][beta 2*Kmax R][posterior Kmax R][emission Kmax R][acc (Kmax+Emax) R][f Emax R]
// [target Emax int][lnode Kmax int]; f, target and acc[Kmax + j] in OUTGOING order (j as orow / oedge count).
// ---------------------------------------------------------------------------------------------------------------------
template <typename R, int W>
__global__ void __launch_bounds__(W) target_graph_bwd(Problem P, TargetGraphArgs G, const R *A, const R *Zs, const R *gs,
                                                      R *gin, R *acc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int Kmax = G.Kmax, Emax = G.Emax;
    R *bv = (R *) (lds + kTgRed);
    R *post = bv + 2 * (size_t) Kmax;
    R *emv = post + Kmax;
    R *ac = emv + Kmax;
    R *fo = ac + Kmax + Emax;
    int *to = (int *) (fo + Emax);
    int *ln = to + Emax;
    const R NINF = Num<R>::ninf();
    const int k = threadIdx.x, b = blockIdx.x, T = P.T, N = P.N;
    const int64_t B = P.B;
    const TgView g = tg_view(G, b);
    const int len = g.K > 0 ? tg_len(P.in_len, b, T) : 0;
    const R Z = Zs[b], gb = gs[b];
    const bool ok = len >= 1 && Z > NINF;
    const bool mine = k < g.K;
    R *accb = acc + (int64_t) b * (Kmax + Emax);
    const int t0 = ok ? len : 0;                      // rows from t0 on are zero
    for (int64_t x = k; x < (int64_t) (T - t0) * N; x += W) gin[((int64_t) (t0 + x / N) * B + b) * N + x % N] = R(0);
    if (!ok) {                                        // (uniform) this utterance adds zeros to grad_transition
        if (mine) accb[k] = R(0);
        for (int e = k; e < g.E; e += W) accb[Kmax + e] = R(0);
        return;
    }
    const R *trm = (const R *) P.transition;
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *Ab = A + (int64_t) b * T * Kmax;
    int o0 = 0, o1 = 0, l0 = 0, l1 = 0, li = 0;
    R trs = R(0), a = NINF, em = R(0);
    if (mine) {
        const int lk = g.label[k];
        in += (int64_t) lk * P.is2;
        o0 = g.orow[k]; o1 = g.orow[k + 1];
        const R *ew = (const R *) G.edge_w + (int64_t) b * Emax;
        for (int j = o0; j < o1; ++j) {               // the fold again, through the outgoing CSR
            const int e = g.oedge[j], q = g.tgt[e];
            fo[j] = trm[(int64_t) g.label[q] * P.ts0 + (int64_t) lk * P.ts1] + ew[e];
            to[j] = q;
            ac[Kmax + j] = R(0);
        }
        ac[k] = R(0);
        ln[k] = g.lnode[k];
        trs = trm[(int64_t) lk * (P.ts0 + P.ts1)];
        bv[(size_t) ((len - 1) & 1) * Kmax + k] = ((const R *) G.final_w)[(int64_t) b * Kmax + k];
        a = Ab[(int64_t) (len - 1) * Kmax + k];
        em = in[(int64_t) (len - 1) * P.is0];
    }
    if (k < g.nlab) { l0 = g.lrow[k]; l1 = g.lrow[k + 1]; li = g.lab[k]; }
    __syncthreads();
    for (int t = len - 1; t >= 0; --t) {
        const R *bt = bv + (size_t) (t & 1) * Kmax;
        R ap = NINF;                                  // alpha[t-1][k] and I[t-1][l_k]: in flight across both barriers
        const R emt = em;
        if (mine) {
            if (t >= 1) {
                ap = Ab[(int64_t) (t - 1) * Kmax + k];
                em = in[(int64_t) (t - 1) * P.is0];
            }
            post[k] = texp((a + bt[k]) - Z);
            emv[k] = emt;
        }
        R *row = gin + ((int64_t) t * B + b) * N;
        for (int i = k; i < N; i += W) row[i] = R(0);
        __syncthreads();
        if (k < g.nlab) {                             // one thread per distinct label of the graph
            R s = R(0);
            for (int n = l0; n < l1; ++n) s += post[ln[n]];
            row[li] = gb * s;
        }
        if (mine && t >= 1) {
            const R stay = (bt[k] + trs) + emt;
            R m = stay;
            for (int j = o0; j < o1; ++j) m = tmax(m, (bt[to[j]] + fo[j]) + emv[to[j]]);
            const bool any = m > NINF;
            R s = any ? texp(stay - m) : R(0);
            ac[k] += texp((ap + stay) - Z);
            for (int j = o0; j < o1; ++j) {
                const R c = (bt[to[j]] + fo[j]) + emv[to[j]];
                if (any) s += texp(c - m);
                ac[Kmax + j] += texp((ap + c) - Z);
            }
            bv[(size_t) ((t - 1) & 1) * Kmax + k] = any ? m + tlog(s) : NINF;
        }
        a = ap;
        __syncthreads();
    }
    if (mine) {
        accb[k] = ac[k];
        for (int j = o0; j < o1; ++j) accb[Kmax + g.oedge[j]] = ac[Kmax + j];
    }
}

template <typename R, int W>
hipError_t tg_forward(const Problem &P, const TargetGraphArgs &G, R *A, R *scores, hipStream_t stream) {
    const size_t dyn = tg_fwd_lds(sizeof(R), G.Kmax, G.Emax);
    tg_set_lds((const void *) target_graph_fwd<R, W>, dyn);
    hipLaunchKernelGGL((target_graph_fwd<R, W>), dim3(P.B), dim3(W), dyn, stream, P, G, A, scores);
    return hipGetLastError();
}

template <typename R, int W>
hipError_t tg_backward(const Problem &P, const TargetGraphArgs &G, const R *A, const R *Zs, const R *gs, R *gin, R *acc,
                       hipStream_t stream) {
    const size_t dyn = tg_bwd_lds(sizeof(R), G.Kmax, G.Emax);
    tg_set_lds((const void *) target_graph_bwd<R, W>, dyn);
    hipLaunchKernelGGL((target_graph_bwd<R, W>), dim3(P.B), dim3(W), dyn, stream, P, G, A, Zs, gs, gin, acc);
    return hipGetLastError();
}

}  // namespace

// The largest Emax a batch of Kmax-node graphs may have: what the backward's LDS layout leaves (one bound for both passes, so
// a batch that scores also trains); -1 when not even the vectors fit.
int64_t target_graph_max_edges(int elem, int Kmax) {
    const size_t fixed = tg_bwd_lds(elem, Kmax, 0);
    if (Kmax > kTargetGraphMaxNodes || fixed > kTgLds) return -1;
    return (int64_t) ((kTgLds - fixed) / (2 * (size_t) elem + 4));
}

size_t target_graph_work_bytes(int elem, int T, int B, int Kmax, bool store) {
    return store ? (size_t) T * Kmax * B * elem : 0;
}

size_t target_graph_scratch_bytes(int elem, int B, int Kmax, int64_t Emax) {
    return (size_t) B * ((size_t) Kmax + Emax) * elem;
}

template <typename R>
hipError_t launch_target_graph_forward(const Problem &P, const TargetGraphArgs &G, bool store, void *work, void *scores,
                                       hipStream_t stream) {
    R *A = store ? (R *) work : nullptr, *sc = (R *) scores;
    if (G.Kmax <= 64) return tg_forward<R, 64>(P, G, A, sc, stream);
    if (G.Kmax <= 256) return tg_forward<R, 256>(P, G, A, sc, stream);
    return tg_forward<R, 1024>(P, G, A, sc, stream);
}

template <typename R>
hipError_t launch_target_graph_backward(const Problem &P, const TargetGraphArgs &G, const void *work, const void *scores,
                                        const void *grad_scores, void *grad_inputs, void *grad_transition, void *scratch,
                                        hipStream_t stream) {
    const R *A = (const R *) work, *Zs = (const R *) scores, *gs = (const R *) grad_scores;
    R *gin = (R *) grad_inputs, *gtr = (R *) grad_transition, *acc = (R *) scratch;
    hipError_t e;
    if (G.Kmax <= 64) e = tg_backward<R, 64>(P, G, A, Zs, gs, gin, acc, stream);
    else if (G.Kmax <= 256) e = tg_backward<R, 256>(P, G, A, Zs, gs, gin, acc, stream);
    else e = tg_backward<R, 1024>(P, G, A, Zs, gs, gin, acc, stream);
    if (e != hipSuccess) return e;
    return tg_grad_transition<R, true>(P, G, (const R *) acc, gs, gtr, stream);
}

template hipError_t launch_target_graph_forward<float>(const Problem &, const TargetGraphArgs &, bool, void *, void *, hipStream_t);
template hipError_t launch_target_graph_forward<double>(const Problem &, const TargetGraphArgs &, bool, void *, void *, hipStream_t);
template hipError_t launch_target_graph_backward<float>(const Problem &, const TargetGraphArgs &, const void *, const void *,
                                                        const void *, void *, void *, void *, hipStream_t);
template hipError_t launch_target_graph_backward<double>(const Problem &, const TargetGraphArgs &, const void *, const void *,
                                                         const void *, void *, void *, void *, hipStream_t);

}  // namespace asg
