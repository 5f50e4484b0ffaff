// torch_asg_amd/csrc/asg_target_graph_conf.hip -- how sure the best path of a per-utterance target graph is of itself: the
// confidence of every token of asg_target_graph_viterbi.hip's path and the posterior of every final node, under the sum over
// all paths of asg_target_graph.hip.  Utterance b, len = clamp(input_lengths[b], 0, T); alpha, beta, f_e and Z are
// asg_target_graph.hip's, in the dtype of the problem:
//   P(i, 0)      = sum over the nodes k of label i of exp((alpha[0][k] + beta[0][k]) - Z)
//   P(i, t >= 1) = sum over the edges e into nodes k of label i of exp((alpha[t-1][src_e] + ((beta[t][k] + f_e) + I[t][l_k])) - Z)
//                  -- "a token of label i starts at frame t"; the stay starts none (and no edge joins two nodes of one label)
//   token_confidences[b][j] = sum of P(tokens[b][j], t) over |t - token_frames[b][j]| <= tol, t in [0, len-1]
//   final_posteriors[b][k]  = exp((alpha[len-1][k] + final_w[k]) - Z)
// An utterance whose Z is -inf (len 0, empty graph, no finite path) gets zeros, never a NaN.
//
// The call is three launches: target_graph_fwd with alpha stored (Z is target_graph_score's), target_graph_viterbi (the
// hypothesis: tokens, token_frames, token_lengths), then target_graph_conf below -- one workgroup per utterance, one thread
// per node, 64 / 256 / 1024 threads wide as the other two.  It pulls beta from len-1 down to 0 through the OUTGOING CSR with
// target_graph_bwd's adds in target_graph_bwd's order: f_e and the targets folded into LDS once, beta in two LDS vectors,
// the frame's emissions published in LDS, alpha[t-1][k] and the next emission loaded ahead of the barrier.  What the
// backward spends on label posteriors, the [T,B,N] gradient and the per-edge accumulators is not here.  The thread of node
// k owns the events of k's outgoing edges (their alpha is its own) and, at frame 0, its own start term.  An event goes to
// HypSink (asg_beam_conf_sink.h): the tokens whose window holds the frame are one index range because token_frames ascends
// strictly; a token's accumulator is a 64-bit fixed-point slot (2^54) of a ring of 256 in LDS, integer adds only, and no
// exp is formed while the range is empty.  Dynamic LDS:
//   [ring 256 x 8 B][beta 2*Kmax R][emission Kmax R][f Emax R][target Emax int][label Kmax int]
// = 2048 + Kmax * (3e + 4) + Emax * (e + 4) bytes, against the backward's 256 + Kmax * (5e + 4) + Emax * (2e + 4): it fits
// wherever that does (tgc_lds below).  Every output element is written here (no memset), no float atomics, nothing
// synchronises the host: bit-identical run to run and capturable.
#include "asg_target_graph_common.h"
#include "asg_beam_conf_sink.h"   // HypSink, the ring and 2^54; bexp / blog / bmax are texp / tlog / tmax of asg_target_graph.hip

namespace asg {

namespace {

static_assert(kTargetGraphConfMaxTol == kBeamWordConfMaxTol, "the ring of HypSink is sized by the word call's tolerance");

constexpr size_t kTgcRing = (size_t) kConfRing * sizeof(unsigned long long);

// With x = Kmax * 2e + Emax * e this is (the backward's request) - x + (2048 - 256).  x >= 1792: not above the backward's.
// x < 1792: Kmax * (3e + 4) + Emax * (e + 4) <= 2x (e >= 4), so the request stays below 2048 + 3584 bytes.  Either way a
// batch within target_graph_max_edges is within kTgLds here.
inline size_t tgc_lds(int elem, int Kmax, int64_t Emax) {
    return kTgcRing + (size_t) Kmax * (3 * elem + 4) + (size_t) Emax * (elem + 4);
}

template <typename R, int W>
__global__ void __launch_bounds__(W) target_graph_conf(Problem P, TargetGraphArgs G, const R *A, const R *Zs, const long long *tokens,
                                                       const long long *frames, const long long *tlen, int tol, R *conf, R *fpost) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int Kmax = G.Kmax, Emax = G.Emax;
    unsigned long long *ring = (unsigned long long *) lds;
    R *bv = (R *) (lds + kTgcRing);
    R *emv = bv + 2 * (size_t) Kmax;
    R *fo = emv + Kmax;
    int *to = (int *) (fo + Emax);
    int *lb = to + Emax;
    const R NINF = Num<R>::ninf();
    const int k = threadIdx.x, b = blockIdx.x, T = P.T;
    const TgView g = tg_view(G, b);
    const int len = g.K > 0 ? tg_len(P.in_len, b, T) : 0;
    const R Z = Zs[b];
    const bool ok = len >= 1 && Z > NINF;
    const bool mine = k < g.K;
    int n = ok ? (int) tlen[b] : 0;                   // the tokens of the hypothesis
    n = n < 0 ? 0 : (n > len ? len : n);
    R *cf = conf + (int64_t) b * T;
    for (int j = n + k; j < T; j += W) cf[j] = R(0);
    if (!ok) {                                        // (uniform)
        if (k < Kmax) fpost[(int64_t) b * Kmax + k] = R(0);
        return;
    }
    const R *trm = (const R *) P.transition;
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *Ab = A + (int64_t) b * T * Kmax;
    int o0 = 0, o1 = 0, lk = 0;
    R trs = R(0), a = NINF, em = R(0), post = R(0);
    if (mine) {
        lk = g.label[k];
        in += (int64_t) lk * P.is2;
        o0 = g.orow[k]; o1 = g.orow[k + 1];
        const R *ew = (const R *) G.edge_w + (int64_t) b * Emax;
        for (int j = o0; j < o1; ++j) {               // the backward's fold, through the outgoing CSR
            const int e = g.oedge[j], q = g.tgt[e];
            fo[j] = trm[(int64_t) g.label[q] * P.ts0 + (int64_t) lk * P.ts1] + ew[e];
            to[j] = q;
        }
        lb[k] = lk;
        trs = trm[(int64_t) lk * (P.ts0 + P.ts1)];
        const R fin = ((const R *) G.final_w)[(int64_t) b * Kmax + k];
        bv[(size_t) ((len - 1) & 1) * Kmax + k] = fin;
        a = Ab[(int64_t) (len - 1) * Kmax + k];
        em = in[(int64_t) (len - 1) * P.is0];
        post = bexp((a + fin) - Z);
    }
    if (k < Kmax) fpost[(int64_t) b * Kmax + k] = post;
    for (int x = k; x < kConfRing; x += W) ring[x] = 0ull;
    HypSink<R> sink;
    sink.wd = tokens + (int64_t) b * T; sink.wf = frames + (int64_t) b * T; sink.cf = cf; sink.ring = ring; sink.tol = tol;
    sink.ka = sink.kb = n;
    __syncthreads();
    for (int t = len - 1; t >= 1; --t) {
        const R *bt = bv + (size_t) (t & 1) * Kmax;
        R ap = NINF;                                  // alpha[t-1][k] and I[t-1][l_k]: in flight across both barriers
        const R emt = em;
        if (mine) {
            ap = Ab[(int64_t) (t - 1) * Kmax + k];
            em = in[(int64_t) (t - 1) * P.is0];
            emv[k] = emt;
        }
        sink.window(t);                               // (the adds of frame t + 1 are behind the barrier that ended it)
        const bool open = sink.open();
        __syncthreads();
        if (mine) {
            const R stay = (bt[k] + trs) + emt;
            R m = stay;
            for (int j = o0; j < o1; ++j) m = bmax(m, (bt[to[j]] + fo[j]) + emv[to[j]]);
            R nb = NINF;
            if (m > NINF) {                           // (every candidate -inf: every event of this node is 0)
                R s = bexp(stay - m);
                for (int j = o0; j < o1; ++j) {
                    const int q = to[j];
                    const R c = (bt[q] + fo[j]) + emv[q];
                    s += bexp(c - m);
                    if (open) sink.add(lb[q], (ap + c) - Z);
                }
                nb = m + blog(s);
            }
            bv[(size_t) ((t - 1) & 1) * Kmax + k] = nb;
        }
        a = ap;
        __syncthreads();
    }
    sink.window(0);                                   // frame 0: every node starts a token with its label
    if (mine && sink.open()) sink.add(lk, (a + bv[k]) - Z);
    __syncthreads();
    // every window is closed, a frame at a time: HypSink finishes the tokens that leave in strides of 1024 threads, and a
    // step of one frame finishes at most one
    for (int t = -1; t >= -tol - 1; --t) sink.window(t);
}

template <typename R, int W>
hipError_t tgc_launch(const Problem &P, const TargetGraphArgs &G, int tol, const void *alpha, const void *Zs,
                      const int64_t *tokens, const int64_t *frames, const int64_t *tlen, void *conf, void *fpost,
                      hipStream_t stream) {
    const size_t dyn = tgc_lds(sizeof(R), G.Kmax, G.Emax);
    tg_set_lds((const void *) target_graph_conf<R, W>, dyn);
    hipLaunchKernelGGL((target_graph_conf<R, W>), dim3(P.B), dim3(W), dyn, stream, P, G, (const R *) alpha, (const R *) Zs,
                       (const long long *) tokens, (const long long *) frames, (const long long *) tlen, tol, (R *) conf,
                       (R *) fpost);
    return hipGetLastError();
}

}  // namespace

template <typename R>
hipError_t launch_target_graph_conf(const Problem &P, const TargetGraphArgs &G, int tol, const void *alpha,
                                    const void *normalisers, const int64_t *tokens, const int64_t *token_frames,
                                    const int64_t *token_lengths, void *token_confidences, void *final_posteriors,
                                    hipStream_t stream) {
    if (G.Kmax <= 64)
        return tgc_launch<R, 64>(P, G, tol, alpha, normalisers, tokens, token_frames, token_lengths, token_confidences,
                                 final_posteriors, stream);
    if (G.Kmax <= 256)
        return tgc_launch<R, 256>(P, G, tol, alpha, normalisers, tokens, token_frames, token_lengths, token_confidences,
                                  final_posteriors, stream);
    return tgc_launch<R, 1024>(P, G, tol, alpha, normalisers, tokens, token_frames, token_lengths, token_confidences,
                               final_posteriors, stream);
}

template hipError_t launch_target_graph_conf<float>(const Problem &, const TargetGraphArgs &, int, const void *, const void *,
                                                    const int64_t *, const int64_t *, const int64_t *, void *, void *, hipStream_t);
template hipError_t launch_target_graph_conf<double>(const Problem &, const TargetGraphArgs &, int, const void *, const void *,
                                                     const int64_t *, const int64_t *, const int64_t *, void *, void *, hipStream_t);

}  // namespace asg
