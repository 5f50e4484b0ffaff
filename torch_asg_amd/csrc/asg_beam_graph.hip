// torch_asg_amd/csrc/asg_beam_graph.hip -- BEAM-PRUNED Viterbi decoding over the ASG lattice composed with a token automaton,
// on gfx950.  The product graph of asg_decode_graph.hip, read from the SOURCE side (TokenGraph.compile_beam: a CSR of outgoing
// edges per product state with {target, label of the target} and the folded weight side by side, and the list of start states).
// The search is specified, not approximate (include/asg_hip.h::asg_beam_decode_graph): the candidates of frame t come only from
// the active set of frame t-1, the best candidate of a target is the largest value with the smallest source index, and the new
// active set is the first K candidate states in (value descending, q ascending) order whose value is >= fl(max - threshold).
// Adds, one subtraction and comparisons only; integer atomics only: results are bit-identical run to run and to the numpy
// restatement (tests/beam_decode_ref.py).
//
// ONE launch, one 1024-thread workgroup per utterance walks the frames; the active set (q, value) lives in LDS.  Per frame:
//   expand A   G lanes per active state stride over its outgoing row (lane 0 adds the stay).  A candidate value becomes an
//              order-preserving unsigned key and goes into the utterance's slot array val[Q] with an integer atomicMax (0 = empty);
//              the lanes that found the slot empty append the target to the touched list (one LDS counter bump per wavefront).
//   expand B   the same candidates again: the ones whose key equals the slot's maximum put (source q << 16 | source slot) into
//              arg[Q] with a 64-bit atomicMin -- the smallest source among the tied, with its slot in the previous beam for the
//              back-pointer.  Max and min are order independent: the winner is the specified one whatever the timing.  (Two
//              phases rather than one (value, source) key because a float64 value already fills the 64 bits an atomic has.)
//   select     walk the touched list: c = value + emission as a key beside the list (0: not a candidate); the maximum m and the
//              minimum; lo = fl(m - threshold).  If more than K keys pass lo, a radix select over LDS histograms (8-bit digits,
//              starting below the bits that m and the minimum share) finds the K-th key, and a second one over q among the keys
//              tied with it finds the largest q taken.  A last walk appends the chosen to the new active set (any order: no result
//              depends on it), stores (q, source slot) of the frame into the workspace and empties val / arg of every touched q, so
//              the next frame starts clean at a cost proportional to the touched count.
// Frame 0 takes the start states as its touched list (their q are distinct: no atomics).  Then the best final state, the
// backtrace through the stored slots and the token collapse, in the same launch.  Work per frame is proportional to the active
// set and its outgoing edges, never to Q or E; once per call each workgroup empties its val / arg (Q entries).
// val / arg are written by atomics (at L2) and read back with device-scope atomic loads, never through a vector L1 line that an
// earlier read may have left behind; everything else a workgroup hands between its wavefronts crosses __syncthreads.
// The frame body (expand A / B, select, the last walk) and the end (best final state, backtrace, collapse) live in
// asg_beam_frame.h: the streaming decoder (asg_beam_stream.hip) compiles the same text.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_frame.h"       // the frame body and the end of the search: the device code the streaming decoder shares

namespace asg {

namespace {

template <typename R, bool TRL>
__global__ void __launch_bounds__(kBT) beam_graph_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, int K, R theta, int cap,
                                                         char *work, size_t per_utt, size_t cnt_off, size_t fin_off,
                                                         R *scores, long long *path, long long *tokens, long long *tlen,
                                                         long long *states) {
    using KT = Key<R>;
    using U = typename KT::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Ctl<U> &ctl = *(Ctl<U> *) lds;
    R *cur_v = (R *) (lds + kFixedLds);                    // [K]
    int *cur_q = (int *) (cur_v + K);                      // [K]
    R *trs = (R *) (cur_q + K + (K & 1));                  // [N][N] if TRL
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Q = g.Q, N = P.N, T = P.T;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *tr = (const R *) P.transition;
    const R *fw = (const R *) g.final_w;
    long long *pb = path + (int64_t) b * T, *tk = tokens + (int64_t) b * T, *st = states + (int64_t) b * T;
    // the utterance's workspace (asg_beam_common.h, beam_work_layout)
    char *wb = work + (size_t) b * per_utt;
    BeamFrame<R> f;
    f.ctl = &ctl; f.cur_v = cur_v; f.cur_q = cur_q; f.trs = trs; f.tr = tr; f.ts0 = P.ts0; f.ts1 = P.ts1;
    f.N = N; f.Q = Q; f.K = K; f.G = beam_lanes_per_state(K); f.theta = theta;
    f.label = g.label; f.orow = bg.orow; f.start_q = bg.start_q; f.num_start = bg.num_start;
    f.oarc = (const int2 *) bg.oarc; f.ow = (const R *) bg.ow; f.sw = (const R *) g.start_w;
    int *bq, *bs;
    f.bind_work(wb, T, cap, bq, bs);
    // cnt_off != 0 (asg_beam_loss.hip): |A_t| of every frame goes to int32 [T] at that offset of the utterance's workspace
    int *cnt = cnt_off ? (int *) (wb + cnt_off) : nullptr;
    if (cnt) for (int t = tid; t < T; t += kBT) cnt[t] = 0;
    // fin_off != 0 (asg_beam_nbest.hip): |A_{len-1}| goes to the int32 at that offset and the values of that set, slot-aligned
    // with bq[len-1], behind it from byte 8 on
    int *fin_n = fin_off ? (int *) (wb + fin_off) : nullptr;

    if (len < 1) {
        beam_no_path(T, pb, tk, st, tlen + b);
        if (tid == 0) { scores[b] = NINF; if (fin_n) *fin_n = 0; }
        return;
    }
    if constexpr (TRL)
        for (int x = tid; x < N * N; x += kBT) trs[x] = tr[(int64_t) (x / N) * P.ts0 + (int64_t) (x % N) * P.ts1];
    if (len >= 2)
        for (int q = tid; q < Q; q += kBT) { dev_store(f.val + q, (U) 0); dev_store(f.arg + q, ~0ull); }
    if (tid == 0) { ctl.na = 0; ctl.n = 0; }
    __syncthreads();

    for (int t = 0; t < len; ++t) {
        const int na = ctl.na;
        if (t >= 1 && na == 0) break;                       // an empty beam stays empty
        beam_frame<R, TRL>(f, t == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bs, t);
        if (cnt && tid == 0) cnt[t] = ctl.na < K ? ctl.na : K;
    }

    // ---- score: the largest v + final_w over the last active set, the smallest q on a tie
    const int na = ctl.na;
    if (fin_n) {
        R *fin_v = (R *) (wb + fin_off + 8);
        for (int k = tid; k < na && k < K; k += kBT) fin_v[k] = cur_v[k];
        if (tid == 0) *fin_n = na < K ? na : K;
    }
    U bkey;
    int bqq, bk;
    beam_best_end<R>(ctl, cur_q, cur_v, na, fw, bkey, bqq, bk);
    if (bkey == 0) {                                        // an empty beam, or no active state with a finite final weight
        beam_no_path(T, pb, tk, st, tlen + b);
        if (tid == 0) scores[b] = NINF;
        return;
    }
    // the score itself, from the winner's own sum (the key folds -0 into +0)
    if (tid == 0) scores[b] = cur_v[bk] + fw[bqq];
    beam_backtrace(bq, bs, K, len, T, bk, g.label, g.state, pb, tk, st, tlen + b);
}

}  // namespace

int beam_graph_k(int Q, int beam_size) { return Q < 1 ? 1 : (beam_size < Q ? beam_size : Q); }

// The touched list holds the targets of one frame: at most K * (largest out-degree + 1), at most Q, at least the start states.
int beam_graph_cap(int Q, int K, int max_out, int num_start) {
    const int64_t c = (int64_t) K * ((int64_t) max_out + 1);
    int cap = (int) (c < (int64_t) Q ? c : (int64_t) Q);
    if (cap < num_start) cap = num_start;
    return cap < 1 ? 1 : cap;
}

size_t beam_graph_work_bytes(int elem, int T, int B, int Q, int K, int cap) {
    return (size_t) B * beam_work_layout(elem, T, Q, K, cap).end;
}

template <typename R>
hipError_t launch_beam_graph(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta, void *work,
                             void *scores, long long *path, long long *tokens, long long *tlen, long long *states,
                             hipStream_t stream, size_t stride, size_t cnt_off, size_t fin_off) {
    const int N = P.N;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const size_t per = stride ? stride : beam_work_layout(sizeof(R), P.T, G.Q, K, cap).end;
    const size_t beam = kFixedLds + (size_t) K * (sizeof(R) + 4) + 8;
    const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
    const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
#define ASG_BEAM(TRL)                                                                                                      \
    do {                                                                                                                   \
        const void *fn = (const void *) beam_graph_kernel<R, TRL>;                                                        \
        if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);     \
        hipLaunchKernelGGL((beam_graph_kernel<R, TRL>), dim3(P.B), dim3(kBT), dyn, stream, P, G, BG, K, (R) theta, cap,   \
                           (char *) work, per, cnt_off, fin_off, (R *) scores, path, tokens, tlen, states);                      \
    } while (0)
    if (trl) ASG_BEAM(true); else ASG_BEAM(false);
#undef ASG_BEAM
    return hipGetLastError();
}
template hipError_t launch_beam_graph<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, double, void *, void *,
                                             long long *, long long *, long long *, long long *, hipStream_t, size_t, size_t, size_t);
template hipError_t launch_beam_graph<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, double, void *, void *,
                                              long long *, long long *, long long *, long long *, hipStream_t, size_t,
                                              size_t, size_t);

}  // namespace asg
