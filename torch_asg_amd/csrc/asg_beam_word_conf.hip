// torch_asg_amd/csrc/asg_beam_word_conf.hip -- WORD CONFIDENCES and END FRAMES of the word-LM beam decoder's hypothesis, from the
// lattice its own search kept, on gfx950.  The specification is include/asg_hip.h::asg_beam_words_confidence;
// tests/beam_word_conf_ref.py restates it in numpy.
//
// Five launches on one stream, the frame loop of the search in one of them:
//   1  beam_word_conf_search: asg_beam_word_loss.hip's search (the frame of asg_beam_word_frame.h in a loop that leaves |A_t|
//      beside the [T][K] lists bq / bh) followed by the decoder's own end in the same launch -- word_best_end and
//      word_backtrace of asg_beam_word_frame.h, the device text beam_word_kernel / beam_word_la_kernel end with -- so the eight
//      outputs of the decoder have that call's bits.  It also writes word_frames: the frames of the winning path's separator
//      edges and, for the word of the final step, len.
//   2 - 4  launch_beam_word_loss_lattice: the target walk (there is no target: it writes the header's 0), beam_loss_sets<WordSets>
//      and beam_word_loss_fwd with alpha stored for every frame -> U, alpha, Z_K (the normalisers).  Unchanged kernels.
//   5  beam_word_conf_bwd: asg_beam_word_conf_pull.h over HypSink -- beam_loss_bwd's beta pull (one 1024-thread workgroup per utterance, frames len-1 .. 1, U_{t+1} with its
//      beta in LDS, G lanes per source pair, a max pass and a sum pass) without label posteriors, (i, j) tile and transition
//      gradient.  The sum pass also forms the posterior exp(alpha + c - Z_K) of every SEPARATOR edge -- the event "word w ends at
//      frame t" -- and, before the first frame, the posteriors of the final step.  An event is added, as a 64-bit fixed-point
//      integer with 54 fractional bits, to every word of the hypothesis that has the event's word and whose window
//      [t_k - tol, t_k + tol] holds the event's frame.  t_k ascends strictly, so the words whose window holds frame t are one
//      range [ka, kb) of at most 2 tol + 1 indices that only moves down with t: the workgroup keeps it in registers, an event
//      scans it, and a word's accumulator is slot k mod 256 of a ring in LDS (ds_add_u64: no trip to L2, and all the events
//      of a frame meet in one or two words -- the worst shape for a global atomic).  A word that leaves the range is converted,
//      stored and its slot zeroed.  Integer adds only: no order of arrival changes a bit.  Every output and every workspace
//      word that is read is written by these kernels: no memset, no host synchronisation, the call captures and replays.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"  // the frame of the search and its end
#include "asg_beam_lattice.h"     // the helpers of the lattice pass: subgroup, find_sorted, the butterflies, to_fixed
#include "asg_beam_word_lat.h"    // WordLat: how a pair's edges are walked
#include "asg_beam_word_conf_pull.h"  // the beta pull, shared with asg_beam_word_nbest_conf.hip
#include "asg_beam_conf_sink.h"   // HypSink and its ring, shared with asg_beam_conf.hip

namespace asg {

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// 1: the search with its end.  beam_word_loss_search's loop (cnt[t] = |A_t| for t < len), then beam_word_kernel's end.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void conf_no_path(int T, long long *pb, long long *tk, long long *st, long long *ls, long long *wd,
                                             long long *wf, long long *tlen, long long *wlen) {
    word_no_path(T, pb, tk, st, ls, wd, tlen, wlen);
    for (int t = threadIdx.x; t < T; t += kBT) wf[t] = -1;
}

// FIN: the instantiation behind the n-best confidences (asg_beam_word_nbest_conf.hip), which also leaves the last set in memory
// at fin_off, as beam_word_kernel<R, TRL, FIN> does; without it the text is what it was before the flag existed.
template <typename R, bool TRL, bool LA, bool FIN>
__global__ void __launch_bounds__(kBT) beam_word_conf_search(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, int K, R theta,
                                                             int cap, int tbits, char *work, size_t per_utt, size_t cnt_off,
                                                             WordLookParam<LA> la, R *scores, long long *path, long long *tokens,
                                                             long long *tlen, long long *states, long long *lm_states,
                                                             long long *words, long long *wlen, long long *wframes,
                                                             size_t fin_off) {
    using U = typename Key<R>::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Ctl<U> &ctl = *(Ctl<U> *) lds;
    WordCtl &wctl = *(WordCtl *) (lds + kWordCtlOff);
    R *cur_v = (R *) (lds + kFixedLds);                    // [K]
    int *cur_q = (int *) (cur_v + K);                      // [K]
    int *cur_h = cur_q + K;                                // [K]
    R *trs = (R *) (cur_h + K);                            // [N][N] if TRL
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = P.N, T = P.T;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *tr = (const R *) P.transition;
    const R *fw = (const R *) g.final_w;
    long long *pb = path + (int64_t) b * T, *tk = tokens + (int64_t) b * T, *st = states + (int64_t) b * T;
    long long *ls = lm_states + (int64_t) b * T, *wd = words + (int64_t) b * T, *wf = wframes + (int64_t) b * T;
    BeamWordFrame<R, LA> f;
    f.ctl = &ctl; f.wctl = &wctl; f.cur_v = cur_v; f.cur_q = cur_q; f.cur_h = cur_h; f.trs = trs; f.tr = tr;
    f.ts0 = P.ts0; f.ts1 = P.ts1; f.N = N; f.theta = theta;
    bind_graph<R, LA>(f, g, bg, lm, K, cap, tbits);
    bind_look<R>(f, la);
    int *bq, *bh, *bs;
    char *wb = work + (size_t) b * per_utt;
    f.bind_work(wb, T, bq, bh, bs);
    int *cnt = (int *) (wb + cnt_off);
    if (len < 1) {
        conf_no_path(T, pb, tk, st, ls, wd, wf, tlen + b, wlen + b);
        if (tid == 0) scores[b] = NINF;
        return;
    }
    if constexpr (TRL)
        for (int x = tid; x < N * N; x += kBT) trs[x] = tr[(int64_t) (x / N) * P.ts0 + (int64_t) (x % N) * P.ts1];
    if (len >= 2) {
        const size_t C = (size_t) 1 << tbits;
        for (size_t s = tid; s < C; s += kBT) { dev_store(f.tkey + s, 0ull); dev_store(f.val + s, (U) 0); dev_store(f.arg + s, ~0ull); }
    }
    if (tid == 0) { ctl.na = 0; ctl.n = 0; }
    __syncthreads();
    int t = 0;
    for (; t < len; ++t) {
        const int na = ctl.na;
        if (t >= 1 && na == 0) break;                       // an empty beam stays empty
        beam_word_frame<R, TRL, LA>(f, t == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bh, bs, t);
        if (tid == 0) cnt[t] = ctl.na < K ? ctl.na : K;
    }
    for (int u = t + tid; u < len; u += kBT) cnt[u] = 0;

    // ---- the decoder's end: the best end over the last kept set, the smallest pair on a tie; the backtrace, the words, the tokens
    const int na = ctl.na < K ? ctl.na : K;
    if constexpr (FIN) {                                    // the n-best stage reads the last set from memory
        char *fin = wb + fin_off;
        R *fv = (R *) (fin + 8);
        int *fq = (int *) (fv + K), *fh = fq + K;
        for (int k = tid; k < na; k += kBT) { fv[k] = cur_v[k]; fq[k] = cur_q[k]; fh[k] = cur_h[k]; }
        if (tid == 0) *(int *) fin = na;
    }
    U bkey;
    int bk;
    word_best_end<R, LA>(f, fw, true, cur_h, cur_q, cur_v, na, bkey, bk);
    if (bkey == 0) {                                        // an empty beam, or no kept pair with a finite end
        conf_no_path(T, pb, tk, st, ls, wd, wf, tlen + b, wlen + b);
        if (tid == 0) scores[b] = NINF;
        return;
    }
    word_backtrace<R, LA>(f, fw, true, cur_h, cur_q, cur_v, bk, bq, bh, bs, len, T, scores + b, pb, tk, st, ls, wd, tlen + b,
                          wlen + b);
    word_end_frames(pb, f.sep, len, T, wlen + b, wf);      // (with the word of the final step)
}

// ---------------------------------------------------------------------------------------------------------------------
// 5: beta with the word-event sink.  Dynamic LDS: [nq u64 M][nb R M][pad to 16][ring u64 256].  beta[t-1] crosses from the lanes
// that sum it to the workgroup through the utterance's two rows in the workspace, as in beam_loss_bwd.
// ---------------------------------------------------------------------------------------------------------------------
// The sink is HypSink (asg_beam_conf_sink.h): the words whose window holds the frame are [ka, kb), a word's accumulator slot
// k mod 256 of the ring.
inline size_t conf_lds(int elem, int M) { return bwd_front(elem, 8, M) + (size_t) kConfRing * 8; }

template <typename R>
__global__ void __launch_bounds__(kBL) beam_word_conf_bwd(Problem P, typename WordLat<R>::Args args, char *work, size_t beta_off,
                                                          const R *Zs, const long long *words, const long long *wlen,
                                                          const long long *wframes, int tol, R *conf) {
    using KeyT = unsigned long long;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int M = args.lay.M, T = P.T;
    KeyT *nq = (KeyT *) lds;                                                   // [M] U_t
    R *nb = (R *) (lds + (size_t) M * sizeof(KeyT));                           // [M] beta[t] of U_t
    unsigned long long *ring = (unsigned long long *) (lds + bwd_front(sizeof(R), sizeof(KeyT), M));
    const int b = blockIdx.x;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    const R Z = Zs[b];
    int nw = 0;
    if (len >= 1 && Z > NINF) {
        const long long n = wlen[b];
        nw = (int) (n < 0 ? 0 : (n > len ? len : n));                          // (a path of len frames ends at most len words)
    }
    beam_word_conf_words<R>(P, args, work + (size_t) b * args.lay.per, beta_off, Z, len, nw, T, tol, words + (int64_t) b * T,
                            wframes + (int64_t) b * T, conf + (int64_t) b * T, ring, nq, nb);
}

}  // namespace

BeamWordConfLayout beam_word_conf_layout(int elem, int T, int K, int cap) {
    BeamWordConfLayout l{};
    l.lat = beam_word_loss_layout(elem, T, K, cap, 0, true);
    l.beta = l.lat.per;
    l.per = l.beta + a256(2 * (size_t) l.lat.M * elem);
    l.lat.per = l.per;
    return l;
}

size_t beam_word_conf_work_bytes(int elem, int T, int B, int K, int cap) {
    return (size_t) B * beam_word_conf_layout(elem, T, K, cap).per;
}

// Launch 1 alone.  `per` and `cnt_off` say where an utterance's block starts and where its kept counts go; with fin_off != 0 the
// search also leaves |A_{len-1}| and its last set there (the FIN instantiations: the n-best confidences).
template <typename R>
hipError_t launch_beam_word_conf_search(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                        const WordLookArgs *LA, int K, double theta, void *work, size_t per, size_t cnt_off,
                                        size_t fin_off, void *scores, long long *path, long long *tokens, long long *tlen,
                                        long long *states, long long *lm_states, long long *words, long long *wlen,
                                        long long *word_frames, hipStream_t stream) {
    const int B = P.B, N = P.N;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const int tbits = word_table_bits(cap);
    char *w = (char *) work;
    const size_t beam = kFixedLds + (size_t) K * (sizeof(R) + 8);
    const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
    const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
#define ASG_BEAM_WORD_CONF_SEARCH(TRL, LAF, FIN, LOOK)                                                                        \
    do {                                                                                                                     \
        set_lds((const void *) beam_word_conf_search<R, TRL, LAF, FIN>, dyn);                                               \
        hipLaunchKernelGGL((beam_word_conf_search<R, TRL, LAF, FIN>), dim3(B), dim3(kBT), dyn, stream, P, G, BG, LM, K,    \
                           (R) theta, cap, tbits, w, per, cnt_off, LOOK, (R *) scores, path, tokens, tlen, states,           \
                           lm_states, words, wlen, word_frames, fin_off);                                                    \
    } while (0)
#define ASG_BEAM_WORD_CONF_SEARCH_F(TRL, LAF, LOOK)                                                                           \
    do {                                                                                                                     \
        if (fin_off) ASG_BEAM_WORD_CONF_SEARCH(TRL, LAF, true, LOOK); else ASG_BEAM_WORD_CONF_SEARCH(TRL, LAF, false, LOOK); \
    } while (0)
    if (LA) { if (trl) ASG_BEAM_WORD_CONF_SEARCH_F(true, true, *LA); else ASG_BEAM_WORD_CONF_SEARCH_F(false, true, *LA); }
    else if (trl) ASG_BEAM_WORD_CONF_SEARCH_F(true, false, WordNoLook{});
    else ASG_BEAM_WORD_CONF_SEARCH_F(false, false, WordNoLook{});
#undef ASG_BEAM_WORD_CONF_SEARCH_F
#undef ASG_BEAM_WORD_CONF_SEARCH
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_word_conf(const Problem &P0, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                 const WordLookArgs *LA, int K, double theta, int tol, void *work, void *scores, long long *path,
                                 long long *tokens, long long *tlen, long long *states, long long *lm_states, long long *words,
                                 long long *wlen, long long *word_frames, void *word_conf, void *normalisers, hipStream_t stream) {
    Problem P = P0;
    P.targets = nullptr;                                                         // the lattice of the search alone: U_t = A_t
    P.tg_len = nullptr;
    const int T = P.T, B = P.B;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const BeamWordConfLayout lay = beam_word_conf_layout(sizeof(R), T, K, cap);
    char *w = (char *) work;
    hipError_t e = launch_beam_word_conf_search<R>(P, G, BG, LM, LA, K, theta, work, lay.per, lay.lat.cnt, 0, scores, path, tokens,
                                                   tlen, states, lm_states, words, wlen, word_frames, stream);
    if (e != hipSuccess) return e;
    e = launch_beam_word_loss_lattice<R>(P, G, BG, LM, lay.lat, K, true, work, normalisers, stream);
    if (e != hipSuccess) return e;
    const size_t dyn = conf_lds(sizeof(R), lay.lat.M);
    set_lds((const void *) beam_word_conf_bwd<R>, dyn);
    hipLaunchKernelGGL((beam_word_conf_bwd<R>), dim3(B), dim3(kBL), dyn, stream, P, typename WordLat<R>::Args{G, BG, LM, lay.lat}, w,
                       lay.beta, (const R *) normalisers, (const long long *) words, (const long long *) wlen,
                       (const long long *) word_frames, tol, (R *) word_conf);
    return hipGetLastError();
}

#define ASG_WORD_CONF_INST(R)                                                                                                   \
    template hipError_t launch_beam_word_conf<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, \
                                                 const WordLookArgs *, int, double, int, void *, void *, long long *,           \
                                                 long long *, long long *, long long *, long long *, long long *, long long *,  \
                                                 long long *, void *, void *, hipStream_t);                     \
    template hipError_t launch_beam_word_conf_search<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &,             \
                                                        const WordLmArgs &, const WordLookArgs *, int, double, void *, size_t,  \
                                                        size_t, size_t, void *, long long *, long long *, long long *,          \
                                                        long long *, long long *, long long *, long long *, long long *,        \
                                                        hipStream_t);
ASG_WORD_CONF_INST(float)
ASG_WORD_CONF_INST(double)
#undef ASG_WORD_CONF_INST

}  // namespace asg
