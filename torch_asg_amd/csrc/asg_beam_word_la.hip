// torch_asg_amd/csrc/asg_beam_word_la.hip -- beam decoding with a lexicon and a word n-gram LM WITH LM LOOK-AHEAD on gfx950
// (include/asg_hip.h::asg_beam_decode_words_la).  The launch of asg_beam_word.hip -- one 1024-thread workgroup per utterance
// walks the frames; table, select, prune, back-pointers and workspace are that file's -- over the frame and the end of
// asg_beam_word_frame.h compiled with the look-ahead flag on: inside a word a pair's value also carries L(h, node), the best LM
// score a word below its trie node can get after h, and every edge adds the difference of its two ends (a separator edge the
// difference between the word's own LM score and the L it entered with), so that one value per pair stays the only search state.
//
// L is evaluated on the device per expanded edge against the pair's history (BeamWordFrame::look): the words below a node are a
// range of ranks (pre-order of the trie), every LM state keeps its arcs sorted by rank, and a sparse table of maxima over those
// rows answers "the best arc of state s in the range" with two binary searches and two reads (state 0, where the chains end and
// the row is the longest, has its answers in a dense [S] array: one read); the walk down the backoff chain adds the backoff
// weights as the LM walk does.  L of the source pair is the same for all its edges: it is taken once per pair
// and phase.  Plain loads of read-only arrays: no workspace, no atomics, nothing to clear.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"

namespace asg {

namespace {

// FIN: the instantiation behind the n-best stage (asg_beam_word_nbest.hip, launch_beam_words_nbest_la), which also leaves the last
// set in memory at fin_off, as beam_word_kernel's does; the decoder's own (FIN false) is the code object it was before (DESIGN.md
// 5v).
template <typename R, bool TRL, bool FIN>
__global__ void __launch_bounds__(kBT) beam_word_la_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, WordLookArgs la,
                                                           int K, R theta, int cap, int tbits, char *work, size_t per_utt,
                                                           R *scores, long long *path, long long *tokens, long long *tlen,
                                                           long long *states, long long *lm_states, long long *words,
                                                           long long *wlen, size_t fin_off) {
    using KT = Key<R>;
    using U = typename KT::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Ctl<U> &ctl = *(Ctl<U> *) lds;
    WordCtl &wctl = *(WordCtl *) (lds + kWordCtlOff);
    R *cur_v = (R *) (lds + kFixedLds);                    // [K]
    int *cur_q = (int *) (cur_v + K);                      // [K]
    int *cur_h = cur_q + K;                                // [K]
    R *trs = (R *) (cur_h + K);                            // [N][N] if TRL (2 * K ints: aligned)
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = P.N, T = P.T;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *tr = (const R *) P.transition;
    const R *fw = (const R *) g.final_w;
    long long *pb = path + (int64_t) b * T, *tk = tokens + (int64_t) b * T, *st = states + (int64_t) b * T;
    long long *ls = lm_states + (int64_t) b * T, *wd = words + (int64_t) b * T;
    BeamWordFrame<R, true> f;
    f.ctl = &ctl; f.wctl = &wctl; f.cur_v = cur_v; f.cur_q = cur_q; f.cur_h = cur_h; f.trs = trs; f.tr = tr;
    f.ts0 = P.ts0; f.ts1 = P.ts1;
    f.N = N; f.K = K; f.G = beam_lanes_per_state(K); f.cap = cap; f.sep = lm.sep; f.theta = theta;
    f.qbits = bits_of(g.Q); f.pbits = f.qbits + bits_of(lm.H);
    f.label = g.label; f.state = g.state; f.orow = bg.orow; f.start_q = bg.start_q; f.num_start = bg.num_start;
    f.oarc = (const int2 *) bg.oarc; f.ow = (const R *) bg.ow; f.sw = (const R *) g.start_w;
    f.lrow = lm.row; f.lword = lm.word; f.lnext = lm.next; f.lback = lm.backoff; f.wos = lm.word_of_state;
    f.lw = (const R *) lm.lw; f.bw = (const R *) lm.bw; f.ew = (const R *) lm.ew; f.lstart = lm.start;
    bind_look<R>(f, la);
    f.tbits = tbits;
    int *bq, *bh, *bs;
    f.bind_work(work + (size_t) b * per_utt, T, bq, bh, bs);

    if (len < 1) {
        word_no_path(T, pb, tk, st, ls, wd, tlen + b, wlen + b);
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

    for (int t = 0; t < len; ++t) {
        const int na = ctl.na;
        if (t >= 1 && na == 0) break;                       // an empty beam stays empty
        beam_word_frame<R, TRL, true>(f, t == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bh, bs, t);
    }

    // ---- the best end over the last kept set, the smallest pair on a tie; the backtrace, the words, the tokens
    const int na = ctl.na < K ? ctl.na : K;
    if constexpr (FIN) {                                    // the n-best stage reads the last set from memory
        char *fin = work + (size_t) b * per_utt + fin_off;
        R *fv = (R *) (fin + 8);
        int *fq = (int *) (fv + K), *fh = fq + K;
        for (int k = tid; k < na; k += kBT) { fv[k] = cur_v[k]; fq[k] = cur_q[k]; fh[k] = cur_h[k]; }
        if (tid == 0) *(int *) fin = na;
    }
    U bkey;
    int bk;
    word_best_end<R, true>(f, fw, true, cur_h, cur_q, cur_v, na, bkey, bk);
    if (bkey == 0) {                                        // an empty beam, or no kept pair with a finite end
        word_no_path(T, pb, tk, st, ls, wd, tlen + b, wlen + b);
        if (tid == 0) scores[b] = NINF;
        return;
    }
    word_backtrace<R, true>(f, fw, true, cur_h, cur_q, cur_v, bk, bq, bh, bs, len, T, scores + b, pb, tk, st, ls, wd, tlen + b,
                      wlen + b);
}

}  // namespace

template <typename R>
hipError_t launch_beam_words_la(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                const WordLookArgs &LA, int K, double theta, void *work, void *scores, long long *path,
                                long long *tokens, long long *tlen, long long *states, long long *lm_states, long long *words,
                                long long *wlen, hipStream_t stream, size_t stride, size_t fin_off) {
    const int N = P.N;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const int tbits = word_table_bits(cap);
    const size_t per = stride ? stride : beam_word_work_bytes(sizeof(R), P.T, 1, K, cap);
    const size_t beam = kFixedLds + (size_t) K * (sizeof(R) + 8);
    const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
    const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
#define ASG_BEAM_WORD_LA(TRL, FIN)                                                                                        \
    do {                                                                                                                  \
        const void *fn = (const void *) beam_word_la_kernel<R, TRL, FIN>;                                                \
        if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);    \
        hipLaunchKernelGGL((beam_word_la_kernel<R, TRL, FIN>), dim3(P.B), dim3(kBT), dyn, stream, P, G, BG, LM, LA, K,   \
                           (R) theta, cap, tbits, (char *) work, per, (R *) scores, path, tokens, tlen, states, lm_states, \
                           words, wlen, fin_off);                                                                         \
    } while (0)
    if (fin_off) { if (trl) ASG_BEAM_WORD_LA(true, true); else ASG_BEAM_WORD_LA(false, true); }
    else if (trl) ASG_BEAM_WORD_LA(true, false); else ASG_BEAM_WORD_LA(false, false);
#undef ASG_BEAM_WORD_LA
    return hipGetLastError();
}
template hipError_t launch_beam_words_la<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                                const WordLookArgs &, int, double, void *, void *, long long *, long long *,
                                                long long *, long long *, long long *, long long *, long long *, hipStream_t,
                                                size_t, size_t);
template hipError_t launch_beam_words_la<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                                 const WordLookArgs &, int, double, void *, void *, long long *, long long *,
                                                 long long *, long long *, long long *, long long *, long long *, hipStream_t,
                                                 size_t, size_t);

}  // namespace asg
