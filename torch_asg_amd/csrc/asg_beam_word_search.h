// torch_asg_amd/csrc/asg_beam_word_search.h -- THE ONE-SHOT SEARCH over pairs (LM history h, lexicon product state q): one launch,
// one 1024-thread workgroup per utterance walks all frames of asg_beam_word_frame.h and, where the caller wants it, ends the search.
// One kernel text and one launcher for the four callers of the word-LM family:
//   asg_beam_word.hip        WordSearch::Decode      the decoder: the eight outputs of asg_beam_decode_words (FIN: the n-best
//                                                    stage behind it, asg_beam_word_nbest.hip)
//   asg_beam_word_loss.hip   WordSearch::Sets        the kept sets alone: |A_t| of every frame beside the [T][K] lists bq / bh
//   asg_beam_word_conf.hip   WordSearch::DecodeSets  both, and word_frames (FIN: asg_beam_word_nbest_conf.hip)
// "The loss and the confidences see the decoder's sets, the confidence calls return the decoder's bits" is this text compiled
// three times.  What differs is chosen at compile time -- the mode, LM look-ahead (LA), transitions in LDS (TRL), the last set
// left in memory (FIN); no runtime flag enters the frame loop, and the plain decoder's instantiations are the code they were.
// The kernel lives in the unnamed namespace: a unit instantiates the modes it launches and no other.
#pragma once
#include <type_traits>
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"

namespace asg {

namespace {

enum class WordSearch { Decode, Sets, DecodeSets };

// What an ending search writes: the decoder's eight outputs (and with DecodeSets word_frames, beside them).  Sets takes an empty one.
struct WordSearchOut {
    void *scores;
    long long *path, *tokens, *tlen, *states, *lm_states, *words, *wlen;
};

// No frame, an emptied beam, or no kept pair with a finite end: -1 / 0 everywhere and a score of -inf.
template <typename R, bool FRAMES>
__device__ __forceinline__ void word_search_no_path(int T, long long *pb, long long *tk, long long *st, long long *ls, long long *wd,
                                                    long long *wf, long long *tlen, long long *wlen, R *scores, int b) {
    word_no_path(T, pb, tk, st, ls, wd, tlen, wlen);
    if constexpr (FRAMES)
        for (int t = threadIdx.x; t < T; t += kBT) wf[t] = -1;
    if (threadIdx.x == 0) scores[b] = Num<R>::ninf();
}

// cnt_off: where in an utterance's block the kept counts go (Sets, DecodeSets).  fin_off: where a FIN instantiation leaves int32
// |A_{len-1}| and, from byte 8 behind it, that set's values [K], product states [K] and LM states [K].  The arguments up to fin_off
// are, in their order, what the plain decoder's kernel has always taken, so that its kernarg segment only grew at the end: what
// the other modes and the look-ahead add comes behind.
template <typename R, bool TRL, bool LA, bool FIN, WordSearch M>
__global__ void __launch_bounds__(kBT) beam_word_search(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, int K, R theta,
                                                        int cap, int tbits, char *work, size_t per_utt, R *scores,
                                                        long long *path, long long *tokens, long long *tlen, long long *states,
                                                        long long *lm_states, long long *words, long long *wlen, size_t fin_off,
                                                        long long *word_frames, size_t cnt_off, WordLookParam<LA> la) {
    constexpr bool kCnt = M != WordSearch::Decode;         // cnt[t] = |A_t| for t < len, 0 behind an emptied beam
    constexpr bool kEnd = M != WordSearch::Sets;           // the best end, the backtrace, the tokens and the words
    constexpr bool kFrames = M == WordSearch::DecodeSets;  // ... and where the words end
    static_assert(kEnd || !FIN, "only a search that ends leaves its last set");
    using U = typename Key<R>::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Ctl<U> &ctl = *(Ctl<U> *) lds;
    WordCtl &wctl = *(WordCtl *) (lds + kWordCtlOff);
    R *cur_v = (R *) (lds + kFixedLds);                    // [K]
    int *cur_q = (int *) (cur_v + K);                      // [K]
    int *cur_h = cur_q + K;                                // [K]
    R *trs = (R *) (cur_h + K);                            // [N][N] if TRL (2 * K ints: aligned)
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = P.N, T = P.T;
    const int len = clamp_len(P.in_len, b, T);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *tr = (const R *) P.transition;
    [[maybe_unused]] const R *fw = (const R *) g.final_w;
    auto row = [&](long long *p) { return p + (int64_t) b * T; };          // the utterance's row of a [B][T] output
    long long *pb = kEnd ? row(path) : nullptr, *tk = kEnd ? row(tokens) : nullptr, *st = kEnd ? row(states) : nullptr;
    long long *ls = kEnd ? row(lm_states) : nullptr, *wd = kEnd ? row(words) : nullptr;
    long long *wf = kFrames ? row(word_frames) : nullptr;
    BeamWordFrame<R, LA> f;
    // (the fields one by one, not through bind_graph: in this order -- the decoder's kernel's since 5n -- the plain decoder's
    // instantiations compile to the instructions they have always had; in bind_graph's they do not)
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
    char *wb = work + (size_t) b * per_utt;
    f.bind_work(wb, T, bq, bh, bs);
    [[maybe_unused]] int *cnt = (int *) (wb + cnt_off);

    if (len < 1) {
        if constexpr (kEnd)
            word_search_no_path<R, kFrames>(T, pb, tk, st, ls, wd, wf, tlen + b, wlen + b, scores, b);
        return;
    }
    if constexpr (TRL)
        for (int x = tid; x < N * N; x += kBT) trs[x] = tr[(int64_t) (x / N) * P.ts0 + (int64_t) (x % N) * P.ts1];
    if (len >= 2) {                                        // (a first frame does not use the table)
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
        if constexpr (kCnt)
            if (tid == 0) cnt[t] = ctl.na < K ? ctl.na : K;
    }
    if constexpr (kCnt)
        for (int u = t + tid; u < len; u += kBT) cnt[u] = 0;

    if constexpr (kEnd) {
        // ---- the best end over the last kept set, the smallest pair on a tie; the backtrace, the words, the tokens
        const int na = ctl.na < K ? ctl.na : K;
        if constexpr (FIN) {                                // the n-best stage reads the last set from memory
            char *fin = wb + fin_off;
            R *fv = (R *) (fin + 8);
            int *fq = (int *) (fv + K), *fh = fq + K;
            for (int k = tid; k < na; k += kBT) { fv[k] = cur_v[k]; fq[k] = cur_q[k]; fh[k] = cur_h[k]; }
            if (tid == 0) *(int *) fin = na;
        }
        U bkey;
        int bk;
        word_best_end<R, LA>(f, fw, true, cur_h, cur_q, cur_v, na, bkey, bk);
        if (bkey == 0) {                                    // an empty beam, or no kept pair with a finite end
            word_search_no_path<R, kFrames>(T, pb, tk, st, ls, wd, wf, tlen + b, wlen + b, scores, b);
            return;
        }
        word_backtrace<R, LA>(f, fw, true, cur_h, cur_q, cur_v, bk, bq, bh, bs, len, T, scores + b, pb, tk, st, ls, wd, tlen + b,
                              wlen + b);
        if constexpr (kFrames) word_end_frames(pb, f.sep, len, T, wlen + b, wf);   // (with the word of the final step)
    }
}

// THE launcher: the sizes of the search (cap, the table, the kept set and -- while they fit beside it -- the transitions in LDS),
// the dynamic-LDS attribute and the dispatch over TRL x LA x FIN.  `per`: the distance of the utterances' blocks, each with the
// decoder's own layout at its front.  LA: the look-ahead, or null.  fin_off != 0 picks FIN.
template <typename R, WordSearch M>
hipError_t launch_beam_word_search(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                   const WordLookArgs *LA, int K, double theta, void *work, size_t per, size_t cnt_off,
                                   size_t fin_off, const WordSearchOut &out, long long *word_frames, hipStream_t stream) {
    const int N = P.N;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const int tbits = word_table_bits(cap);
    const size_t beam = kFixedLds + (size_t) K * (sizeof(R) + 8);
    const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
    const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
    auto run = [&](auto trl_c, auto la_c, auto fin_c, const auto &look) {
        auto *fn = beam_word_search<R, decltype(trl_c)::value, decltype(la_c)::value, decltype(fin_c)::value, M>;
        if (dyn > 64 * 1024) (void) hipFuncSetAttribute((const void *) fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);
        hipLaunchKernelGGL(fn, dim3(P.B), dim3(kBT), dyn, stream, P, G, BG, LM, K, (R) theta, cap, tbits, (char *) work, per,
                           (R *) out.scores, out.path, out.tokens, out.tlen, out.states, out.lm_states, out.words, out.wlen, fin_off,
                           word_frames, cnt_off, look);
    };
    auto with_fin = [&](auto trl_c, auto la_c, const auto &look) {
        if constexpr (M != WordSearch::Sets) {
            if (fin_off) return run(trl_c, la_c, std::true_type{}, look);
        }
        run(trl_c, la_c, std::false_type{}, look);
    };
    auto with_la = [&](auto trl_c) {
        if (LA) with_fin(trl_c, std::true_type{}, *LA); else with_fin(trl_c, std::false_type{}, WordNoLook{});
    };
    if (trl) with_la(std::true_type{}); else with_la(std::false_type{});
    return hipGetLastError();
}

}  // namespace

}  // namespace asg
