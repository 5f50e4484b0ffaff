// torch_asg_amd/csrc/asg_beam_word_nbest.hip -- the N BEST hypotheses of the beam search over pairs (LM history h, lexicon product
// state q) of asg_beam_word.hip and asg_beam_word_stream.hip, each with its score split into the acoustic part (emissions and
// transitions), the lexicon part (automaton weights, token_score, final weight) and the LM part (every LM walk's own sum and the
// end of the sentence), on gfx950.  The specification is include/asg_hip.h::asg_beam_decode_words_nbest;
// tests/beam_word_nbest_ref.py restates it.
//
// Lexicon and LM are deterministic, so a token sequence determines its pair: the kept pairs of the last frame carry different
// token sequences, and the search has left (q, h, source slot) of every kept pair of every frame on the device.  ONE kernel,
// beam_word_nbest_kernel, one 1024-thread workgroup per utterance or stream slot, told where the last set and the [T][K] rows
// live (BeamWordNbestSrc):
//   one-shot   behind beam_word_kernel on the same stream (the decoder's own device code, so the same sets and back-pointers bit
//              for bit), asked to leave |A_{len-1}| and that set beside its rows;
//   stream     over a stream state, which holds the set in memory already; it is only read.
//   window     over a window state of asg_beam_word_window.hip, whose rows are rings: every row is the uncommitted tail of its
//              chain, without sums (the kernel's third source, described at its template below); it is only read.
//   keys     per entry of the last set the end -- with `final` word_end's (v + final_w) + endw, the LM walk of a word-end node
//            done here once, without it the value v -- as (~key of end, pair << 14 | slot).
//   sort     a fixed bitonic network in LDS over the power of two >= |A|, padded with all-ones entries, ascending: end
//            descending, then pair order; entries without a finite end sort behind every candidate.  P2(K) * (8 + e) bytes: 128
//            KiB at K = 8192 in float64.
//   walk     one lane per hypothesis follows bs / bq backwards into its column of the frame-major int32 [T][nb] block (and, when
//            lm_states is asked for, bh into that output), then forwards for the three sums, carrying h through its own LM walks:
//            emission and transition of every frame; start weight, the weight of every edge taken -- binary search for the target
//            in the source's CSR row -- and final weight; the sum of every separator edge's LM walk and the end.  Adds only, in
//            frame order.  Strips of 1024 hypotheses.
//   write    one wavefront per output row: path / states from the column, tokens by the ballot and popcount collapse of the
//            decoders, words by the same collapse over the separator edges, then the final word; the same loop fills the padding
//            rows.
// Every output, padding row and scratch word that is read is written here: no memset, no copy.  One integer LDS counter; no
// atomics on values: bit-identical run to run.
//
// The same kernel with the look-ahead flag (LA) serves the searches with LM look-ahead: behind beam_word_la_kernel, or over a state
// that asg_beam_word_stream_advance_la left.  The end of an entry is then word_end<R, true>'s / word_prefix<R, true>'s, which take
// the estimate the value still carries back; the walk, the three sums and the write stage are the same text.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"  // step, word_end, the pair: the bits of the ends are the one-best decoder's
#include "asg_beam_window_common.h"  // the window's header and its clamps, the ring's step

namespace asg {

namespace {

constexpr int kNT = 1024;          // workgroup

// behind the utterances of the one-shot call: what the one-best search writes (scores [B], token and word lengths [B], path /
// tokens / states / lm_states / words [5][B][T])
inline size_t tail_bytes(int T, int B) { return 3 * a256((size_t) B * 8) + a256((size_t) 5 * B * T * 8); }

template <typename U>
__device__ __forceinline__ bool entry_less(U ka, unsigned long long pa, U kb, unsigned long long pb) {
    return ka < kb || (ka == kb && pa < pb);
}

// LA: over a search with LM look-ahead (asg_beam_decode_words_nbest_la, asg_beam_word_stream_nbest_la).  The values of the set then
// carry L(h, node): the keys and `scores` take it back as the one-best does -- word_end<R, true>, word_prefix<R, true>, that text
// -- and nothing else changes: the walk and the three sums never see a look-ahead term.  Off by default: the
// instantiations without it compile the text they compiled before the flag existed.
//
// SRC says where the search lives (asg_kernels.h).  kBeamWordNbestRows is the text above, for the one-shot workspace and the stream
// state.  kBeamWordNbestWindow (asg_beam_word_window_nbest, with LA asg_beam_word_window_nbest_la) reads a window state, and what
// differs is selected with `if constexpr`:
//   header   WordWinHdr through window_header and window_live_base; frames, committed and status as beam_word_window_result_kernel
//            writes them; a row has len = pos - base frames, 0 .. W, and an empty tail still counts.
//   walk     the row of frame pos-1 from a 64-bit remainder, then ring_prev: at most W steps into column t = frame - base; no
//            forward pass and no sums (the edge into frame `base` needs the product state and the history of frame base-1, which
//            the header does not keep).
//   write    tokens collapsed from the header's `carry` (collapse_tokens_from's rule); words by collapse_words_from's rule, the
//            label and automaton state before column 0 being `carry` / `carry_state`, so a separator edge on the first
//            uncommitted frame gives its word once; the final word from the set's own q, also behind an empty tail, bounded by W
//            as the result kernel bounds it.
// The state is only read.
template <typename R, bool LA = false, int SRC = kBeamWordNbestRows>
__global__ void __launch_bounds__(kNT) beam_word_nbest_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm,
                                                              BeamWordNbestSrc src, int K, int cap, int tbits, int nbest, int P2max,
                                                              int final,
                                                              R *scores, R *escores, R *gscores, R *lscores, long long *path,
                                                              long long *tokens, long long *tlen, long long *states,
                                                              long long *lm_states, long long *words, long long *wlen,
                                                              long long *nhyp, long long *frames, long long *committed,
                                                              long long *status, WordLookParam<LA> la) {
    using KT = Key<R>;
    using U = typename KT::U;
    constexpr bool kWin = SRC == kBeamWordNbestWindow;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int ncand;
    unsigned long long *sp = (unsigned long long *) lds;                  // [P2max] pair << 14 | slot
    U *sk = (U *) (sp + P2max);                                           // [P2max] ~key of end
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int T = src.Tw, nb = src.nb;
    const R NINF = Num<R>::ninf();
    const char *wb = src.base + (size_t) b * src.per;
    int len, na;
    [[maybe_unused]] int row_top = 0, cstate0 = -1;                       // the window: the ring's row of frame pos-1, and the
    [[maybe_unused]] long long carry0 = -1;                               // automaton state and label the collapses start from
    if constexpr (kWin) {
        const WordWinHdr *hdr = (const WordWinHdr *) (wb + src.pos_off);
        long long pos = hdr->pos, base = hdr->base;
        na = hdr->na;
        window_header(pos, base, na, K);
        if (tid == 0) {
            frames[b] = pos;
            committed[b] = base;
            status[b] = (hdr->status & 1) | (pos >= 1 && na == 0 ? 2 : 0);
        }
        base = window_live_base(pos, base, T);                            // (a set that is not empty has pos <= base + W)
        len = na > 0 ? (int) (pos - base) : 0;                            // 0 .. W: the tail may be empty, and its row still counts
        row_top = pos >= 1 ? (int) ((pos - 1) % T) : 0;
        carry0 = hdr->carry; cstate0 = hdr->carry_state;
    } else {
        len = src.pos_off ? *(const int *) (wb + src.pos_off) : clamp_len(P.in_len, b, T);
        len = len < 0 ? 0 : (len > T ? T : len);
        na = len >= 1 ? *(const int *) (wb + src.na_off) : 0;
        na = na < 0 ? 0 : (na > K ? K : na);
    }
    const R *in = P.inputs ? (const R *) P.inputs + (int64_t) b * P.is1 : nullptr;   // the stream keeps no emissions
    const R *tr = (const R *) P.transition;
    const R *sw = (const R *) g.start_w, *fw = (const R *) g.final_w, *ow = (const R *) bg.ow;
    const int2 *oarc = (const int2 *) bg.oarc;
    const BeamWordWorkLayout wl = beam_word_work_layout(sizeof(R), T, K, cap, tbits);
    const int *bq = (const int *) (wb + wl.bq), *bh = (const int *) (wb + wl.bh), *bs = (const int *) (wb + wl.bs);
    const R *set_v = (const R *) (wb + src.set_off);
    const int *set_q = (const int *) (set_v + K), *set_h = set_q + K;
    int *cols = (int *) (src.cols + (size_t) b * src.cols_per);           // [T][nb]
    const int64_t ob = (int64_t) b * nbest;                               // the slot's first output row
    BeamWordFrame<R, LA> f{};                                             // what step and word_end read; nothing of the frame loop
    f.qbits = bits_of(g.Q); f.sep = lm.sep; f.K = K;
    f.label = g.label; f.state = g.state;
    f.lrow = lm.row; f.lword = lm.word; f.lnext = lm.next; f.lback = lm.backoff; f.wos = lm.word_of_state;
    f.lw = (const R *) lm.lw; f.bw = (const R *) lm.bw; f.ew = (const R *) lm.ew; f.lstart = lm.start;
    bind_look<R>(f, la);
    const int Q = g.Q;

    int P2 = 1;
    while (P2 < na) P2 *= 2;                                              // (<= P2max: na <= K)
    if (tid == 0) {
        ncand = 0;
        if constexpr (!kWin) {
            if (frames) frames[b] = len;
            if (status) status[b] = *(const int *) (wb + src.ovf_off) != 0;
        }
    }
    __syncthreads();
    // ---- the ends of the last set as keys (the LM walk of a word-end pair: once, here)
    for (int x0 = 0; x0 < P2; x0 += kNT) {
        const int x = x0 + tid;
        U ik = ~(U) 0;
        unsigned long long ps = ~0ull;
        bool cand = false;
        if (x < na) {
            const int q = set_q[x], h = set_h[x];
            R end = set_v[x];
            int w;
            if constexpr (LA) {                                           // a prefix: without the estimate the value still carries
                cand = q >= 0 && q < Q && (!final || word_end<R, LA>(f, fw, h, q, end, end, w));
                if (cand && !final) end = word_prefix<R, LA>(f, h, q, end);
                cand = cand && end > NINF;
            } else cand = q >= 0 && q < Q && (!final || word_end<R>(f, fw, h, q, end, end, w)) && end > NINF;
            if (cand) { ik = (U) ~KT::enc(end); ps = (f.pair(h, q) << kWordSlotBits) | (unsigned) x; }
        }
        if (x < P2) { sk[x] = ik; sp[x] = ps; }
        const unsigned long long m = __ballot(cand);
        if (lane == 0 && m) atomicAdd(&ncand, __popcll(m));
    }
    __syncthreads();
    // ---- bitonic network, ascending in (~key, pair << 14 | slot)
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = tid; x < P2; x += kNT) {
                const int y = x ^ j;
                if (y > x) {
                    const U ka = sk[x], kb = sk[y];
                    const unsigned long long pa = sp[x], pb = sp[y];
                    const bool up = (x & k) == 0;
                    if (entry_less(kb, pb, ka, pa) == up) { sk[x] = kb; sk[y] = ka; sp[x] = pb; sp[y] = pa; }
                }
            }
            __syncthreads();
        }
    const int nh = ncand < nbest ? ncand : nbest;                         // (<= na <= K, so <= nb)
    if (tid == 0) nhyp[b] = nh;

    // ---- one lane per hypothesis: backwards through the slots, forwards for the sums
    for (int r = tid; r < nh; r += kNT) {
        int k = (int) (sp[r] & ((1ull << kWordSlotBits) - 1ull));
        const int kl = k;
        long long *lsr = lm_states ? lm_states + (ob + r) * T : nullptr;
        [[maybe_unused]] int rr = row_top;                                // (the ring: the row of frame base + t, stepped)
        for (int t = len - 1; t >= 0; --t) {
            if (k < 0 || k >= K) k = 0;                                   // (cannot happen: every kept pair stored its source's slot)
            const size_t at = (size_t) (kWin ? rr : t) * K + k;
            int q = bq[at];
            q = q < 0 ? 0 : (q >= Q ? Q - 1 : q);                         // (nor this: the column indexes the graph's arrays)
            cols[(size_t) t * nb + r] = q;
            if (lsr) lsr[t] = bh[at];
            k = bs[at];
            if constexpr (kWin) rr = ring_prev(rr, T);
        }
        if constexpr (kWin) {                                             // no forward pass: the score alone, from the pair's own sum
            R end = set_v[kl];
            int w;
            if (final) (void) word_end<R, LA>(f, fw, set_h[kl], set_q[kl], set_v[kl], end, w);
            else if constexpr (LA) end = word_prefix<R, LA>(f, set_h[kl], set_q[kl], end);
            scores[ob + r] = end;
            continue;
        }
        int qp = cols[r], ip = f.label[qp], h = f.lstart;
        R a = in ? in[(int64_t) ip * P.is2] : NINF;
        R gs = sw[qp], ls = (R) 0;
        for (int t = 1; t < len; ++t) {
            const int q = cols[(size_t) t * nb + r], i = f.label[q];
            if (in) a = (a + tr[(int64_t) i * P.ts0 + (int64_t) ip * P.ts1]) + in[(int64_t) t * P.is0 + (int64_t) i * P.is2];
            if (q != qp) {
                int lo = bg.orow[qp];
                const int e1 = bg.orow[qp + 1];
                int hi = e1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (oarc[mid].x < q) lo = mid + 1; else hi = mid;
                }
                gs = gs + ((lo < e1 && oarc[lo].x == q) ? ow[lo] : NINF);
                if (i == f.sep) {                                         // a word ended: the LM walk of the search, again
                    int h2;
                    R add;
                    if (f.step(h, f.wos[f.state[qp]], h2, add)) { h = h2; ls = ls + add; }
                    else ls = NINF;                                       // (cannot happen: the search took this edge)
                }
            }
            qp = q; ip = i;
        }
        R end = set_v[kl];                                                // from the pair's own sum (the key folds -0 into +0)
        if (final) {
            gs = gs + fw[qp];
            const int s = f.state[qp];
            R endw = f.ew[h];
            if (s != 0) {
                int h2;
                R add = NINF;
                endw = f.step(h, f.wos[s], h2, add) ? add + f.ew[h2] : NINF;
            }
            ls = ls + endw;
            int w;
            (void) word_end<R, LA>(f, fw, set_h[kl], set_q[kl], set_v[kl], end, w);
        } else if constexpr (LA) end = word_prefix<R, LA>(f, set_h[kl], set_q[kl], end);
        scores[ob + r] = end;
        if (escores) escores[ob + r] = a;
        gscores[ob + r] = gs;
        lscores[ob + r] = ls;
    }
    __threadfence();
    __syncthreads();

    // ---- one wavefront per output row
    for (int r = wave; r < nbest; r += kNT / 64) {
        long long *tk = tokens + (ob + r) * T, *wd = words + (ob + r) * T;
        long long *pb = path ? path + (ob + r) * T : nullptr, *st = states ? states + (ob + r) * T : nullptr;
        long long *ls = lm_states ? lm_states + (ob + r) * T : nullptr;
        if (r >= nh) {
            for (int t = lane; t < T; t += 64) {
                tk[t] = -1; wd[t] = -1;
                if (pb) pb[t] = -1;
                if (st) st[t] = -1;
                if (ls) ls[t] = -1;
            }
            if (lane == 0) {
                scores[ob + r] = NINF;
                if constexpr (!kWin) {
                    gscores[ob + r] = NINF; lscores[ob + r] = NINF;
                    if (escores) escores[ob + r] = NINF;
                }
                tlen[ob + r] = 0; wlen[ob + r] = 0;
            }
            continue;
        }
        int base = 0, wbase = 0;
        long long carry = kWin ? carry0 : -1;
        int carry_q = -1;
        for (int c0 = 0; c0 < len; c0 += 64) {
            const int t = c0 + lane;
            long long cur = -1;
            int q = -1;
            if (t < len) {
                q = cols[(size_t) t * nb + r];
                cur = f.label[q];
                if (pb) pb[t] = cur;
                if (st) st[t] = f.state[q];
            }
            long long prv = __shfl_up(cur, 1);
            int qv = __shfl_up(q, 1);
            if (lane == 0) { prv = carry; qv = carry_q; }
            const bool keep = t < len && cur != prv;
            const unsigned long long m = __ballot(keep);
            const int pre = __popcll(m & ((1ull << lane) - 1ull));
            if (keep) tk[base + pre] = cur;
            base += __popcll(m);
            // a separator edge is the one way into the separator's product state: the word is the one that ends in the node before
            // (the window: the label before column 0 is the last committed one, and there is none before the first frame)
            const bool wend = keep && cur == f.sep && (kWin ? prv >= 0 : t >= 1);
            const unsigned long long mw = __ballot(wend);
            const int wpre = __popcll(mw & ((1ull << lane) - 1ull));
            if constexpr (kWin) {                                         // ... and its automaton state the carried one
                if (wend) wd[wbase + wpre] = f.wos[t >= 1 ? f.state[qv] : ((unsigned) cstate0 < (unsigned) src.S ? cstate0 : 0)];
            } else if (wend) wd[wbase + wpre] = f.wos[f.state[qv]];
            wbase += __popcll(mw);
            carry = __shfl(cur, 63);
            carry_q = __shfl(q, 63);
        }
        if constexpr (kWin) {
            if (final) {                                                  // the word of the last step, from the set: the tail may be empty
                int q = set_q[(int) (sp[r] & ((1ull << kWordSlotBits) - 1ull))];
                q = q < 0 ? 0 : (q >= Q ? Q - 1 : q);
                const int s = f.state[q], wfin = s != 0 ? f.wos[s] : -1;
                if (wfin >= 0 && wbase < T) {                             // (a path that ends in a word has fewer separator edges than frames)
                    if (lane == 0) wd[wbase] = wfin;
                    ++wbase;
                }
            }
        } else {
            if (final && lane == 0) {                                     // the word of the last step (every row has an end)
                const int s = f.state[cols[(size_t) (len - 1) * nb + r]];
                if (s != 0) wd[wbase] = f.wos[s];
            }
            if (final) wbase += f.state[cols[(size_t) (len - 1) * nb + r]] != 0;
        }
        for (int t = base + lane; t < T; t += 64) tk[t] = -1;
        for (int t = wbase + lane; t < T; t += 64) wd[t] = -1;
        for (int t = len + lane; t < T; t += 64) {
            if (pb) pb[t] = -1;
            if (st) st[t] = -1;
            if (ls) ls[t] = -1;
        }
        if (lane == 0) { tlen[ob + r] = base; wlen[ob + r] = wbase; }
    }
}

template <typename R, bool LA, int SRC = kBeamWordNbestRows>
hipError_t launch_nbest_kernel(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                               const WordLookParam<LA> &look, const BeamWordNbestSrc &src, int B, int K, int nbest, int final,
                               void *scores, void *escores, void *gscores, void *lscores, long long *path, long long *tokens,
                               long long *tlen, long long *states, long long *lm_states, long long *words, long long *wlen,
                               long long *num_hyps, long long *frames, long long *status, hipStream_t stream,
                               long long *committed = nullptr) {
    int P2 = 1;
    while (P2 < K) P2 *= 2;
    const size_t dyn = (size_t) P2 * (8 + sizeof(typename Key<R>::U));
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const void *fn = (const void *) beam_word_nbest_kernel<R, LA, SRC>;
    if (dyn + 64 > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);
    hipLaunchKernelGGL((beam_word_nbest_kernel<R, LA, SRC>), dim3(B), dim3(kNT), dyn, stream, P, G, BG, LM, src, K, cap,
                       word_table_bits(cap), nbest, P2, final,
                       (R *) scores, (R *) escores, (R *) gscores, (R *) lscores, path, tokens, tlen, states, lm_states, words,
                       wlen, num_hyps, frames, committed, status, look);
    return hipGetLastError();
}

}  // namespace

// The n-best kernel alone over what a search of this family left (src), one-shot (final = 1, the lengths of the problem): behind
// the decoder's search here, behind beam_word_conf_search in asg_beam_word_nbest_conf.hip.  LA: that search's look-ahead, or NULL.
template <typename R>
hipError_t launch_beam_word_nbest_over(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                       const WordLookArgs *LA, const BeamWordNbestSrc &src, int K, int nbest, void *scores,
                                       void *emission_scores, void *graph_scores, void *lm_scores, long long *path,
                                       long long *tokens, long long *tlen, long long *states, long long *lm_states,
                                       long long *words, long long *wlen, long long *num_hyps, hipStream_t stream) {
    if (LA)
        return launch_nbest_kernel<R, true>(P, G, BG, LM, *LA, src, P.B, K, nbest, 1, scores, emission_scores, graph_scores, lm_scores,
                                            path, tokens, tlen, states, lm_states, words, wlen, num_hyps, nullptr, nullptr, stream);
    return launch_nbest_kernel<R, false>(P, G, BG, LM, WordNoLook{}, src, P.B, K, nbest, 1, scores, emission_scores, graph_scores,
                                         lm_scores, path, tokens, tlen, states, lm_states, words, wlen, num_hyps, nullptr, nullptr,
                                         stream);
}
template hipError_t launch_beam_word_nbest_over<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                                       const WordLookArgs *, const BeamWordNbestSrc &, int, int, void *, void *,
                                                       void *, void *, long long *, long long *, long long *, long long *,
                                                       long long *, long long *, long long *, long long *, hipStream_t);
template hipError_t launch_beam_word_nbest_over<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                                        const WordLookArgs *, const BeamWordNbestSrc &, int, int, void *, void *,
                                                        void *, void *, long long *, long long *, long long *, long long *,
                                                        long long *, long long *, long long *, long long *, hipStream_t);

BeamWordNbestLayout beam_word_nbest_layout(int elem, int T, int K, int cap, int nbest) {
    BeamWordNbestLayout l{};
    l.nb = nbest < K ? nbest : K;
    size_t off = beam_word_work_layout(elem, T, K, cap, word_table_bits(cap)).end;   // the word decoder's own part, at the front
    l.fin = off;  off += a256(8 + (size_t) K * (elem + 8));
    l.rows = off; off += a256((size_t) T * l.nb * 4);
    l.per = off;
    return l;
}

size_t beam_word_nbest_work_bytes(int elem, int T, int B, int K, int cap, int nbest) {
    return (size_t) B * beam_word_nbest_layout(elem, T, K, cap, nbest).per + tail_bytes(T, B);
}

size_t beam_word_stream_nbest_work_bytes(int max_frames, int B, int K, int nbest) {
    return (size_t) B * a256((size_t) max_frames * (nbest < K ? nbest : K) * 4);
}

namespace {

// The search -- asg_beam_word.hip's, or with LA asg_beam_word_la.hip's -- asked to leave its last set, then the n-best kernel
// over what it left, on one stream.
template <typename R, bool LA>
hipError_t beam_words_nbest(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                            const WordLookParam<LA> &look, int K, double theta, int nbest, void *work, void *scores,
                            void *emission_scores, void *graph_scores, void *lm_scores, long long *path, long long *tokens,
                            long long *tlen, long long *states, long long *lm_states, long long *words, long long *wlen,
                            long long *num_hyps, hipStream_t stream) {
    const int T = P.T, B = P.B;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const BeamWordNbestLayout lay = beam_word_nbest_layout(sizeof(R), T, K, cap, nbest);
    char *w = (char *) work, *tail = w + (size_t) B * lay.per;
    const size_t bb = a256((size_t) B * 8), BT = (size_t) B * T;
    long long *wide = (long long *) (tail + 3 * bb);                        // path, tokens, states, lm_states, words of the one best
    hipError_t e;
    if constexpr (LA)
        e = launch_beam_words_la<R>(P, G, BG, LM, look, K, theta, work, tail, wide, wide + BT, (long long *) (tail + bb),
                                    wide + 2 * BT, wide + 3 * BT, wide + 4 * BT, (long long *) (tail + 2 * bb), stream, lay.per,
                                    lay.fin);
    else
        e = launch_beam_words<R>(P, G, BG, LM, K, theta, work, tail, wide, wide + BT, (long long *) (tail + bb), wide + 2 * BT,
                                 wide + 3 * BT, wide + 4 * BT, (long long *) (tail + 2 * bb), stream, lay.per, lay.fin);
    if (e != hipSuccess) return e;
    BeamWordNbestSrc src{};
    src.base = w; src.per = lay.per; src.set_off = lay.fin + 8; src.na_off = lay.fin; src.pos_off = 0; src.ovf_off = 0;
    src.cols = w + lay.rows; src.cols_per = lay.per; src.Tw = T; src.nb = lay.nb;
    return launch_nbest_kernel<R, LA>(P, G, BG, LM, look, src, B, K, nbest, 1, scores, emission_scores, graph_scores, lm_scores, path,
                                      tokens, tlen, states, lm_states, words, wlen, num_hyps, nullptr, nullptr, stream);
}

}  // namespace

template <typename R>
hipError_t launch_beam_words_nbest(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, int K,
                                   double theta, int nbest, void *work, void *scores, void *emission_scores, void *graph_scores,
                                   void *lm_scores, long long *path, long long *tokens, long long *tlen, long long *states,
                                   long long *lm_states, long long *words, long long *wlen, long long *num_hyps,
                                   hipStream_t stream) {
    return beam_words_nbest<R, false>(P, G, BG, LM, WordNoLook{}, K, theta, nbest, work, scores, emission_scores, graph_scores,
                                      lm_scores, path, tokens, tlen, states, lm_states, words, wlen, num_hyps, stream);
}
template <typename R>
hipError_t launch_beam_words_nbest_la(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                      const WordLookArgs &LA, int K, double theta, int nbest, void *work, void *scores,
                                      void *emission_scores, void *graph_scores, void *lm_scores, long long *path,
                                      long long *tokens, long long *tlen, long long *states, long long *lm_states,
                                      long long *words, long long *wlen, long long *num_hyps, hipStream_t stream) {
    return beam_words_nbest<R, true>(P, G, BG, LM, LA, K, theta, nbest, work, scores, emission_scores, graph_scores, lm_scores,
                                     path, tokens, tlen, states, lm_states, words, wlen, num_hyps, stream);
}
template hipError_t launch_beam_words_nbest<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, int,
                                                   double, int, void *, void *, void *, void *, void *, long long *, long long *,
                                                   long long *, long long *, long long *, long long *, long long *, long long *,
                                                   hipStream_t);
template hipError_t launch_beam_words_nbest<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, int,
                                                    double, int, void *, void *, void *, void *, void *, long long *, long long *,
                                                    long long *, long long *, long long *, long long *, long long *, long long *,
                                                    hipStream_t);
template hipError_t launch_beam_words_nbest_la<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                                      const WordLookArgs &, int, double, int, void *, void *, void *, void *, void *,
                                                      long long *, long long *, long long *, long long *, long long *, long long *,
                                                      long long *, long long *, hipStream_t);
template hipError_t launch_beam_words_nbest_la<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                                       const WordLookArgs &, int, double, int, void *, void *, void *, void *,
                                                       void *, long long *, long long *, long long *, long long *, long long *,
                                                       long long *, long long *, long long *, hipStream_t);

namespace {

template <typename R, bool LA>
hipError_t beam_word_stream_nbest(const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, const WordLookParam<LA> &look,
                                  int K, int max_frames, int B, const void *state, int final, int nbest, void *work, void *scores,
                                  void *graph_scores, void *lm_scores, long long *path, long long *tokens, long long *tlen,
                                  long long *states, long long *lm_states, long long *words, long long *wlen, long long *num_hyps,
                                  long long *frames, long long *status, hipStream_t stream, size_t stride) {
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const BeamStreamLayout lay = beam_word_stream_layout(sizeof(R), max_frames, K, cap);
    BeamWordNbestSrc src{};
    src.base = (const char *) state; src.per = stride ? stride : lay.per;   // (a slot with parts of the caller's behind it)
    src.set_off = lay.set; src.na_off = lay.hdr + 4; src.pos_off = lay.hdr;
    src.ovf_off = lay.hdr + 8;
    src.nb = nbest < K ? nbest : K;
    src.cols = (char *) work; src.cols_per = a256((size_t) max_frames * src.nb * 4); src.Tw = max_frames;
    Problem P{};                                                            // no emissions, no lengths: the state has both
    P.T = max_frames; P.B = B; P.N = 0;
    return launch_nbest_kernel<R, LA>(P, G, BG, LM, look, src, B, K, nbest, final != 0, scores, nullptr, graph_scores, lm_scores, path,
                                      tokens, tlen, states, lm_states, words, wlen, num_hyps, frames, status, stream);
}

}  // namespace

template <typename R>
hipError_t launch_beam_word_stream_nbest(const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, int K, int max_frames,
                                         int B, const void *state, int final, int nbest, void *work, void *scores,
                                         void *graph_scores, void *lm_scores, long long *path, long long *tokens, long long *tlen,
                                         long long *states, long long *lm_states, long long *words, long long *wlen,
                                         long long *num_hyps, long long *frames, long long *status, hipStream_t stream,
                                         size_t stride) {
    return beam_word_stream_nbest<R, false>(G, BG, LM, WordNoLook{}, K, max_frames, B, state, final, nbest, work, scores,
                                            graph_scores, lm_scores, path, tokens, tlen, states, lm_states, words, wlen, num_hyps,
                                            frames, status, stream, stride);
}
template <typename R>
hipError_t launch_beam_word_stream_nbest_la(const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                            const WordLookArgs &LA, int K, int max_frames, int B, const void *state, int final,
                                            int nbest, void *work, void *scores, void *graph_scores, void *lm_scores,
                                            long long *path, long long *tokens, long long *tlen, long long *states,
                                            long long *lm_states, long long *words, long long *wlen, long long *num_hyps,
                                            long long *frames, long long *status, hipStream_t stream, size_t stride) {
    return beam_word_stream_nbest<R, true>(G, BG, LM, LA, K, max_frames, B, state, final, nbest, work, scores, graph_scores,
                                           lm_scores, path, tokens, tlen, states, lm_states, words, wlen, num_hyps, frames, status,
                                           stream, stride);
}
template hipError_t launch_beam_word_stream_nbest<float>(const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, int, int, int,
                                                         const void *, int, int, void *, void *, void *, void *, long long *,
                                                         long long *, long long *, long long *, long long *, long long *,
                                                         long long *, long long *, long long *, long long *, hipStream_t, size_t);
template hipError_t launch_beam_word_stream_nbest<double>(const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, int, int, int,
                                                          const void *, int, int, void *, void *, void *, void *, long long *,
                                                          long long *, long long *, long long *, long long *, long long *,
                                                          long long *, long long *, long long *, long long *, hipStream_t, size_t);
template hipError_t launch_beam_word_stream_nbest_la<float>(const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                                            const WordLookArgs &, int, int, int, const void *, int, int, void *,
                                                            void *, void *, void *, long long *, long long *, long long *,
                                                            long long *, long long *, long long *, long long *, long long *,
                                                            long long *, long long *, hipStream_t, size_t);
template hipError_t launch_beam_word_stream_nbest_la<double>(const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                                             const WordLookArgs &, int, int, int, const void *, int, int, void *,
                                                             void *, void *, void *, long long *, long long *, long long *,
                                                             long long *, long long *, long long *, long long *, long long *,
                                                             long long *, long long *, hipStream_t, size_t);

size_t beam_word_window_nbest_work_bytes(int W, int B, int K, int nbest) {
    return (size_t) B * a256((size_t) W * (nbest < K ? nbest : K) * 4);
}

// The kernel over a window state: the slot is a word stream's of W frames with the rows kept as rings and WordWinHdr at lay.hdr.
template <typename R>
hipError_t launch_beam_word_window_nbest(const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                         const WordLookArgs *LA, int S, int K, int W, int B, const void *state, int final,
                                         int nbest, void *work, void *scores, long long *path, long long *tokens, long long *tlen,
                                         long long *states, long long *lm_states, long long *words, long long *wlen,
                                         long long *num_hyps, long long *frames, long long *committed, long long *status,
                                         hipStream_t stream) {
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const BeamStreamLayout lay = beam_word_window_layout(sizeof(R), W, K, cap);
    BeamWordNbestSrc src{};
    src.base = (const char *) state; src.per = lay.per; src.set_off = lay.set; src.pos_off = lay.hdr;
    src.nb = nbest < K ? nbest : K;
    src.cols = (char *) work; src.cols_per = a256((size_t) W * src.nb * 4); src.Tw = W; src.S = S;
    Problem P{};                                                            // no emissions, no lengths: the state has both
    P.T = W; P.B = B; P.N = 0;
    if (LA)
        return launch_nbest_kernel<R, true, kBeamWordNbestWindow>(P, G, BG, LM, *LA, src, B, K, nbest, final != 0, scores, nullptr,
                                                                  nullptr, nullptr, path, tokens, tlen, states, lm_states, words,
                                                                  wlen, num_hyps, frames, status, stream, committed);
    return launch_nbest_kernel<R, false, kBeamWordNbestWindow>(P, G, BG, LM, WordNoLook{}, src, B, K, nbest, final != 0, scores,
                                                               nullptr, nullptr, nullptr, path, tokens, tlen, states, lm_states,
                                                               words, wlen, num_hyps, frames, status, stream, committed);
}
#define ASG_BEAM_WORD_WINDOW_NBEST_INST(R)                                                                                      \
    template hipError_t launch_beam_word_window_nbest<R>(const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,           \
                                                         const WordLookArgs *, int, int, int, int, const void *, int, int, void *, \
                                                         void *, long long *, long long *, long long *, long long *, long long *, \
                                                         long long *, long long *, long long *, long long *, long long *,        \
                                                         long long *, hipStream_t);
ASG_BEAM_WORD_WINDOW_NBEST_INST(float)
ASG_BEAM_WORD_WINDOW_NBEST_INST(double)
#undef ASG_BEAM_WORD_WINDOW_NBEST_INST

}  // namespace asg
