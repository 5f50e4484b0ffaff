// torch_asg_amd/csrc/asg_beam_word_window.hip -- WINDOWED streaming beam decoding with a lexicon and a word n-gram LM on gfx950:
// the stream of asg_beam_word_stream.hip in bounded memory, as asg_beam_window.hip is the stream of asg_beam_stream.hip.  The
// search is the one over pairs (LM history h, lexicon product state q) of asg_beam_word_frame.h, compiled into this translation
// unit as into the other three, but the back-pointers live in a RING of W rows -- frame u in row u mod W -- and the prefix of the
// transcript on which all surviving hypotheses agree is COMMITTED: handed out by the advance that finds it, in labels, automaton
// states, LM states, tokens and WORDS, and never looked at again.  The specification is
// include/asg_hip.h::asg_beam_word_window_advance; tests/beam_word_window_ref.py restates it.  The window never touches the
// search: the frame body reads its sources from the set in LDS and writes the row it is given.
//
// One slot of the state (beam_word_window_layout; every part 256-byte aligned):
//   the one-shot word decoder's workspace of one utterance with T = W (asg_beam_common.h, beam_word_work_layout): bq / bh / bs
//     int32 [W][K], the table tkey u64 [C], arg u64 [C], val key [C], ckey key [cap], cpair u64 [cap], touched int32 [cap];
//   a 256-byte header: int64 pos (frames consumed), int64 base (frames committed), int32 |A|, carry (label of the last committed
//     frame, -1: none), carry_state (its automaton state, -1: none), status (bit 0: a forced commit has happened);
//   the stored set: values [K] (dtype), then product states int32 [K], then LM states int32 [K].
// Three kernels, each one launch, no host synchronisation, no copy, no memset:
//   beam_word_window_reset_kernel    per chosen slot: the header (carries -1) and the whole table emptied.
//   beam_word_window_advance_kernel  one 1024-thread workgroup per slot: the frames of the chunk through beam_word_frame, a commit
//                                    attempt after every frame whose count is a multiple of P, the eight outputs with their padding.
//   beam_word_window_result_kernel   one workgroup per slot: the best end over the stored set, the backtrace over the uncommitted
//                                    tail (at most W steps), its token and word collapse started from the carries.  It only reads.
// A commit attempt is asg_beam_window.hip's over the slots of pairs, and the same text: asg_beam_window_common.h holds the
// convergence scan (window_converge), the clamp of a slot's header (window_header), the forced commit's arithmetic
// (window_forced) and window_commit, where one lane walks the converged slot's chain down to `base`, one wavefront collapses the
// labels into tokens and -- for this family -- another finds the words (collapse_words_from, asg_beam_word_frame.h): a word is
// the separator behind another label, and the label and state before the first frame of a segment are the carries, so an edge
// that straddles two commits or two calls gives its word once.  This unit keeps its header, its control blocks and its call of
// word_best_end.
//
// With LM look-ahead (include/asg_hip.h::asg_beam_word_window_advance_la) the advance and result kernels are compiled a second
// time with the frame's look-ahead flag on.  Convergence looks at slots only and is the same text; the forced commit follows the
// best prefix pair, which word_best_end then ranks by value minus look-ahead (word_prefix); the state has the same bytes.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"
#include "asg_beam_window_common.h"   // the commit attempt, shared with asg_beam_window.hip

namespace asg {

namespace {

// The window's control blocks sit behind Ctl (at 0) and WordCtl (at kWordCtlOff, the 64-bit select and reduction block) inside
// the fixed LDS: the fixed block stays kFixedLds bytes.
constexpr size_t kWinCtlOff = (kWordCtlOff + sizeof(WordCtl) + 63) & ~(size_t) 63;
constexpr size_t kWinOutOff = kWinCtlOff + 64;

// The header of a slot (asg_beam_window_common.h has it, for the n-best kernel that reads it).
using WinHdr = WordWinHdr;

// What a commit attempt shares.
struct WinCtl {
    long long base;              // frames committed so far
    int carry, carry_state, status;
    int ncommit, ntok, nword;    // frames / tokens / words this call has appended to its outputs
    WinScan scan;
};

// What the commits of one call write to, and the ring they read (LDS: a commit is rare, and the frame loop keeps its scalar
// registers for the search).
struct WinOut {
    static constexpr bool kWords = true;     // (window_commit: the ring bh, the output nl, the wavefront that finds the words)
    static constexpr bool kFrames = false;   // (... and no start frames of the tokens)
    const int *bq, *bh, *bs;     // the ring [W][K]
    int K, Q, W, S, sep;
    const int *label, *state, *wos;
    long long *np, *ns, *nl, *nt, *nw;   // this slot's rows of new_path / new_states / new_lm_states / new_tokens / new_words
    long long cols;              // W + Tc
};
static_assert(sizeof(WinCtl) <= 64 && kWinOutOff + sizeof(WinOut) <= kFixedLds, "control blocks");

__global__ void __launch_bounds__(256) beam_word_window_reset_kernel(char *state, BeamStreamLayout lay, BeamWordWorkLayout wl,
                                                                      unsigned C, int key_bytes, const unsigned char *mask) {
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;
    char *wb = state + (size_t) b * lay.per;
    beam_word_reset_tables(wb, wl, C, key_bytes);
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        WinHdr *h = (WinHdr *) (wb + lay.hdr);
        h->pos = 0; h->base = 0; h->na = 0; h->carry = -1; h->carry_state = -1; h->status = 0;
    }
}

template <typename R, bool TRL, bool LA = false>
__global__ void __launch_bounds__(kBT) beam_word_window_advance_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, int S,
                                                                       int K, R theta, int cap, int tbits, int W, int CP,
                                                                       char *state, BeamStreamLayout lay, long long *new_path,
                                                                       long long *new_states, long long *new_lm_states,
                                                                       long long *new_tokens, long long *new_words,
                                                                       long long *new_frames, long long *new_tlen,
                                                                       long long *new_wlen, WordLookParam<LA> la) {
    using KT = Key<R>;
    using U = typename KT::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Ctl<U> &ctl = *(Ctl<U> *) lds;
    WordCtl &wctl = *(WordCtl *) (lds + kWordCtlOff);
    WinCtl &wc = *(WinCtl *) (lds + kWinCtlOff);
    WinOut &o = *(WinOut *) (lds + kWinOutOff);
    unsigned *mark = (unsigned *) (lds + kFixedLds);       // the two mark sets of the scan
    R *cur_v = (R *) (lds + kFixedLds + mark_bytes(K));    // [K]
    int *cur_q = (int *) (cur_v + K);                      // [K]
    int *cur_h = cur_q + K;                                // [K]
    R *trs = (R *) (cur_h + K);                            // [N][N] if TRL (2 * K ints: aligned)
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = P.N;
    char *wb = state + (size_t) b * lay.per;
    WinHdr *hdr = (WinHdr *) (wb + lay.hdr);
    R *set_v = (R *) (wb + lay.set);                        // values [K], then product states [K], then LM states [K]
    const long long cols = (long long) W + P.T;
    long long *np = new_path + (int64_t) b * cols, *ns = new_states + (int64_t) b * cols, *nl = new_lm_states + (int64_t) b * cols;
    long long *nt = new_tokens + (int64_t) b * cols, *nwd = new_words + (int64_t) b * cols;
    if (tid == 0) {
        o.bq = nullptr; o.bh = nullptr; o.bs = nullptr;
        o.K = K; o.Q = g.Q; o.W = W; o.S = S; o.sep = lm.sep; o.label = g.label; o.state = g.state; o.wos = lm.word_of_state;
        o.np = np; o.ns = ns; o.nl = nl; o.nt = nt; o.nw = nwd; o.cols = cols;
    }

    long long pos = hdr->pos, base0 = hdr->base;
    int na0 = hdr->na;
    window_header(pos, base0, na0, K);
    if (na0 > 0) base0 = window_live_base(pos, base0, W);
    const int n = clamp_len(P.in_len, b, P.T);
    if (tid == 0) {
        wc.base = base0; wc.carry = hdr->carry; wc.carry_state = hdr->carry_state; wc.status = hdr->status;
        wc.ncommit = 0; wc.ntok = 0; wc.nword = 0;
    }

    if (n >= 1) {
        const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
        const R *tr = (const R *) P.transition;
        BeamWordFrame<R, LA> f;
        f.ctl = &ctl; f.wctl = &wctl; f.cur_v = cur_v; f.cur_q = cur_q; f.cur_h = cur_h; f.trs = trs; f.tr = tr;
        f.ts0 = P.ts0; f.ts1 = P.ts1; f.N = N; f.theta = theta;
        bind_graph<R>(f, g, bg, lm, K, cap, tbits);
        bind_look<R>(f, la);
        int *bq, *bh, *bs;
        f.bind_work(wb, W, bq, bh, bs);
        if (tid == 0) { o.bq = bq; o.bh = bh; o.bs = bs; }

        beam_word_load_set<R, TRL, LA>(f, trs, set_v, na0);

        int row = (int) (pos % W), ph = (int) (pos % CP);   // the next frame's row, and pos mod P; both kept by stepping
        for (int t = 0; t < n; ++t) {
            const long long gt = pos + t;                   // the frame's index in the utterance
            int na = ctl.na;
            if (gt >= 1 && na == 0) break;                  // an empty beam stays empty (and commits nothing more)
            const int fr = row;
            beam_word_frame<R, TRL, LA>(f, gt == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bh, bs, fr);
            const long long p1 = gt + 1;                    // pos, counting this frame
            row = row + 1 == W ? 0 : row + 1;
            ph = ph + 1 == CP ? 0 : ph + 1;
            na = ctl.na;
            na = na < K ? na : K;
            if (ph != 0 || na == 0) continue;
            // ================================================================ commit attempt
            // ---- convergence: the latest frame at which every survivor has the same ancestor
            long long base = wc.base;
            int cslot, crow;
            const long long c = window_converge(bs, K, W, na, p1, base, fr, mark, wc.scan, cslot, crow);
            if (c >= base) {
                window_commit(wc, o, c, crow, c, cslot);
                base = wc.base;
            }
            // ---- forced commit: the next CP frames must not overwrite a live row
            const long long F = window_forced(p1, base, W, CP);
            if (F > 0) {
                U bkey;
                int bk;
                word_best_end<R, LA>(f, nullptr, false, cur_h, cur_q, cur_v, na, bkey, bk);  // the best prefix
                __syncthreads();                            // (the reduction slots are read before anything reuses them)
                if (bkey != 0 && bk >= 0) {
                    if (tid == 0) wc.status |= 1;
                    window_commit(wc, o, p1 - 1, fr, base + F - 1, bk);
                }
            }
        }
        const int na = beam_word_store_set<R, LA>(f, set_v);
        if (tid == 0) hdr->na = na;
    }
    __syncthreads();
    const int nc = wc.ncommit, ntk = wc.ntok, nwo = wc.nword;
    for (long long x = nc + tid; x < cols; x += kBT) { np[x] = -1; ns[x] = -1; nl[x] = -1; }
    for (long long x = ntk + tid; x < cols; x += kBT) nt[x] = -1;
    for (long long x = nwo + tid; x < cols; x += kBT) nwd[x] = -1;
    if (tid == 0) {
        new_frames[b] = nc;
        new_tlen[b] = ntk;
        new_wlen[b] = nwo;
        hdr->pos = pos + n; hdr->base = wc.base; hdr->carry = wc.carry; hdr->carry_state = wc.carry_state; hdr->status = wc.status;
    }
}

template <typename R, bool LA = false>
__global__ void __launch_bounds__(kBT) beam_word_window_result_kernel(GraphArgs g, WordLmArgs lm, int S, int K, int cap, int tbits,
                                                                      int W, const char *state, BeamStreamLayout lay, int final,
                                                                      R *scores, long long *path, long long *tokens, long long *tlen,
                                                                      long long *states, long long *lm_states, long long *words,
                                                                      long long *wlen, long long *frames, long long *committed,
                                                                      long long *status, WordLookParam<LA> la) {
    using U = typename Key<R>::U;
    __shared__ WordCtl wctl;
    __shared__ int wfin_s;
    const int tid = threadIdx.x, b = blockIdx.x;
    const R NINF = Num<R>::ninf();
    char *wb = const_cast<char *>(state) + (size_t) b * lay.per;            // (only read: bind_work takes the workspace as it is)
    const WinHdr *hdr = (const WinHdr *) (wb + lay.hdr);
    const R *set_v = (const R *) (wb + lay.set);
    const int *set_q = (const int *) (set_v + K);
    const int *set_h = set_q + K;
    long long *pb = path + (int64_t) b * W, *tk = tokens + (int64_t) b * W, *st = states + (int64_t) b * W;
    long long *ls = lm_states + (int64_t) b * W, *wd = words + (int64_t) b * W;
    BeamWordFrame<R, LA> f;
    f.ctl = nullptr; f.wctl = &wctl; f.cur_v = nullptr; f.cur_q = nullptr; f.cur_h = nullptr; f.trs = nullptr; f.tr = nullptr;
    f.ts0 = 0; f.ts1 = 0; f.N = 0; f.theta = (R) 0;
    bind_graph<R>(f, g, BeamGraphArgs{}, lm, K, cap, tbits);
    bind_look<R>(f, la);
    int *bq, *bh, *bs;
    f.bind_work(wb, W, bq, bh, bs);
    long long pos = hdr->pos, base = hdr->base;
    int na = hdr->na;
    window_header(pos, base, na, K);
    if (tid == 0) {
        frames[b] = pos;
        committed[b] = base;
        status[b] = (hdr->status & 1) | (pos >= 1 && na == 0 ? 2 : 0);
    }
    const R *fw = (const R *) g.final_w;
    U bkey;
    int bk;
    word_best_end<R, LA>(f, fw, final != 0, set_h, set_q, set_v, na, bkey, bk);
    if (bkey == 0 || bk < 0) {                              // no frame yet, an empty set, or no finite end
        word_no_path(W, pb, tk, st, ls, wd, tlen + b, wlen + b);
        if (tid == 0) scores[b] = NINF;
        return;
    }
    base = window_live_base(pos, base, W);                  // (a set that is not empty has pos <= base + W)
    const int live = (int) (pos - base);                    // 0 .. W
    for (int t = live + tid; t < W; t += kBT) { pb[t] = -1; st[t] = -1; ls[t] = -1; }
    if (tid == 0) {
        R e = set_v[bk];
        int wfin = -1;
        if (final) (void) word_end<R, LA>(f, fw, set_h[bk], set_q[bk], set_v[bk], e, wfin);
        else e = word_prefix<R, LA>(f, set_h[bk], set_q[bk], set_v[bk]);
        scores[b] = e;
        wfin_s = wfin;
        int k = bk, r = (int) ((pos + W - 1) % W);          // the row of frame pos - 1
        for (long long t = pos - 1; t >= base; --t, r = ring_prev(r, W)) {
            long long lab = -1, sta = -1, lms = -1;
            if ((unsigned) k < (unsigned) K) {               // (always: every kept pair stored its source's slot)
                const int64_t at = (int64_t) r * K + k;
                int q = bq[at];
                q = (unsigned) q < (unsigned) g.Q ? q : 0;
                lms = bh[at];
                k = bs[at];
                lab = g.label[q];
                sta = g.state[q];
            }
            pb[t - base] = lab; st[t - base] = sta; ls[t - base] = lms;
        }
    }
    __threadfence();
    __syncthreads();
    if (tid < 64) {
        long long carry = hdr->carry;
        const int nt = collapse_tokens_from(pb, live, carry, tk, tid);
        for (int t = nt + tid; t < W; t += 64) tk[t] = -1;
        if (tid == 0) tlen[b] = nt;
    } else if (tid < 128) {
        const int l = tid - 64;
        int nw = collapse_words_from(pb, st, live, hdr->carry, hdr->carry_state, lm.sep, lm.word_of_state, S, wd, l);
        const int wfin = wfin_s;
        if (wfin >= 0 && nw < W) {                          // (a path that ends in a word has fewer separator edges than frames)
            if (l == 0) wd[nw] = wfin;
            ++nw;
        }
        for (int t = nw + l; t < W; t += 64) wd[t] = -1;
        if (l == 0) wlen[b] = nw;
    }
}

}  // namespace

// The slot of a word window stream is the slot of a word stream of W frames: the ring has the [frame][K] layout with W rows.
BeamStreamLayout beam_word_window_layout(int elem, int W, int K, int cap) { return beam_word_stream_layout(elem, W, K, cap); }

size_t beam_word_window_state_bytes(int elem, int W, int B, int K, int cap) {
    return (size_t) B * beam_word_window_layout(elem, W, K, cap).per;
}

hipError_t launch_beam_word_window_reset(int elem, const BeamGraphArgs &BG, int K, int W, int B, void *state,
                                         const unsigned char *mask, hipStream_t stream) {
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const BeamStreamLayout lay = beam_word_window_layout(elem, W, K, cap);
    const int tbits = word_table_bits(cap);
    const size_t C = (size_t) 1 << tbits;
    hipLaunchKernelGGL(beam_word_window_reset_kernel, dim3(B, reset_blocks(C)), dim3(256), 0, stream, (char *) state, lay,
                       beam_word_work_layout(elem, W, K, cap, tbits), (unsigned) C, elem, mask);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_word_window_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                           const WordLookArgs *LA, int S, int K, double theta, int W, int CP, void *state,
                                           long long *new_path,
                                           long long *new_states, long long *new_lm_states, long long *new_tokens,
                                           long long *new_words, long long *new_frames, long long *new_tlen, long long *new_wlen,
                                           hipStream_t stream) {
    const int N = P.N;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const int tbits = word_table_bits(cap);
    const BeamStreamLayout lay = beam_word_window_layout(sizeof(R), W, K, cap);
    // the LDS of the word stream plus the two mark sets: control blocks, marks, the set, and the transitions when they fit
    const size_t beam = kFixedLds + mark_bytes(K) + (size_t) K * (sizeof(R) + 8);
    const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
    const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
#define ASG_BEAM_WORD_WINDOW(TRL, LAF, LOOK)                                                                                   \
    do {                                                                                                                       \
        const void *fn = (const void *) beam_word_window_advance_kernel<R, TRL, LAF>;                                         \
        if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);         \
        hipLaunchKernelGGL((beam_word_window_advance_kernel<R, TRL, LAF>), dim3(P.B), dim3(kBT), dyn, stream, P, G, BG, LM,   \
                           S, K, (R) theta, cap, tbits, W, CP, (char *) state, lay, new_path, new_states, new_lm_states,       \
                           new_tokens, new_words, new_frames, new_tlen, new_wlen, LOOK);                                       \
    } while (0)
    if (LA) { if (trl) ASG_BEAM_WORD_WINDOW(true, true, *LA); else ASG_BEAM_WORD_WINDOW(false, true, *LA); }
    else if (trl) ASG_BEAM_WORD_WINDOW(true, false, WordNoLook{}); else ASG_BEAM_WORD_WINDOW(false, false, WordNoLook{});
#undef ASG_BEAM_WORD_WINDOW
    return hipGetLastError();
}
template hipError_t launch_beam_word_window_advance<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &,
                                                           const WordLmArgs &, const WordLookArgs *, int, int, double, int, int, void *, long long *,
                                                           long long *, long long *, long long *, long long *, long long *,
                                                           long long *, long long *, hipStream_t);
template hipError_t launch_beam_word_window_advance<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &,
                                                            const WordLmArgs &, const WordLookArgs *, int, int, double, int, int, void *, long long *,
                                                            long long *, long long *, long long *, long long *, long long *,
                                                            long long *, long long *, hipStream_t);

template <typename R>
hipError_t launch_beam_word_window_result(const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                          const WordLookArgs *LA, int S, int K, int W, int B, const void *state, int final, void *scores, long long *path, long long *tokens,
                                          long long *tlen, long long *states, long long *lm_states, long long *words,
                                          long long *wlen, long long *frames, long long *committed, long long *status,
                                          hipStream_t stream) {
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const BeamStreamLayout lay = beam_word_window_layout(sizeof(R), W, K, cap);
#define ASG_BEAM_WORD_WINDOW_RESULT(LAF, LOOK)                                                                                 \
    hipLaunchKernelGGL((beam_word_window_result_kernel<R, LAF>), dim3(B), dim3(kBT), 0, stream, G, LM, S, K, cap,              \
                       word_table_bits(cap), W, (const char *) state, lay, final, (R *) scores, path, tokens, tlen, states,    \
                       lm_states, words, wlen, frames, committed, status, LOOK)
    if (LA) ASG_BEAM_WORD_WINDOW_RESULT(true, *LA); else ASG_BEAM_WORD_WINDOW_RESULT(false, WordNoLook{});
#undef ASG_BEAM_WORD_WINDOW_RESULT
    return hipGetLastError();
}
template hipError_t launch_beam_word_window_result<float>(const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                                          const WordLookArgs *, int, int, int, int, const void *, int, void *, long long *, long long *, long long *,
                                                          long long *, long long *, long long *, long long *, long long *,
                                                          long long *, long long *, hipStream_t);
template hipError_t launch_beam_word_window_result<double>(const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                                           const WordLookArgs *, int, int, int, int, const void *, int, void *, long long *, long long *, long long *,
                                                           long long *, long long *, long long *, long long *, long long *,
                                                           long long *, long long *, hipStream_t);

}  // namespace asg
