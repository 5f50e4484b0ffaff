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
//   the one-shot word decoder's workspace of one utterance with T = W: bq / bh / bs int32 [W][K], the table tkey u64 [C], arg u64
//     [C], val key [C], ckey key [cap], cpair u64 [cap], touched int32 [cap];
//   a 256-byte header: int64 pos (frames consumed), int64 base (frames committed), int32 |A|, carry (label of the last committed
//     frame, -1: none), carry_state (its automaton state, -1: none), status (bit 0: a forced commit has happened);
//   the stored set: values [K] (dtype), then product states int32 [K], then LM states int32 [K].
// Three kernels, each one launch, no host synchronisation, no copy, no memset:
//   beam_word_window_reset_kernel    per chosen slot: the header (carries -1) and the whole table emptied.
//   beam_word_window_advance_kernel  one 1024-thread workgroup per slot: the frames of the chunk through beam_word_frame, a commit
//                                    attempt after every frame whose count is a multiple of P, the eight outputs with their padding.
//   beam_word_window_result_kernel   one workgroup per slot: the best end over the stored set, the backtrace over the uncommitted
//                                    tail (at most W steps), its token and word collapse started from the carries.  It only reads.
// A commit attempt is asg_beam_window.hip's over the slots of pairs: the convergence scan marks, frame by frame backwards, the
// slots that some survivor descends from -- two K-bit sets in LDS, lanes striding over the slots, an integer atomicOr per marked
// slot, a popcount to count them -- and stops where one slot is left; one lane then walks that slot's chain down to `base`, one
// wavefront collapses the labels into tokens and another finds the words: a word is the separator behind another label, and the
// label and state before the first frame of a segment are the carries, so an edge that straddles two commits or two calls gives
// its word once.  The rows of this call's frames were written by this workgroup with plain stores and are read after a
// __syncthreads (beam_word_frame ends with one); those of earlier calls cross a kernel boundary.  Integer atomics only, and the
// marks are a set: bit-identical run to run.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"

namespace asg {

namespace {

inline size_t a256(size_t x) { return (x + 255) / 256 * 256; }

constexpr int kResetBlocks = 64;         // workgroups per slot in the reset
// The window's control blocks sit behind Ctl (at 0) and WordCtl (at kWordCtlOff, the 64-bit select and reduction block) inside
// the fixed LDS: the fixed block stays kFixedLds bytes.
constexpr size_t kWinCtlOff = (kWordCtlOff + sizeof(WordCtl) + 63) & ~(size_t) 63;
constexpr size_t kWinOutOff = kWinCtlOff + 64;

// The header of a slot.
struct WinHdr {
    long long pos, base;
    int na, carry, carry_state, status;
};
static_assert(sizeof(WinHdr) <= 256, "header");

// What a commit attempt shares.
struct WinCtl {
    long long base;              // frames committed so far
    int carry, carry_state, status;
    int ncommit, ntok, nword;    // frames / tokens / words this call has appended to its outputs
    int cnt[2];                  // |R| of the scan's steps, alternating
    int slot;                    // a marked slot (the one, when |R| == 1)
};

// What the commits of one call write to, and the ring they read (LDS: a commit is rare, and the frame loop keeps its scalar
// registers for the search).
struct WinOut {
    const int *bq, *bh, *bs;     // the ring [W][K]
    int K, Q, W, S, sep;
    const int *label, *state, *wos;
    long long *np, *ns, *nl, *nt, *nw;   // this slot's rows of new_path / new_states / new_lm_states / new_tokens / new_words
    long long cols;              // W + Tc
};
static_assert(sizeof(WinCtl) <= 64 && kWinOutOff + sizeof(WinOut) <= kFixedLds, "control blocks");

// The bytes of the two mark sets for K slots, kept a multiple of 16 so that the set behind them stays aligned.
__host__ __device__ inline size_t mark_bytes(int K) { return ((size_t) 2 * ((K + 31) / 32) * 4 + 15) & ~(size_t) 15; }

// One wavefront: the words of a SEGMENT of a path that continues an earlier one.  pb / st [0..len) are the labels and automaton
// states behind a frame whose label was `carry` and whose state was `carry_state` (-1: there is no such frame).  A word ends
// where the separator stands behind another label: it is the word of the state before.  They go to wd[0..), nothing is padded.
// -> the number appended; every lane gets it.
__device__ inline int collapse_words_from(const long long *pb, const long long *st, int len, long long carry, long long carry_state,
                                          int sep, const int *wos, int S, long long *wd, int lane) {
    int base = 0;
    for (int c0 = 0; c0 < len; c0 += 64) {
        const int t = c0 + lane;
        const long long cur = t < len ? pb[t] : -1, curs = t < len ? st[t] : -1;
        long long prv = __shfl_up(cur, 1), prvs = __shfl_up(curs, 1);
        if (lane == 0) { prv = carry; prvs = carry_state; }
        const bool keep = t < len && cur == sep && prv != sep && prv >= 0;
        const unsigned long long m = __ballot(keep);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (keep) wd[base + pre] = wos[(unsigned long long) prvs < (unsigned long long) S ? (int) prvs : 0];
        base += __popcll(m);
        carry = __shfl(cur, 63);             // (the last block's carries are not used again)
        carry_state = __shfl(curs, 63);
    }
    return base;
}

__global__ void __launch_bounds__(256) beam_word_window_reset_kernel(char *state, BeamStreamLayout lay, unsigned C, int key_bytes,
                                                                      size_t tkey_off, size_t arg_off, size_t val_off,
                                                                      const unsigned char *mask) {
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;
    char *wb = state + (size_t) b * lay.per;
    unsigned long long *tkey = (unsigned long long *) (wb + tkey_off), *arg = (unsigned long long *) (wb + arg_off);
    for (unsigned s = blockIdx.y * 256 + threadIdx.x; s < C; s += gridDim.y * 256) {
        dev_store(tkey + s, 0ull);
        dev_store(arg + s, ~0ull);
        if (key_bytes == 8) dev_store((unsigned long long *) (wb + val_off) + s, 0ull);
        else dev_store((unsigned int *) (wb + val_off) + s, 0u);
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        WinHdr *h = (WinHdr *) (wb + lay.hdr);
        h->pos = 0; h->base = 0; h->na = 0; h->carry = -1; h->carry_state = -1; h->status = 0;
    }
}

// The parts of a BeamWordFrame that do not depend on the call: the graph, the LM and the shape of the search.
template <typename R>
__device__ __forceinline__ void bind_graph(BeamWordFrame<R> &f, const GraphArgs &g, const BeamGraphArgs &bg, const WordLmArgs &lm,
                                           int K, int cap, int tbits) {
    f.K = K; f.G = beam_lanes_per_state(K); f.cap = cap; f.sep = lm.sep; f.tbits = tbits;
    f.qbits = bits_of(g.Q); f.pbits = f.qbits + bits_of(lm.H);
    f.label = g.label; f.state = g.state; f.orow = bg.orow; f.start_q = bg.start_q; f.num_start = bg.num_start;
    f.oarc = (const int2 *) bg.oarc; f.ow = (const R *) bg.ow; f.sw = (const R *) g.start_w;
    f.lrow = lm.row; f.lword = lm.word; f.lnext = lm.next; f.lback = lm.backoff; f.wos = lm.word_of_state;
    f.lw = (const R *) lm.lw; f.bw = (const R *) lm.bw; f.ew = (const R *) lm.ew; f.lstart = lm.start;
}

// Commit the frames base .. cto on the path that passes slot k of frame `top`, which lives in row `r` (base <= cto <= top <
// base + W): one lane walks the chain, one wavefront collapses the segment's labels behind `carry`, another finds its words
// behind `carry` / `carry_state`.  The whole workgroup calls it; it begins after and ends with a __syncthreads.
__device__ __forceinline__ void window_commit(WinCtl &wc, const WinOut &o, long long top, int r, long long cto, int k) {
    const int tid = threadIdx.x;
    const long long base = wc.base;
    const int c0 = wc.ncommit, t0 = wc.ntok, w0 = wc.nword;
    const long long carry0 = wc.carry, cstate0 = wc.carry_state;
    long long room = o.cols - c0;                            // (never short: committed <= the live frames before the call + n)
    int len = (int) (cto - base + 1);
    len = len < 0 ? 0 : ((long long) len > room ? (int) room : len);
    if (tid == 0) {
        const int K = o.K, W = o.W;
        long long t = top;
        for (; t > cto && (unsigned) k < (unsigned) K; --t, r = r == 0 ? W - 1 : r - 1) k = o.bs[(int64_t) r * K + k];
        for (; t > base + len - 1; --t) r = r == 0 ? W - 1 : r - 1;       // (only if the output row were short)
        for (; t >= base; --t, r = r == 0 ? W - 1 : r - 1) {
            long long lab = -1, sta = -1, lms = -1;
            if ((unsigned) k < (unsigned) K) {               // (always: every kept pair stored its source's slot)
                const int64_t at = (int64_t) r * K + k;
                int q = o.bq[at];
                q = (unsigned) q < (unsigned) o.Q ? q : 0;
                lms = o.bh[at];
                k = o.bs[at];
                lab = o.label[q];
                sta = o.state[q];
            }
            o.np[c0 + (t - base)] = lab;
            o.ns[c0 + (t - base)] = sta;
            o.nl[c0 + (t - base)] = lms;
        }
    }
    __threadfence();
    __syncthreads();
    if (tid < 64) {
        long long carry = carry0;
        const int nt = collapse_tokens_from(o.np + c0, len, carry, o.nt + t0, tid);
        if (tid == 0) { wc.ntok = t0 + nt; wc.carry = (int) carry; wc.ncommit = c0 + len; wc.base = base + len; }
    } else if (tid < 128) {
        const int nw = collapse_words_from(o.np + c0, o.ns + c0, len, carry0, cstate0, o.sep, o.wos, o.S, o.nw + w0, tid - 64);
        if (tid == 64) {
            wc.nword = w0 + nw;
            if (len > 0) wc.carry_state = (int) o.ns[c0 + len - 1];
        }
    }
    __syncthreads();
}

template <typename R, bool TRL>
__global__ void __launch_bounds__(kBT) beam_word_window_advance_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, int S,
                                                                       int K, R theta, int cap, int tbits, int W, int CP,
                                                                       char *state, BeamStreamLayout lay, long long *new_path,
                                                                       long long *new_states, long long *new_lm_states,
                                                                       long long *new_tokens, long long *new_words,
                                                                       long long *new_frames, long long *new_tlen,
                                                                       long long *new_wlen) {
    using KT = Key<R>;
    using U = typename KT::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Ctl<U> &ctl = *(Ctl<U> *) lds;
    WordCtl &wctl = *(WordCtl *) (lds + kWordCtlOff);
    WinCtl &wc = *(WinCtl *) (lds + kWinCtlOff);
    WinOut &o = *(WinOut *) (lds + kWinOutOff);
    const int nw = (K + 31) / 32;                          // words of a mark set
    unsigned *mark = (unsigned *) (lds + kFixedLds);       // [2][nw]
    R *cur_v = (R *) (lds + kFixedLds + mark_bytes(K));    // [K]
    int *cur_q = (int *) (cur_v + K);                      // [K]
    int *cur_h = cur_q + K;                                // [K]
    R *trs = (R *) (cur_h + K);                            // [N][N] if TRL (2 * K ints: aligned)
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
    const int N = P.N;
    char *wb = state + (size_t) b * lay.per;
    WinHdr *hdr = (WinHdr *) (wb + lay.hdr);
    R *set_v = (R *) (wb + lay.set);                        // [K]
    int *set_q = (int *) (set_v + K);                       // [K]
    int *set_h = set_q + K;                                 // [K]
    const long long cols = (long long) W + P.T;
    long long *np = new_path + (int64_t) b * cols, *ns = new_states + (int64_t) b * cols, *nl = new_lm_states + (int64_t) b * cols;
    long long *nt = new_tokens + (int64_t) b * cols, *nwd = new_words + (int64_t) b * cols;
    if (tid == 0) {
        o.bq = nullptr; o.bh = nullptr; o.bs = nullptr;
        o.K = K; o.Q = g.Q; o.W = W; o.S = S; o.sep = lm.sep; o.label = g.label; o.state = g.state; o.wos = lm.word_of_state;
        o.np = np; o.ns = ns; o.nl = nl; o.nt = nt; o.nw = nwd; o.cols = cols;
    }

    // (a state that was reset holds 0 <= base <= pos, and pos <= base + W while its set is not empty: behind an empty set pos
    // goes on alone, and base is never used again)
    long long pos = hdr->pos;
    pos = pos < 0 ? 0 : pos;
    int na0 = pos >= 1 ? hdr->na : 0;
    na0 = na0 < 0 ? 0 : (na0 > K ? K : na0);
    long long base0 = hdr->base;
    base0 = base0 > pos ? pos : base0;
    base0 = na0 > 0 && base0 < pos - W ? pos - W : base0;
    base0 = base0 < 0 ? 0 : base0;
    const int n = clamp_len(P.in_len, b, P.T);
    if (tid == 0) {
        wc.base = base0; wc.carry = hdr->carry; wc.carry_state = hdr->carry_state; wc.status = hdr->status;
        wc.ncommit = 0; wc.ntok = 0; wc.nword = 0;
    }

    if (n >= 1) {
        const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
        const R *tr = (const R *) P.transition;
        BeamWordFrame<R> f;
        f.ctl = &ctl; f.wctl = &wctl; f.cur_v = cur_v; f.cur_q = cur_q; f.cur_h = cur_h; f.trs = trs; f.tr = tr;
        f.ts0 = P.ts0; f.ts1 = P.ts1; f.N = N; f.theta = theta;
        bind_graph<R>(f, g, bg, lm, K, cap, tbits);
        int *bq, *bh, *bs;
        f.bind_work(wb, W, bq, bh, bs);
        if (tid == 0) { o.bq = bq; o.bh = bh; o.bs = bs; }

        if constexpr (TRL)
            for (int x = tid; x < N * N; x += kBT) trs[x] = tr[(int64_t) (x / N) * P.ts0 + (int64_t) (x % N) * P.ts1];
        for (int k = tid; k < na0; k += kBT) { cur_v[k] = set_v[k]; cur_q[k] = set_q[k]; cur_h[k] = set_h[k]; }
        if (tid == 0) { ctl.na = na0; ctl.n = 0; }
        __syncthreads();

        int row = (int) (pos % W), ph = (int) (pos % CP);   // the next frame's row, and pos mod P; both kept by stepping
        for (int t = 0; t < n; ++t) {
            const long long gt = pos + t;                   // the frame's index in the utterance
            int na = ctl.na;
            if (gt >= 1 && na == 0) break;                  // an empty beam stays empty (and commits nothing more)
            const int fr = row;
            beam_word_frame<R, TRL>(f, gt == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bh, bs, fr);
            const long long p1 = gt + 1;                    // pos, counting this frame
            row = row + 1 == W ? 0 : row + 1;
            ph = ph + 1 == CP ? 0 : ph + 1;
            na = ctl.na;
            na = na < K ? na : K;
            if (ph != 0 || na == 0) continue;
            // ================================================================ commit attempt
            // ---- convergence: the latest frame at which every survivor has the same ancestor
            long long base = wc.base;
            long long c = -1;
            int cslot = 0, crow = fr;
            if (na == 1) c = p1 - 1;
            else {
                unsigned *cur = mark, *nxt = mark + nw;
                for (int w = tid; w < nw; w += kBT) {
                    const int lo = w * 32;
                    cur[w] = na >= lo + 32 ? ~0u : (na > lo ? (1u << (na - lo)) - 1u : 0u);
                    nxt[w] = 0;
                }
                if (tid == 0) { wc.cnt[0] = 0; wc.cnt[1] = 0; }
                __syncthreads();
                int par = 0, ru = fr;                       // ru: the row of frame u
                for (long long u = p1 - 1; u > base; --u, par ^= 1, ru = ru == 0 ? W - 1 : ru - 1) {
                    const int *bsu = bs + (int64_t) ru * K;
                    for (int k = tid; k < K; k += kBT)
                        if ((cur[k >> 5] >> (k & 31)) & 1u) {
                            const int s = bsu[k];
                            if ((unsigned) s < (unsigned) K) atomicOr(&nxt[s >> 5], 1u << (s & 31));
                        }
                    __syncthreads();
                    int mine = 0;
                    for (int w = tid; w < nw; w += kBT) {
                        const unsigned x = nxt[w];
                        cur[w] = 0;
                        mine += __popc(x);
                        if (x) wc.slot = w * 32 + __ffs((int) x) - 1;
                    }
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) mine += __shfl_xor(mine, d);
                    if (lane == 0 && mine) atomicAdd(&wc.cnt[par], mine);
                    if (tid == 0) wc.cnt[par ^ 1] = 0;
                    __syncthreads();
                    const int cnt = wc.cnt[par];
                    unsigned *sw = cur; cur = nxt; nxt = sw;
                    if (cnt <= 1) {                         // (never 0: every kept pair stored its source's slot)
                        if (cnt == 1) { c = u - 1; cslot = wc.slot; crow = ru == 0 ? W - 1 : ru - 1; }
                        break;
                    }
                }
            }
            if (c >= base) {
                window_commit(wc, o, c, crow, c, cslot);
                base = wc.base;
            }
            // ---- forced commit: the next CP frames must not overwrite a live row
            const long long live = p1 - base;
            if (live > W - CP) {
                const long long F = live - (W - CP);
                U bkey;
                int bk;
                word_best_end<R>(f, nullptr, false, cur_h, cur_q, cur_v, na, bkey, bk);      // the best prefix
                __syncthreads();                            // (the reduction slots are read before anything reuses them)
                if (bkey != 0 && bk >= 0) {
                    if (tid == 0) wc.status |= 1;
                    window_commit(wc, o, p1 - 1, fr, base + F - 1, bk);
                }
            }
        }
        int na = ctl.na;
        na = na < K ? na : K;
        for (int k = tid; k < na; k += kBT) { set_v[k] = cur_v[k]; set_q[k] = cur_q[k]; set_h[k] = cur_h[k]; }
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

template <typename R>
__global__ void __launch_bounds__(kBT) beam_word_window_result_kernel(GraphArgs g, WordLmArgs lm, int S, int K, int cap, int tbits,
                                                                      int W, const char *state, BeamStreamLayout lay, int final,
                                                                      R *scores, long long *path, long long *tokens, long long *tlen,
                                                                      long long *states, long long *lm_states, long long *words,
                                                                      long long *wlen, long long *frames, long long *committed,
                                                                      long long *status) {
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
    BeamWordFrame<R> f;
    f.ctl = nullptr; f.wctl = &wctl; f.cur_v = nullptr; f.cur_q = nullptr; f.cur_h = nullptr; f.trs = nullptr; f.tr = nullptr;
    f.ts0 = 0; f.ts1 = 0; f.N = 0; f.theta = (R) 0;
    bind_graph<R>(f, g, BeamGraphArgs{}, lm, K, cap, tbits);
    int *bq, *bh, *bs;
    f.bind_work(wb, W, bq, bh, bs);
    long long pos = hdr->pos;
    pos = pos < 0 ? 0 : pos;
    long long base = hdr->base;
    base = base > pos ? pos : base;
    base = base < 0 ? 0 : base;
    int na = pos >= 1 ? hdr->na : 0;
    na = na < 0 ? 0 : (na > K ? K : na);
    if (tid == 0) {
        frames[b] = pos;
        committed[b] = base;
        status[b] = (hdr->status & 1) | (pos >= 1 && na == 0 ? 2 : 0);
    }
    const R *fw = (const R *) g.final_w;
    U bkey;
    int bk;
    word_best_end<R>(f, fw, final != 0, set_h, set_q, set_v, na, bkey, bk);
    if (bkey == 0 || bk < 0) {                              // no frame yet, an empty set, or no finite end
        word_no_path(W, pb, tk, st, ls, wd, tlen + b, wlen + b);
        if (tid == 0) scores[b] = NINF;
        return;
    }
    base = base < pos - W ? pos - W : base;                 // (a set that is not empty has pos <= base + W)
    const int live = (int) (pos - base);                    // 0 .. W
    for (int t = live + tid; t < W; t += kBT) { pb[t] = -1; st[t] = -1; ls[t] = -1; }
    if (tid == 0) {
        R e = set_v[bk];
        int wfin = -1;
        if (final) (void) word_end<R>(f, fw, set_h[bk], set_q[bk], set_v[bk], e, wfin);
        scores[b] = e;
        wfin_s = wfin;
        int k = bk, r = (int) ((pos + W - 1) % W);          // the row of frame pos - 1
        for (long long t = pos - 1; t >= base; --t, r = r == 0 ? W - 1 : r - 1) {
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
BeamStreamLayout beam_word_window_layout(int elem, int W, int K, int cap) {
    BeamStreamLayout l{};
    size_t off = beam_word_work_bytes(elem, W, 1, K, cap);
    l.hdr = off;  off += 256;
    l.set = off;  off += a256((size_t) K * (elem + 8));
    l.per = off;
    return l;
}

size_t beam_word_window_state_bytes(int elem, int W, int B, int K, int cap) {
    return (size_t) B * beam_word_window_layout(elem, W, K, cap).per;
}

hipError_t launch_beam_word_window_reset(int elem, const BeamGraphArgs &BG, int K, int W, int B, void *state,
                                         const unsigned char *mask, hipStream_t stream) {
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const BeamStreamLayout lay = beam_word_window_layout(elem, W, K, cap);
    const size_t C = (size_t) 1 << word_table_bits(cap);
    const size_t tkey_off = 3 * a256((size_t) W * K * 4), arg_off = tkey_off + a256(C * 8), val_off = arg_off + a256(C * 8);
    size_t by = (C + 255) / 256;
    by = by < 1 ? 1 : (by > (size_t) kResetBlocks ? (size_t) kResetBlocks : by);
    hipLaunchKernelGGL(beam_word_window_reset_kernel, dim3(B, (unsigned) by), dim3(256), 0, stream, (char *) state, lay, (unsigned) C,
                       elem, tkey_off, arg_off, val_off, mask);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_word_window_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, int S,
                                           int K, double theta, int W, int CP, void *state, long long *new_path,
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
#define ASG_BEAM_WORD_WINDOW(TRL)                                                                                              \
    do {                                                                                                                       \
        const void *fn = (const void *) beam_word_window_advance_kernel<R, TRL>;                                              \
        if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);         \
        hipLaunchKernelGGL((beam_word_window_advance_kernel<R, TRL>), dim3(P.B), dim3(kBT), dyn, stream, P, G, BG, LM, S, K,  \
                           (R) theta, cap, tbits, W, CP, (char *) state, lay, new_path, new_states, new_lm_states, new_tokens, \
                           new_words, new_frames, new_tlen, new_wlen);                                                         \
    } while (0)
    if (trl) ASG_BEAM_WORD_WINDOW(true); else ASG_BEAM_WORD_WINDOW(false);
#undef ASG_BEAM_WORD_WINDOW
    return hipGetLastError();
}
template hipError_t launch_beam_word_window_advance<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &,
                                                           const WordLmArgs &, int, int, double, int, int, void *, long long *,
                                                           long long *, long long *, long long *, long long *, long long *,
                                                           long long *, long long *, hipStream_t);
template hipError_t launch_beam_word_window_advance<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &,
                                                            const WordLmArgs &, int, int, double, int, int, void *, long long *,
                                                            long long *, long long *, long long *, long long *, long long *,
                                                            long long *, long long *, hipStream_t);

template <typename R>
hipError_t launch_beam_word_window_result(const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, int S, int K, int W,
                                          int B, const void *state, int final, void *scores, long long *path, long long *tokens,
                                          long long *tlen, long long *states, long long *lm_states, long long *words,
                                          long long *wlen, long long *frames, long long *committed, long long *status,
                                          hipStream_t stream) {
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const BeamStreamLayout lay = beam_word_window_layout(sizeof(R), W, K, cap);
    hipLaunchKernelGGL((beam_word_window_result_kernel<R>), dim3(B), dim3(kBT), 0, stream, G, LM, S, K, cap, word_table_bits(cap), W,
                       (const char *) state, lay, final, (R *) scores, path, tokens, tlen, states, lm_states, words, wlen, frames,
                       committed, status);
    return hipGetLastError();
}
template hipError_t launch_beam_word_window_result<float>(const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, int, int, int,
                                                          int, const void *, int, void *, long long *, long long *, long long *,
                                                          long long *, long long *, long long *, long long *, long long *,
                                                          long long *, long long *, hipStream_t);
template hipError_t launch_beam_word_window_result<double>(const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, int, int, int,
                                                           int, const void *, int, void *, long long *, long long *, long long *,
                                                           long long *, long long *, long long *, long long *, long long *,
                                                           long long *, long long *, hipStream_t);

}  // namespace asg
