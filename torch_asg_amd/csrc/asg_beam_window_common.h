// torch_asg_amd/csrc/asg_beam_window_common.h -- what the two WINDOWED streaming decoders share besides the search: the commit
// attempt of asg_beam_window.hip (product states) and asg_beam_word_window.hip (pairs, with the extra ring bh, the output of LM
// states and the words).  A window never touches the search, so none of this is on the per-frame path: a commit attempt runs after
// every P-th frame, and everything here works on the ring of source slots bs [W][K] alone -- frame u in row u mod W -- which both
// families keep in the same form.  The scan marks, frame by frame backwards, the slots that some survivor descends from -- two K-bit sets in LDS, lanes striding
// over the slots, an integer atomicOr per marked slot, a popcount to count them -- and stops where one slot is left.  The rows
// of this call's frames were written by this workgroup with plain stores and are read after a __syncthreads (a frame ends with
// one); those of earlier calls cross a kernel boundary.  Integer atomics only, and the marks are a set: bit-identical run to run.
// Each unit includes its frame header first and keeps its own WinHdr, WinCtl and WinOut; WinOut::kWords selects the word parts.
// (The families' WinHdr are TokenWinHdr and WordWinHdr below: asg_beam_nbest.hip and asg_beam_word_nbest.hip read a window's
// header too, with window_header, window_live_base and ring_prev.)
#pragma once
#include "asg_beam_frame.h"

namespace asg {

namespace {

// The bytes of the two mark sets for K slots, kept a multiple of 16 so that the set behind them stays aligned.
__host__ __device__ inline size_t mark_bytes(int K) { return ((size_t) 2 * ((K + 31) / 32) * 4 + 15) & ~(size_t) 15; }

// The row of the frame before the one in row r.
__device__ __forceinline__ int ring_prev(int r, int W) { return r == 0 ? W - 1 : r - 1; }

// What the scan shares (LDS, inside each family's WinCtl).
struct WinScan {
    int cnt[2];              // |R| of the scan's steps, alternating
    int slot;                // a marked slot (the one, when |R| == 1)
};

// The header of a slot of the token family's window: asg_beam_window.hip keeps it (as its WinHdr), and the n-best kernel of
// asg_beam_nbest.hip reads it.
struct TokenWinHdr {
    long long pos, base;
    int na, carry, status;
};
static_assert(sizeof(TokenWinHdr) <= 256, "header");

// The header of a slot of the word family's window: asg_beam_word_window.hip keeps it (as its WinHdr), and the n-best kernel of
// asg_beam_word_nbest.hip reads it.
struct WordWinHdr {
    long long pos, base;
    int na, carry, carry_state, status;
};
static_assert(sizeof(WordWinHdr) <= 256, "header");

// The header of a slot as the kernels use it.  A state that was reset holds 0 <= base <= pos, and pos <= base + W while its set
// is not empty: behind an empty set pos goes on alone, and base is never used again.  -> pos >= 0, 0 <= na <= K (0 before the
// first frame), 0 <= base <= pos.  The last invariant, base >= pos - W, is window_live_base: the advance applies it when the set
// is not empty, the result after it has reported `committed` and found an end.
__device__ __forceinline__ void window_header(long long &pos, long long &base, int &na, int K) {
    pos = pos < 0 ? 0 : pos;
    na = pos >= 1 ? na : 0;
    na = na < 0 ? 0 : (na > K ? K : na);
    base = base > pos ? pos : base;
    base = base < 0 ? 0 : base;
}
__device__ __forceinline__ long long window_live_base(long long pos, long long base, int W) {
    return base < pos - W ? pos - W : base;
}

// The convergence scan over the ring bs after frame p1 - 1, which lives in row `fr` and kept na >= 1 slots: -> the latest frame
// c in base .. p1 - 1 at which every survivor has the same ancestor, with that ancestor's slot and its row; -1: the survivors
// still differ at frame `base`.  The whole workgroup calls it, after a __syncthreads; `mark` holds the two sets, [2][(K + 31) /
// 32] words.
__device__ __forceinline__ long long window_converge(const int *bs, int K, int W, int na, long long p1, long long base, int fr,
                                                     unsigned *mark, WinScan &sc, int &cslot, int &crow) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int nw = (K + 31) / 32;                           // words of a mark set
    long long c = -1;
    cslot = 0; crow = fr;
    if (na == 1) return p1 - 1;
    unsigned *cur = mark, *nxt = mark + nw;
    for (int w = tid; w < nw; w += kBT) {
        const int lo = w * 32;
        cur[w] = na >= lo + 32 ? ~0u : (na > lo ? (1u << (na - lo)) - 1u : 0u);
        nxt[w] = 0;
    }
    if (tid == 0) { sc.cnt[0] = 0; sc.cnt[1] = 0; }
    __syncthreads();
    int par = 0, ru = fr;                                   // ru: the row of frame u
    for (long long u = p1 - 1; u > base; --u, par ^= 1, ru = ring_prev(ru, W)) {
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
            if (x) sc.slot = w * 32 + __ffs((int) x) - 1;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) mine += __shfl_xor(mine, d);
        if (lane == 0 && mine) atomicAdd(&sc.cnt[par], mine);
        if (tid == 0) sc.cnt[par ^ 1] = 0;
        __syncthreads();
        const int cnt = sc.cnt[par];
        unsigned *sw = cur; cur = nxt; nxt = sw;
        if (cnt <= 1) {                                     // (never 0: every kept slot stored its source's slot)
            if (cnt == 1) { c = u - 1; cslot = sc.slot; crow = ring_prev(ru, W); }
            break;
        }
    }
    return c;
}

// The forced commit: with frames base .. p1 - 1 live, the next CP frames must not overwrite a live row.  -> how many frames
// have to be committed for that, 0: none.
__device__ __forceinline__ long long window_forced(long long p1, long long base, int W, int CP) {
    const long long live = p1 - base;
    return live > W - CP ? live - (W - CP) : 0;
}

// One wavefront, behind collapse_tokens_from over the same segment: the absolute frame at which every kept label was kept --
// frame `first` + t for pb[t] -- to tf[0..), the walk of beam_conf_tokens (asg_beam_conf_pull.h) with the segment's carry.
__device__ inline void collapse_frames_from(const long long *pb, int len, long long carry, long long first, long long *tf,
                                            int lane) {
    int base = 0;
    for (int c0 = 0; c0 < len; c0 += 64) {
        const int t = c0 + lane;
        const long long cur = t < len ? pb[t] : -1;
        long long prv = __shfl_up(cur, 1);
        if (lane == 0) prv = carry;
        const bool keep = t < len && cur != prv;
        const unsigned long long m = __ballot(keep);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (keep) tf[base + pre] = first + t;
        base += __popcll(m);
        carry = __shfl(cur, 63);                             // (only read when another 64 frames follow)
    }
}

// Commit the frames base .. cto on the path that passes slot k of frame `top`, which lives in row `r` (base <= cto <= top <
// base + W): one lane walks the chain, one wavefront collapses the segment's labels behind `carry`, and with WO::kWords another
// finds its words behind `carry` / `carry_state`; with WO::kFrames (the lattice-keeping token window, asg_beam_conf_window.hip)
// the first wavefront also writes every committed token's start frame to o.tf.  The whole workgroup calls it; it begins after and
// ends with a __syncthreads.
// (A slot outside 0 .. K-1 cannot happen; if it did, the token family would stop writing the segment, the word family pad with -1.)
template <typename WC, typename WO>
__device__ __forceinline__ void window_commit(WC &wc, const WO &o, long long top, int r, long long cto, int k) {
    const int tid = threadIdx.x;
    const long long base = wc.base;
    const int c0 = wc.ncommit;
    // (the word family's second wavefront needs the carries as they are now, before the first replaces `carry`: read here)
    int w0 = 0;
    long long wcarry = -1, wcstate = -1;
    if constexpr (WO::kWords) { w0 = wc.nword; wcarry = wc.carry; wcstate = wc.carry_state; }
    long long room = o.cols - c0;                            // (never short: committed <= the live frames before the call + n)
    int len = (int) (cto - base + 1);
    len = len < 0 ? 0 : ((long long) len > room ? (int) room : len);
    if (tid == 0) {
        const int K = o.K, W = o.W;
        long long t = top;
        for (; t > cto && (unsigned) k < (unsigned) K; --t, r = ring_prev(r, W)) k = o.bs[(int64_t) r * K + k];
        for (; t > base + len - 1; --t) r = ring_prev(r, W);              // (only if the output row were short)
        for (; t >= base; --t, r = ring_prev(r, W)) {
            long long lab = -1, sta = -1, lms = -1;
            if ((unsigned) k < (unsigned) K) {
                const int64_t at = (int64_t) r * K + k;
                int q = o.bq[at];
                q = (unsigned) q < (unsigned) o.Q ? q : 0;
                if constexpr (WO::kWords) lms = o.bh[at];
                k = o.bs[at];
                lab = o.label[q];
                sta = o.state[q];
            } else if constexpr (!WO::kWords) break;
            o.np[c0 + (t - base)] = lab;
            o.ns[c0 + (t - base)] = sta;
            if constexpr (WO::kWords) o.nl[c0 + (t - base)] = lms;
        }
    }
    __threadfence();
    __syncthreads();
    if (tid < 64) {
        const int t0 = wc.ntok;
        long long carry = wc.carry;
        if constexpr (WO::kFrames) collapse_frames_from(o.np + c0, len, carry, base, o.tf + t0, tid);
        const int nt = collapse_tokens_from(o.np + c0, len, carry, o.nt + t0, tid);
        if (tid == 0) { wc.ntok = t0 + nt; wc.carry = (int) carry; wc.ncommit = c0 + len; wc.base = base + len; }
    }
    if constexpr (WO::kWords) {
        if (tid >= 64 && tid < 128) {
            const int nw = collapse_words_from(o.np + c0, o.ns + c0, len, wcarry, wcstate, o.sep, o.wos, o.S, o.nw + w0, tid - 64);
            if (tid == 64) {
                wc.nword = w0 + nw;
                if (len > 0) wc.carry_state = (int) o.ns[c0 + len - 1];
            }
        }
    }
    __syncthreads();
}

}  // namespace

}  // namespace asg
