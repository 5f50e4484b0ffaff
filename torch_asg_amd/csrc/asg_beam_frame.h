// torch_asg_amd/csrc/asg_beam_frame.h -- the device code of ONE FRAME of the beam search, and of its end (best final state,
// backtrace, token collapse), shared by the one-shot decoder (asg_beam_graph.hip: beam_graph_kernel walks every frame of an
// utterance in one launch) and the streaming decoder (asg_beam_stream.hip: beam_stream_advance_kernel enters the frame loop with
// the set an earlier call left, beam_stream_result_kernel is the end as a call of its own).  Both translation units compile this
// one text, so the sets, the back-pointers and every tie are the same bit for bit: that is what "decoding in chunks equals
// decoding in one call" rests on (include/asg_hip.h::asg_beam_stream_advance), as the beam-pruned loss already rests on it.
// The steps of a frame are described at the top of asg_beam_graph.hip.  Behind the frame: what the two streams (asg_beam_stream.hip,
// asg_beam_window.hip) share around it -- the clearing loop of their resets (beam_reset_tables) and the way their advance kernels
// enter and leave the frame loop (beam_load_set, beam_store_set).
#pragma once
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"

namespace asg {

namespace {

constexpr int kBT = 1024;          // workgroup
constexpr int kSlotBits = 16;      // arg = source q << 16 | source slot: K <= 2^16 slots, q < 2^31
constexpr size_t kLdsMax = 160 * 1024;
constexpr size_t kFixedLds = 4096; // histograms, counters, reduction slots

template <typename U> __device__ __forceinline__ U dev_load(const U *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename U> __device__ __forceinline__ void dev_store(U *p, U v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One wavefront: tokens[0..T) of one utterance from its finished path[0..len), -1 behind them, and the token count (the
// convention of asg_decode_graph.hip).
__device__ inline void collapse_tokens(const long long *pb, int len, int T, long long *tk, long long *tl, int lane) {
    int base = 0;
    long long carry = -1;
    for (int c0 = 0; c0 < len; c0 += 64) {
        const int t = c0 + lane;
        const long long cur = t < len ? pb[t] : -1;
        long long prv = __shfl_up(cur, 1);
        if (lane == 0) prv = carry;
        const bool keep = t < len && cur != prv;
        const unsigned long long m = __ballot(keep);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (keep) tk[base + pre] = cur;
        base += __popcll(m);
        carry = __shfl(cur, 63);
    }
    for (int t = base + lane; t < T; t += 64) tk[t] = -1;
    if (lane == 0) *tl = base;
}

// One wavefront: the same collapse for a SEGMENT of a path that continues an earlier one (asg_beam_window.hip): pb[0..len) are
// the labels behind a frame whose label was `carry` (-1: none), so a first label equal to `carry` is no token.  The kept labels
// go to tk[0..) -- the caller passes the next free column -- and nothing is padded.  -> the number appended; `carry` becomes the
// segment's last label (unchanged for len == 0).  Every lane gets both.
__device__ inline int collapse_tokens_from(const long long *pb, int len, long long &carry, long long *tk, int lane) {
    int base = 0;
    for (int c0 = 0; c0 < len; c0 += 64) {
        const int t = c0 + lane;
        const long long cur = t < len ? pb[t] : -1;
        long long prv = __shfl_up(cur, 1);
        if (lane == 0) prv = carry;
        const bool keep = t < len && cur != prv;
        const unsigned long long m = __ballot(keep);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (keep) tk[base + pre] = cur;
        base += __popcll(m);
        const int last = len - c0 < 64 ? len - c0 - 1 : 63;
        carry = __shfl(cur, last);
    }
    return base;
}

// Append for the lanes with `want` (all lanes of the wavefront that are in the enclosing loop call it): one bump of the LDS
// counter per wavefront; -> the lane's position.
__device__ __forceinline__ int wave_append(bool want, int *counter) {
    const unsigned long long m = __ballot(want);
    if (m == 0) return 0;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long) m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(counter, __popcll(m));
    base = __shfl(base, leader);
    return base + __popcll(m & ((1ull << lane) - 1ull));
}

// Shared control block (the front of the dynamic LDS).
template <typename U>
struct Ctl {
    int hist[2][256];
    U kmax, kmin;            // largest / smallest candidate key of the frame
    U kth;                   // select: the K-th key (or lo when everything that passes lo is taken)
    U pre;                   // radix select: the digits fixed so far
    int need;                // radix select: how many are still to take among the keys that match `pre`
    int qcut;                // the largest q taken among the keys equal to kth (0x7FFFFFFF: all of them)
    int n;                   // touched count
    int na;                  // active count
    int done;                // radix select: finished early
    int bq, bk;              // final argmax
    unsigned long long redv[kBT / 64];
    int redq[kBT / 64], redk[kBT / 64];
};
static_assert(sizeof(Ctl<unsigned long long>) <= kFixedLds, "control block");

// Wavefront 0: the digit at which the counts, walked from the top (DESC) or the bottom (!DESC), reach `need`; -> (digit, the
// count strictly before it).  256 bins, four per lane.
template <bool DESC>
__device__ __forceinline__ void find_digit(const int *hist, int need, int lane, int &digit, int &before) {
    int c[4], s = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const int bin = DESC ? 255 - (4 * lane + x) : 4 * lane + x;
        c[x] = hist[bin];
        s += c[x];
    }
    int incl = s;                                    // inclusive scan over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    int excl = incl - s;
    const bool mine = excl < need && incl >= need;
    int d = -1, bf = 0;
    if (mine) {
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            if (d < 0 && excl + c[x] >= need) { d = DESC ? 255 - (4 * lane + x) : 4 * lane + x; bf = excl; }
            excl += c[x];
        }
    }
    const unsigned long long m = __ballot(mine);
    const int src = m ? __ffsll((long long) m) - 1 : 0;
    digit = __shfl(d, src);
    before = __shfl(bf, src);
}

// What the frames of one utterance share: the LDS of its workgroup and its slot arrays in global memory (one utterance's part
// of the workspace: asg_kernels.h, BeamGraphArgs).
template <typename R>
struct BeamFrame {
    using U = typename Key<R>::U;
    Ctl<U> *ctl;
    R *cur_v;                    // LDS [K] values of the active set
    int *cur_q;                  // LDS [K] its product states
    const R *trs;                // LDS [N][N] transitions (TRL)
    const R *tr;                 // ... or in global memory, strides ts0 / ts1
    int64_t ts0, ts1;
    int N, Q, K, G;              // G lanes per active state in the expansion
    R theta;
    const int *label, *orow, *start_q;
    int num_start;
    const int2 *oarc;
    const R *ow, *sw;
    unsigned long long *arg;     // [Q]
    U *val;                      // [Q]
    U *ckey;                     // [cap]
    int *tl;                     // [cap] the touched list

    // The utterance's slot arrays inside its workspace `wb` (beam_work for T frames); -> the [T][K] lists through bq / bs.
    __device__ __forceinline__ void bind_work(char *wb, int T, int cap, int *&bq, int *&bs) {
        const BeamWork<char *> l = beam_work(wb, sizeof(U), T, Q, K, cap);
        bq = (int *) l.bq;  bs = (int *) l.bs;  arg = (unsigned long long *) l.arg;
        val = (U *) l.val;  ckey = (U *) l.ckey;  tl = (int *) l.tl;
    }
};

// Subgroup of G lanes per active state: wide when the beam is narrow.
__device__ __forceinline__ int beam_lanes_per_state(int K) {
    int G = 1;
    while (G < 64 && G * 2 * K <= kBT) G *= 2;
    return G;
}

// One frame: from the active set (f.cur_q, f.cur_v)[0..na) of the frame before -- or, with `first`, from the start states -- to
// the new one, with (q, source slot) of every kept state into row `row` of the [.][K] lists bq / bs.  `xt` are the frame's
// emissions (stride is2).  The whole workgroup calls it; it begins after and ends with a __syncthreads.  val / arg of every
// touched q are empty again on return (a first frame does not use them), f.ctl->na holds the new count and f.ctl->n is 0.
template <typename R, bool TRL>
__device__ __forceinline__ void beam_frame(const BeamFrame<R> &f, bool first, int na, const R *xt, int64_t is2, int *bq, int *bs,
                                           int row) {
    using KT = Key<R>;
    using U = typename KT::U;
    Ctl<U> &ctl = *f.ctl;
    const int tid = threadIdx.x, lane = tid & 63;
    const int K = f.K, G = f.G, Q = f.Q, N = f.N;
    (void) N;
    const R NINF = Num<R>::ninf();
    const R theta = f.theta;
    R *cur_v = f.cur_v;
    int *cur_q = f.cur_q;
    unsigned long long *arg = f.arg;
    U *val = f.val, *ckey = f.ckey;
    int *tl = f.tl;
    const int2 *oarc = f.oarc;
    const R *ow = f.ow, *sw = f.sw;
    auto TR = [&](int i, int j) -> R {
        if constexpr (TRL) return f.trs[i * N + j];
        else return f.tr[(int64_t) i * f.ts0 + (int64_t) j * f.ts1];
    };
    const unsigned long long ARG_NONE = ~0ull;

    // ================================================================ candidates
    if (first) {
        const int ns = f.num_start;
        for (int j = tid; j < ns; j += kBT) tl[j] = f.start_q[j];
        if (tid == 0) ctl.n = ns;
    } else {
        for (int phase = 0; phase < 2; ++phase) {
            for (int k0 = 0; k0 < na; k0 += kBT / G) {
                const int k = k0 + tid / G, lg = tid % G;
                const bool act = k < na;
                int qs = 0, j = 0, e = 0, e1 = 0;
                R v = NINF;
                if (act) {
                    qs = cur_q[k]; v = cur_v[k]; j = f.label[qs];
                    e = f.orow[qs] + lg; e1 = f.orow[qs + 1];
                }
                const unsigned long long me = ((unsigned long long) qs << kSlotBits) | (unsigned) k;
                // the stay, then the row; the whole wavefront stays in the loop until its last lane is done (wave_append)
                bool stay = act && lg == 0;
                while (__any(stay || e < e1)) {
                    int tq = -1;
                    R c = NINF;
                    if (stay) { tq = qs; c = v + TR(j, j); stay = false; }
                    else if (e < e1) {
                        const int2 a = oarc[e];
                        tq = a.x;
                        c = (v + TR(a.y, j)) + ow[e];
                        e += G;
                    }
                    const bool ok = tq >= 0 && c > NINF;          // a -inf candidate never makes a candidate state
                    const U key = KT::enc(c);
                    if (phase == 0) {
                        bool fresh = false;
                        if (ok) fresh = atomicMax(val + tq, key) == 0;
                        const int pos = wave_append(fresh, &ctl.n);
                        if (fresh) tl[pos] = tq;
                    } else if (ok && dev_load(val + tq) == key) {
                        atomicMin(arg + tq, me);
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid < 256) { ctl.hist[0][tid] = 0; ctl.hist[1][tid] = 0; }
    if (tid == 0) { ctl.kmax = 0; ctl.kmin = ~(U) 0; ctl.na = 0; ctl.done = 0; ctl.qcut = 0x7FFFFFFF; }
    __syncthreads();
    // ================================================================ select
    const int n = ctl.n;
    {   // c = best + emission as keys; their maximum and minimum
        U mx = 0, mn = ~(U) 0;
        for (int j = tid; j < n; j += kBT) {
            const int q = tl[j];
            const R base = first ? sw[q] : KT::dec(dev_load(val + q));
            const R c = base + xt[(int64_t) f.label[q] * is2];
            const U key = c > NINF ? KT::enc(c) : (U) 0;
            ckey[j] = key;
            if (key) { mx = key > mx ? key : mx; mn = key < mn ? key : mn; }
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const U a = (U) __shfl_xor(mx, o), c2 = (U) __shfl_xor(mn, o);
            mx = a > mx ? a : mx; mn = c2 < mn ? c2 : mn;
        }
        if (lane == 0 && mx) { atomicMax(&ctl.kmax, mx); atomicMin(&ctl.kmin, mn); }
    }
    __syncthreads();
    const U kmax = ctl.kmax;
    U lokey = ~(U) 0;                                    // no candidate: nothing passes
    if (kmax) {
        lokey = KT::enc(KT::dec(kmax) - theta);
        const U kmin = ctl.kmin;
        const U from = lokey > kmin ? lokey : kmin;      // every key that passes lies in [from, kmax]
        // ---- the K-th key: 8-bit digits below the bits that `from` and kmax share
        int rem = from == kmax ? 0 : KT::kBits - (int) (sizeof(U) == 8 ? __clzll((long long) (from ^ kmax))
                                                                       : __clz((int) (from ^ kmax)));
        if (tid == 0) { ctl.pre = rem >= KT::kBits ? (U) 0 : (kmax >> rem); ctl.need = K; ctl.kth = lokey; }
        __syncthreads();
        bool first_pass = true;
        int hb = 0;
        if (rem == 0) {
            // every passing key equals kmax: count them through one histogram bin
            for (int j = tid; j < n; j += kBT) if (ckey[j] == kmax) atomicAdd(&ctl.hist[0][0], 1);
            __syncthreads();
            if (tid == 0) {
                const int cnt = ctl.hist[0][0];
                ctl.kth = kmax;
                if (cnt <= K) ctl.done = 1; else ctl.need = K;
                ctl.hist[0][0] = 0;
            }
            __syncthreads();
            first_pass = false;
        }
        while (rem > 0) {
            const int w = rem < 8 ? rem : 8, shift = rem - w;
            const U pre = ctl.pre;
            int *h = ctl.hist[hb];
            for (int j = tid; j < n; j += kBT) {
                const U key = ckey[j];
                if (key >= lokey && key != 0 && (rem >= KT::kBits || (key >> rem) == pre))
                    atomicAdd(&h[(int) ((key >> shift) & (U) ((1 << w) - 1))], 1);
            }
            if (tid < 256) ctl.hist[hb ^ 1][tid] = 0;
            __syncthreads();
            if (tid < 64) {
                int total = 0;
                if (first_pass) {                         // everything that passes lo: taken whole when it fits
                    for (int x = 0; x < 4; ++x) total += h[4 * lane + x];
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) total += __shfl_xor(total, o);
                }
                if (first_pass && total <= K) {
                    if (lane == 0) { ctl.done = 1; ctl.kth = lokey; }
                } else {
                    int d, before;
                    find_digit<true>(h, ctl.need, lane, d, before);
                    if (lane == 0) {
                        ctl.need -= before;
                        ctl.pre = (rem >= KT::kBits ? (U) 0 : (pre << w)) | (U) d;
                        if (shift == 0) {
                            ctl.kth = ctl.pre;
                            if (h[d] == ctl.need) ctl.done = 1;      // every key tied with the K-th is taken
                        }
                    }
                }
            }
            __syncthreads();
            if (ctl.done) break;
            first_pass = false;
            rem = shift;
            hb ^= 1;
        }
        // ---- ties at the K-th key: the `need` smallest q among them
        if (!ctl.done) {
            const U kth = ctl.kth;
            if (tid < 256) { ctl.hist[0][tid] = 0; ctl.hist[1][tid] = 0; }
            if (tid == 0) ctl.pre = 0;
            __syncthreads();
            int qrem = 32 - __clz(Q > 1 ? Q - 1 : 1);
            hb = 0;
            while (qrem > 0) {
                const int w = qrem < 8 ? qrem : 8, shift = qrem - w;
                const unsigned pre = (unsigned) ctl.pre;
                int *h = ctl.hist[hb];
                for (int j = tid; j < n; j += kBT) {
                    if (ckey[j] != kth) continue;
                    const unsigned q = (unsigned) tl[j];
                    if ((q >> qrem) == pre) atomicAdd(&h[(q >> shift) & ((1u << w) - 1u)], 1);
                }
                if (tid < 256) ctl.hist[hb ^ 1][tid] = 0;
                __syncthreads();
                if (tid < 64) {
                    int d, before;
                    find_digit<false>(h, ctl.need, lane, d, before);
                    if (lane == 0) {
                        ctl.need -= before;
                        ctl.pre = (U) ((pre << w) | (unsigned) d);
                        if (shift == 0) ctl.qcut = (int) ctl.pre;
                    }
                }
                __syncthreads();
                qrem = shift;
                hb ^= 1;
            }
        }
    }
    // ---- the new active set, the frame's back-pointers, and val / arg emptied
    {
        const U kth = ctl.kth;
        const int qcut = ctl.qcut;
        int *bqt = bq + (int64_t) row * K, *bst = bs + (int64_t) row * K;
        for (int j0 = 0; j0 < n; j0 += kBT) {
            const int j = j0 + tid;
            bool sel = false;
            int q = 0;
            U key = 0;
            if (j < n) {
                q = tl[j];
                key = ckey[j];
                sel = kmax != 0 && key != 0 && key >= lokey && (key > kth || (key == kth && q <= qcut));
            }
            const int slot = wave_append(sel, &ctl.na);
            if (sel && slot < K) {                       // (never more than K: the select counted them)
                cur_q[slot] = q;
                cur_v[slot] = KT::dec(key);
                bqt[slot] = q;
                bst[slot] = first ? -1 : (int) (dev_load(arg + q) & ((1ull << kSlotBits) - 1ull));
            }
            if (j < n && !first) { dev_store(val + q, (U) 0); dev_store(arg + q, ARG_NONE); }
        }
    }
    if (tid == 0) ctl.n = 0;
    __syncthreads();
}

// A stream's reset (asg_beam_stream.hip, asg_beam_window.hip): val = 0 and arg = none for all Q states of the slot at `wb`, shared
// among the workgroups of 256 threads that blockIdx.y counts; key_bytes is 4 or 8.
__device__ __forceinline__ void beam_reset_tables(char *wb, const BeamWorkLayout &l, int Q, int key_bytes) {
    unsigned long long *arg = (unsigned long long *) (wb + l.arg);
    for (int q = blockIdx.y * 256 + threadIdx.x; q < Q; q += gridDim.y * 256) {
        dev_store(arg + q, ~0ull);
        if (key_bytes == 8) dev_store((unsigned long long *) (wb + l.val) + q, 0ull);
        else dev_store((unsigned int *) (wb + l.val) + q, 0u);
    }
}

// A stream's advance (asg_beam_stream.hip, asg_beam_window.hip) enters the frame loop with the set an earlier call left at
// `set_v` -- values [K], then product states int32 [K]: the transitions into LDS when they live there, the na0 stored states into
// f.cur_v / f.cur_q, the counters.  The whole workgroup calls it; it ends with a __syncthreads.
template <typename R, bool TRL>
__device__ __forceinline__ void beam_load_set(const BeamFrame<R> &f, R *trs, const R *set_v, int na0) {
    const int tid = threadIdx.x, N = f.N;
    const int *set_q = (const int *) (set_v + f.K);
    if constexpr (TRL)
        for (int x = tid; x < N * N; x += kBT) trs[x] = f.tr[(int64_t) (x / N) * f.ts0 + (int64_t) (x % N) * f.ts1];
    for (int k = tid; k < na0; k += kBT) { f.cur_v[k] = set_v[k]; f.cur_q[k] = set_q[k]; }
    if (tid == 0) { f.ctl->na = na0; f.ctl->n = 0; }
    __syncthreads();
}
// ... and leaves it: the set back to `set_v`; -> its size, for the header.
template <typename R>
__device__ __forceinline__ int beam_store_set(const BeamFrame<R> &f, R *set_v) {
    int *set_q = (int *) (set_v + f.K);
    int na = f.ctl->na;
    na = na < f.K ? na : f.K;
    for (int k = threadIdx.x; k < na; k += kBT) { set_v[k] = f.cur_v[k]; set_q[k] = f.cur_q[k]; }
    return na;
}

// The best end over a set (sq, sv)[0..na): end = sv + fw[sq], or sv itself when fw is null; the largest, the smallest q on a
// tie (-0 and +0 are one key).  Every thread of the workgroup gets (key, q, slot); key 0: no finite end.  One __syncthreads.
template <typename R>
__device__ __forceinline__ void beam_best_end(Ctl<typename Key<R>::U> &ctl, const int *sq, const R *sv, int na, const R *fw,
                                              typename Key<R>::U &bkey, int &bqq, int &bk) {
    using KT = Key<R>;
    using U = typename KT::U;
    const int tid = threadIdx.x, lane = tid & 63;
    const R NINF = Num<R>::ninf();
    bkey = 0;
    bqq = 0x7FFFFFFF;
    bk = -1;
    for (int k = tid; k < na; k += kBT) {
        const int q = sq[k];
        const R s = fw ? sv[k] + fw[q] : sv[k];
        const U key = s > NINF ? KT::enc(s) : (U) 0;
        if (key && (key > bkey || (key == bkey && q < bqq))) { bkey = key; bqq = q; bk = k; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const U ok = (U) __shfl_xor(bkey, o);
        const int oq = __shfl_xor(bqq, o), okk = __shfl_xor(bk, o);
        if (ok > bkey || (ok == bkey && oq < bqq)) { bkey = ok; bqq = oq; bk = okk; }
    }
    if (lane == 0) { ctl.redv[tid >> 6] = bkey; ctl.redq[tid >> 6] = bqq; ctl.redk[tid >> 6] = bk; }
    __syncthreads();
    bkey = (U) ctl.redv[0]; bqq = ctl.redq[0]; bk = ctl.redk[0];
    for (int s = 1; s < kBT / 64; ++s) {
        const U ok = (U) ctl.redv[s];
        if (ok > bkey || (ok == bkey && ctl.redq[s] < bqq)) { bkey = ok; bqq = ctl.redq[s]; bk = ctl.redk[s]; }
    }
}

// No hypothesis: every integer output of the utterance -1, no tokens.  (The caller writes the score.)
__device__ __forceinline__ void beam_no_path(int T, long long *pb, long long *tk, long long *st, long long *tlen) {
    const int tid = threadIdx.x;
    for (int t = tid; t < T; t += kBT) { pb[t] = -1; tk[t] = -1; st[t] = -1; }
    if (tid == 0) *tlen = 0;
}

// The path that ends in slot bk of frame len-1, through the [.][K] lists bq / bs, into pb / st [T] (-1 behind len), and its
// tokens.  The whole workgroup calls it.
__device__ __forceinline__ void beam_backtrace(const int *bq, const int *bs, int K, int len, int T, int bk, const int *label,
                                               const int *state, long long *pb, long long *tk, long long *st, long long *tlen) {
    const int tid = threadIdx.x;
    for (int t = len + tid; t < T; t += kBT) { pb[t] = -1; st[t] = -1; }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        int k = bk;
        for (int t = len - 1; t >= 0; --t) {
            if (k < 0 || k >= K) break;                      // (cannot happen: every kept state stored its source's slot)
            const int q = bq[(int64_t) t * K + k];
            k = bs[(int64_t) t * K + k];
            pb[t] = label[q];
            st[t] = state[q];
        }
    }
    __threadfence();
    __syncthreads();
    if (tid < 64) collapse_tokens(pb, len, T, tk, tlen, tid);
}

}  // namespace

}  // namespace asg
