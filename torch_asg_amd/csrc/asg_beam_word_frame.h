// torch_asg_amd/csrc/asg_beam_word_frame.h -- ONE FRAME of the beam search over pairs (LM history h, lexicon product state q)
// and the END of that search, shared by the one-shot decoder (asg_beam_word.hip: beam_word_kernel walks all frames of an
// utterance in one launch) and the streaming decoder (asg_beam_word_stream.hip: beam_word_stream_advance_kernel enters the frame
// loop with the set an earlier call left, beam_word_stream_result_kernel is the end as a call of its own).  Both translation
// units compile this text, as asg_beam_graph.hip and asg_beam_stream.hip compile asg_beam_frame.h: that is what "decoding in
// chunks gives the bits of decoding in one call" rests on (include/asg_hip.h::asg_beam_word_stream_advance).  The frame is
// described at the top of asg_beam_word.hip.  Also here, for the two word streams (asg_beam_word_stream.hip,
// asg_beam_word_window.hip): bind_graph, the clearing loop of their resets (beam_word_reset_tables), the way their advance kernels
// enter and leave the frame loop (beam_word_load_set, beam_word_store_set), and collapse_words_from for the window's commits.
#pragma once
#include <type_traits>
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_frame.h"       // Ctl, find_digit, wave_append, collapse_tokens, dev_load / dev_store

namespace asg {

namespace {

constexpr int kWordSlotBits = 14;            // arg = source pair << 14 | source slot: K <= 8192 < 2^14, a pair < 2^50
constexpr int kMaxBackoff = 64;              // an LM walk of more backoff steps rejects (no loop without a bound)
constexpr size_t kWordCtlOff = 3072;         // WordCtl behind Ctl inside the fixed LDS
static_assert(sizeof(Ctl<unsigned long long>) <= kWordCtlOff, "control block");

struct WordCtl {
    unsigned long long ppre, pcut;           // tie select over pairs: the digits fixed so far, the largest pair taken
    unsigned long long rkey[kBT / 64], rpair[kBT / 64];
    int rk[kBT / 64];
};
static_assert(kWordCtlOff + sizeof(WordCtl) <= kFixedLds, "control block");

__device__ __forceinline__ int bits_of(int n) { return 32 - __clz(n > 1 ? n - 1 : 1); }   // >= 1

// LM look-ahead (asg_beam_word_la.hip, include/asg_hip.h::asg_beam_decode_words_la; the `_la` forms of the two word streams) is a
// compile-time flag of the frame and the end, off by default: every instantiation without it compiles the text it compiled
// before the flag existed.
template <typename R, bool LA>
struct WordLook {};
template <typename R>
struct WordLook<R, true> {
    const int *rlo, *rhi;        // [S] the ranks of the words below a trie node: [rlo, rhi)
    const int *la_state;         // [H] the history the look-ahead of h is taken from
    const int *krow, *krank;     // [H+1], [A'] the ranked arcs of each LM state, rank ascending
    const R *tab;                // [levels][A'] tab[k][i] = max of lw over the 2^k ranked arcs from i (inside the row of i)
    const R *dense0;             // [S] E(0, n): what the search in row 0, the longest, would find
    int A;                       // A'
};

template <typename R, bool LA = false>
struct BeamWordFrame {
    using U = typename Key<R>::U;
    Ctl<U> *ctl;
    WordCtl *wctl;
    R *cur_v;                    // LDS [K] values of the kept set
    int *cur_q, *cur_h;          // LDS [K] its pairs
    const R *trs;                // LDS [N][N] transitions (TRL)
    const R *tr;                 // ... or in global memory
    int64_t ts0, ts1;
    int N, K, G, cap, sep;
    int qbits, pbits;            // pair = h << qbits | q, pbits = hbits + qbits <= 50
    R theta;
    const int *label, *state, *orow, *start_q;
    int num_start;
    const int2 *oarc;
    const R *ow, *sw;
    // the word LM, weights folded
    const int *lrow, *lword, *lnext, *lback, *wos;
    const R *lw, *bw, *ew;
    int lstart;
    // the utterance's workspace
    unsigned long long *tkey;    // [C] the table's keys: pair + 1, 0 = empty
    unsigned long long *arg;     // [C]
    U *val;                      // [C]
    int tbits;                   // C = 1 << tbits
    U *ckey;                     // [cap]
    unsigned long long *cpair;   // [cap]
    int *tl;                     // [cap] the touched slots

    // The utterance's slot arrays inside its workspace `wb` (beam_word_work for T frames); -> the [T][K] lists.
    __device__ __forceinline__ void bind_work(char *wb, int T, int *&bq, int *&bh, int *&bs) {
        const BeamWordWork<char *> l = beam_word_work(wb, sizeof(U), T, K, cap, tbits);
        bq = (int *) l.bq;  bh = (int *) l.bh;  bs = (int *) l.bs;
        tkey = (unsigned long long *) l.tkey;  arg = (unsigned long long *) l.arg;  val = (U *) l.val;
        ckey = (U *) l.ckey;  cpair = (unsigned long long *) l.cpair;  tl = (int *) l.tl;
    }
    __device__ __forceinline__ unsigned long long pair(int h, int q) const {
        return ((unsigned long long) (unsigned) h << qbits) | (unsigned) q;
    }
    __device__ __forceinline__ unsigned home(unsigned long long key) const {
        return (unsigned) ((key * 0x9E3779B97F4A7C15ull) >> (64 - tbits));
    }
    // The slot of `key`, inserted if it is not there (`fresh`: by this lane); -1 if the table is full (it cannot be: C >= 2 * cap).
    __device__ __forceinline__ int insert(unsigned long long key, bool &fresh) const {
        const unsigned mask = (1u << tbits) - 1u;
        unsigned s = home(key);
        for (unsigned p = 0; p <= mask; ++p) {
            unsigned long long k = dev_load(tkey + s);
            if (k == 0) {
                k = atomicCAS(tkey + s, 0ull, key);
                if (k == 0) { fresh = true; return (int) s; }
            }
            if (k == key) return (int) s;
            s = (s + 1) & mask;
        }
        return -1;
    }
    __device__ __forceinline__ int find(unsigned long long key) const {
        const unsigned mask = (1u << tbits) - 1u;
        unsigned s = home(key);
        for (unsigned p = 0; p <= mask; ++p) {
            const unsigned long long k = dev_load(tkey + s);
            if (k == key) return (int) s;
            if (k == 0) return -1;
            s = (s + 1) & mask;
        }
        return -1;
    }
    // The LM walk: word w after state h -> (h2, a = 0 + bw per backoff step + lw of the arc), adds in walk order; false: rejected.
    __device__ __forceinline__ bool step(int h, int w, int &h2, R &a) const {
        a = (R) 0;
        if (w < 0) return false;
        for (int n = 0; n <= kMaxBackoff; ++n) {
            int lo = lrow[h];
            const int end = lrow[h + 1];
            int hi = end;
            while (lo < hi) {
                const int mid = (int) (((unsigned) lo + (unsigned) hi) >> 1);
                if (lword[mid] < w) lo = mid + 1; else hi = mid;
            }
            if (lo < end && lword[lo] == w) { a = a + lw[lo]; h2 = lnext[lo]; return true; }
            const int bo = lback[h];
            if (bo < 0) return false;
            a = a + bw[h];
            h = bo;
        }
        return false;
    }
    // L(h, n): the look-ahead of trie node n after history h -- 0 at the root; else, from s = la_state[h] down the backoff
    // chain, the largest (backoff sum so far) + E(s, n), E the range maximum of row s over the ranks of n: two binary searches
    // in krank and two reads of the table per level, one read of dense0 at state 0.  -inf: the LM accepts no word below n.
    __device__ R look(int h, int n) const {
        if (n == 0) return (R) 0;
        const int r0 = la.rlo[n], r1 = la.rhi[n];
        int s = la.la_state[h];
        R r = Num<R>::ninf(), a = (R) 0;
        for (int it = 0; it <= kMaxBackoff; ++it) {
            R e = Num<R>::ninf();
            if (s == 0) e = la.dense0[n];
            else {
                const int end = la.krow[s + 1];
                int lo = la.krow[s], hi = end;
                while (lo < hi) {
                    const int mid = (int) (((unsigned) lo + (unsigned) hi) >> 1);
                    if (la.krank[mid] < r0) lo = mid + 1; else hi = mid;
                }
                const int first = lo;
                hi = end;
                while (lo < hi) {
                    const int mid = (int) (((unsigned) lo + (unsigned) hi) >> 1);
                    if (la.krank[mid] < r1) lo = mid + 1; else hi = mid;
                }
                if (first < lo) {
                    const int k = 31 - __clz(lo - first);
                    const R *row = la.tab + (int64_t) k * la.A;
                    const R x = row[first], y = row[lo - (1 << k)];
                    e = x > y ? x : y;
                }
            }
            const R c = a + e;
            r = c > r ? c : r;
            const int bo = lback[s];
            if (bo < 0) break;
            a = a + bw[s];
            s = bo;
        }
        return r;
    }
    WordLook<R, LA> la;
};

// What a kernel with the look-ahead flag takes beside the LM: the look-ahead's arrays with it, nothing without.
struct WordNoLook {};
template <bool LA>
using WordLookParam = std::conditional_t<LA, WordLookArgs, WordNoLook>;
template <typename R>
__device__ __forceinline__ void bind_look(BeamWordFrame<R, true> &f, const WordLookArgs &la) {
    f.la.rlo = la.rlo; f.la.rhi = la.rhi; f.la.la_state = la.la_state; f.la.krow = la.krow; f.la.krank = la.krank;
    f.la.tab = (const R *) la.tab; f.la.dense0 = (const R *) la.dense0; f.la.A = la.A;
}
template <typename R>
__device__ __forceinline__ void bind_look(BeamWordFrame<R, false> &, const WordNoLook &) {}

// The parts of a BeamWordFrame that do not depend on the call: the graph, the LM and the shape of the search.
template <typename R, bool LA>
__device__ __forceinline__ void bind_graph(BeamWordFrame<R, LA> &f, const GraphArgs &g, const BeamGraphArgs &bg, const WordLmArgs &lm,
                                           int K, int cap, int tbits) {
    f.K = K; f.G = beam_lanes_per_state(K); f.cap = cap; f.sep = lm.sep; f.tbits = tbits;
    f.qbits = bits_of(g.Q); f.pbits = f.qbits + bits_of(lm.H);
    f.label = g.label; f.state = g.state; f.orow = bg.orow; f.start_q = bg.start_q; f.num_start = bg.num_start;
    f.oarc = (const int2 *) bg.oarc; f.ow = (const R *) bg.ow; f.sw = (const R *) g.start_w;
    f.lrow = lm.row; f.lword = lm.word; f.lnext = lm.next; f.lback = lm.backoff; f.wos = lm.word_of_state;
    f.lw = (const R *) lm.lw; f.bw = (const R *) lm.bw; f.ew = (const R *) lm.ew; f.lstart = lm.start;
}

// A word stream's reset (asg_beam_word_stream.hip, asg_beam_word_window.hip): the whole table of the slot whose workspace is
// `wb` emptied -- tkey = 0, val = 0, arg = none for all C slots -- by the workgroups of 256 threads that blockIdx.y counts.
__device__ __forceinline__ void beam_word_reset_tables(char *wb, const BeamWordWorkLayout &l, unsigned C, int key_bytes) {
    unsigned long long *tkey = (unsigned long long *) (wb + l.tkey), *arg = (unsigned long long *) (wb + l.arg);
    for (unsigned s = blockIdx.y * 256 + threadIdx.x; s < C; s += gridDim.y * 256) {
        dev_store(tkey + s, 0ull);
        dev_store(arg + s, ~0ull);
        if (key_bytes == 8) dev_store((unsigned long long *) (wb + l.val) + s, 0ull);
        else dev_store((unsigned int *) (wb + l.val) + s, 0u);
    }
}

// One frame: from the kept set (f.cur_h, f.cur_q, f.cur_v)[0..na) of the frame before -- or, with `first`, from the start states
// -- to the new one, with (q, h, source slot) of every kept pair into row `row` of the [.][K] lists bq / bh / bs.  `xt` are the
// frame's emissions (stride is2).  The whole workgroup calls it; it begins after and ends with a __syncthreads.  The table is
// empty again on return (a first frame does not use it), f.ctl->na holds the new count and f.ctl->n is 0.
template <typename R, bool TRL, bool LA = false>
__device__ __forceinline__ void beam_word_frame(const BeamWordFrame<R, LA> &f, bool first, int na, const R *xt, int64_t is2, int *bq,
                                                int *bh, int *bs, int row) {
    using KT = Key<R>;
    using U = typename KT::U;
    Ctl<U> &ctl = *f.ctl;
    WordCtl &wctl = *f.wctl;
    const int tid = threadIdx.x, lane = tid & 63;
    const int K = f.K, G = f.G, N = f.N, cap = f.cap;
    (void) N;
    const R NINF = Num<R>::ninf();
    const R theta = f.theta;
    R *cur_v = f.cur_v;
    int *cur_q = f.cur_q, *cur_h = f.cur_h;
    unsigned long long *arg = f.arg, *tkey = f.tkey, *cpair = f.cpair;
    U *val = f.val, *ckey = f.ckey;
    int *tl = f.tl;
    const int2 *oarc = f.oarc;
    const R *ow = f.ow, *sw = f.sw;
    const unsigned long long qmask = (1ull << f.qbits) - 1ull;
    auto TR = [&](int i, int j) -> R {
        if constexpr (TRL) return f.trs[i * N + j];
        else return f.tr[(int64_t) i * f.ts0 + (int64_t) j * f.ts1];
    };
    const unsigned long long ARG_NONE = ~0ull;

    // ================================================================ candidates
    if (first) {
        if (tid == 0) ctl.n = f.num_start;
    } else {
        for (int phase = 0; phase < 2; ++phase) {
            for (int k0 = 0; k0 < na; k0 += kBT / G) {
                const int k = k0 + tid / G, lg = tid % G;
                const bool act = k < na;
                int qs = 0, hs = 0, j = 0, e = 0, e1 = 0;
                R v = NINF;
                [[maybe_unused]] R ls = (R) 0;                        // L(hs, state(qs)): one value for all edges of the pair
                if (act) {
                    qs = cur_q[k]; hs = cur_h[k]; v = cur_v[k]; j = f.label[qs];
                    e = f.orow[qs] + lg; e1 = f.orow[qs + 1];
                    if constexpr (LA) ls = f.look(hs, f.state[qs]);
                }
                const unsigned long long me = (f.pair(hs, qs) << kWordSlotBits) | (unsigned) k;
                // the stay, then the row; the whole wavefront stays in the loop until its last lane is done (wave_append)
                bool stay = act && lg == 0;
                while (__any(stay || e < e1)) {
                    int tq = -1, th = hs;
                    R c = NINF;
                    if (stay) { tq = qs; c = v + TR(j, j); stay = false; }
                    else if (e < e1) {
                        const int2 a = oarc[e];
                        tq = a.x;
                        c = (v + TR(a.y, j)) + ow[e];
                        if (a.y == f.sep) {                           // a word ends: the LM moves
                            R add;
                            int h2;
                            if (f.step(hs, f.wos[f.state[qs]], h2, add)) {
                                th = h2;
                                if constexpr (LA) c = c + (add - ls); else c = c + add;
                            } else tq = -1;
                        } else if constexpr (LA) {                    // into a node: its look-ahead for the source's
                            const R lt = f.look(hs, f.state[tq]);
                            if (lt > NINF) c = c + (lt - ls); else tq = -1;       // a dead end is pruned here
                        }
                        e += G;
                    }
                    const bool ok = tq >= 0 && c > NINF;          // a -inf candidate never makes a candidate pair
                    const U key = KT::enc(c);
                    const unsigned long long pk = f.pair(th, tq) + 1ull;
                    if (phase == 0) {
                        bool fresh = false;
                        if (ok) {
                            const int s = f.insert(pk, fresh);
                            if (s >= 0) atomicMax(val + s, key);
                            if (fresh) th = s;                    // (th is done with: it carries the slot to the append)
                        }
                        const int pos = wave_append(fresh, &ctl.n);
                        if (fresh && pos < cap) tl[pos] = th;
                    } else if (ok) {
                        const int s = f.find(pk);
                        if (s >= 0 && dev_load(val + s) == key) atomicMin(arg + s, me);
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid < 256) { ctl.hist[0][tid] = 0; ctl.hist[1][tid] = 0; }
    if (tid == 0) { ctl.kmax = 0; ctl.kmin = ~(U) 0; ctl.na = 0; ctl.done = 0; wctl.pcut = ~0ull; }
    __syncthreads();
    // ================================================================ select (the value part is asg_beam_frame.h's, verbatim)
    const int n = ctl.n < cap ? ctl.n : cap;
    {   // c = best + emission as keys, the pairs beside them; their maximum and minimum
        U mx = 0, mn = ~(U) 0;
        for (int j = tid; j < n; j += kBT) {
            unsigned long long p;
            R base;
            if (first) {
                const int q = f.start_q[j];
                p = f.pair(f.lstart, q);
                base = sw[q];
                if constexpr (LA) base = base + f.look(f.lstart, f.state[q]);
            }
            else { const int s = tl[j]; p = dev_load(tkey + s) - 1ull; base = KT::dec(dev_load(val + s)); }
            const R c = base + xt[(int64_t) f.label[(int) (p & qmask)] * is2];
            const U key = c > NINF ? KT::enc(c) : (U) 0;
            ckey[j] = key;
            cpair[j] = p;
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
        // ---- ties at the K-th key: the `need` smallest pairs among them, over the pair's pbits bits
        if (!ctl.done) {
            const U kth = ctl.kth;
            if (tid < 256) { ctl.hist[0][tid] = 0; ctl.hist[1][tid] = 0; }
            if (tid == 0) wctl.ppre = 0;
            __syncthreads();
            int prem = f.pbits;
            hb = 0;
            while (prem > 0) {
                const int w = prem < 8 ? prem : 8, shift = prem - w;
                const unsigned long long pre = wctl.ppre;
                int *h = ctl.hist[hb];
                for (int j = tid; j < n; j += kBT) {
                    if (ckey[j] != kth) continue;
                    const unsigned long long p = cpair[j];
                    if ((p >> prem) == pre) atomicAdd(&h[(int) ((p >> shift) & ((1ull << w) - 1ull))], 1);
                }
                if (tid < 256) ctl.hist[hb ^ 1][tid] = 0;
                __syncthreads();
                if (tid < 64) {
                    int d, before;
                    find_digit<false>(h, ctl.need, lane, d, before);
                    if (lane == 0) {
                        ctl.need -= before;
                        wctl.ppre = (pre << w) | (unsigned long long) d;
                        if (shift == 0) wctl.pcut = wctl.ppre;
                    }
                }
                __syncthreads();
                prem = shift;
                hb ^= 1;
            }
        }
    }
    // ---- the new kept set, the frame's back-pointers, and the table emptied
    {
        const U kth = ctl.kth;
        const unsigned long long pcut = wctl.pcut;
        int *bqt = bq + (int64_t) row * K, *bht = bh + (int64_t) row * K, *bst = bs + (int64_t) row * K;
        for (int j0 = 0; j0 < n; j0 += kBT) {
            const int j = j0 + tid;
            bool sel = false;
            unsigned long long p = 0;
            U key = 0;
            int s = 0;
            if (j < n) {
                p = cpair[j];
                key = ckey[j];
                if (!first) s = tl[j];
                sel = kmax != 0 && key != 0 && key >= lokey && (key > kth || (key == kth && p <= pcut));
            }
            const int slot = wave_append(sel, &ctl.na);
            if (sel && slot < K) {                       // (never more than K: the select counted them)
                const int q = (int) (p & qmask), h = (int) (p >> f.qbits);
                cur_q[slot] = q;
                cur_h[slot] = h;
                cur_v[slot] = KT::dec(key);
                bqt[slot] = q;
                bht[slot] = h;
                bst[slot] = first ? -1 : (int) (dev_load(arg + s) & ((1ull << kWordSlotBits) - 1ull));
            }
            if (j < n && !first) { dev_store(tkey + s, 0ull); dev_store(val + s, (U) 0); dev_store(arg + s, ARG_NONE); }
        }
    }
    if (tid == 0) ctl.n = 0;
    __syncthreads();
}

// A word stream's advance (asg_beam_word_stream.hip, asg_beam_word_window.hip) enters the frame loop with the set an earlier call
// left at `set_v` -- values [K], then product states int32 [K], then LM states int32 [K]: the transitions into LDS when they live
// there, the na0 stored pairs into f.cur_v / f.cur_q / f.cur_h, the counters.  The whole workgroup calls it; it ends with a
// __syncthreads.
template <typename R, bool TRL, bool LA>
__device__ __forceinline__ void beam_word_load_set(const BeamWordFrame<R, LA> &f, R *trs, const R *set_v, int na0) {
    const int tid = threadIdx.x, N = f.N;
    const int *set_q = (const int *) (set_v + f.K), *set_h = set_q + f.K;
    if constexpr (TRL)
        for (int x = tid; x < N * N; x += kBT) trs[x] = f.tr[(int64_t) (x / N) * f.ts0 + (int64_t) (x % N) * f.ts1];
    for (int k = tid; k < na0; k += kBT) { f.cur_v[k] = set_v[k]; f.cur_q[k] = set_q[k]; f.cur_h[k] = set_h[k]; }
    if (tid == 0) { f.ctl->na = na0; f.ctl->n = 0; }
    __syncthreads();
}
// ... and leaves it: the set back to `set_v`; -> its size, for the header.
template <typename R, bool LA>
__device__ __forceinline__ int beam_word_store_set(const BeamWordFrame<R, LA> &f, R *set_v) {
    int *set_q = (int *) (set_v + f.K), *set_h = set_q + f.K;
    int na = f.ctl->na;
    na = na < f.K ? na : f.K;
    for (int k = threadIdx.x; k < na; k += kBT) { set_v[k] = f.cur_v[k]; set_q[k] = f.cur_q[k]; set_h[k] = f.cur_h[k]; }
    return na;
}

// The end of a kept pair (h, q) with value v: (v + final_w[q]) + endw, endw = ew[h] at the root, a + ew[h'] after the LM walk of
// the word that ends in q's node; false: no end (mid-word, or the walk rejects).  `w`: that word, or -1.
template <typename R, bool LA = false>
__device__ __forceinline__ bool word_end(const BeamWordFrame<R, LA> &f, const R *fw, int h, int q, R v, R &e, int &w) {
    const int s = f.state[q];
    R endw;
    w = -1;
    if (s == 0) endw = f.ew[h];
    else {
        const int ww = f.wos[s];
        int h2;
        R a;
        if (!f.step(h, ww, h2, a)) return false;
        if constexpr (LA) endw = (a - f.look(h, s)) + f.ew[h2]; else endw = a + f.ew[h2];
        w = ww;
    }
    e = (v + fw[q]) + endw;
    return true;
}

__device__ __forceinline__ void word_no_path(int T, long long *pb, long long *tk, long long *st, long long *lm, long long *wd,
                                             long long *tlen, long long *wlen) {
    const int tid = threadIdx.x;
    for (int t = tid; t < T; t += kBT) { pb[t] = -1; tk[t] = -1; st[t] = -1; lm[t] = -1; wd[t] = -1; }
    if (tid == 0) { *tlen = 0; *wlen = 0; }
}

// One wavefront: the words of a SEGMENT of a path that continues an earlier one (asg_beam_word_window.hip).  pb / st [0..len)
// are the labels and automaton states behind a frame whose label was `carry` and whose state was `carry_state` (-1: there is no
// such frame).  A word ends where the separator stands behind another label: it is the word of the state before.  They go to
// wd[0..), nothing is padded.  -> the number appended; every lane gets it.
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

// The value of a kept pair (h, q) as a PREFIX score: the value itself -- with look-ahead, the value without the estimate
// L(h, state(q)) it still carries (0 at the root, finite for every kept pair).
template <typename R, bool LA>
__device__ __forceinline__ R word_prefix(const BeamWordFrame<R, LA> &f, int h, int q, R v) {
    if constexpr (LA) return v - f.look(h, f.state[q]);
    else return v;
}

// The best end over a set (sh, sq, sv)[0..na), the smallest pair on a tie (-0 and +0 are one key): with `final` the end of
// word_end, without it word_prefix -- the best PREFIX, which may end mid-word.  Every thread of the workgroup gets (key,
// slot); key 0: no finite end.  One __syncthreads; f.wctl holds the reduction slots.
template <typename R, bool LA = false>
__device__ __forceinline__ void word_best_end(const BeamWordFrame<R, LA> &f, const R *fw, bool final, const int *sh, const int *sq,
                                              const R *sv, int na, typename Key<R>::U &bkey, int &bk) {
    using KT = Key<R>;
    using U = typename KT::U;
    WordCtl &wctl = *f.wctl;
    const int tid = threadIdx.x, lane = tid & 63;
    const R NINF = Num<R>::ninf();
    bkey = 0;
    unsigned long long bpair = ~0ull;
    bk = -1;
    for (int k = tid; k < na; k += kBT) {
        R e;
        int w;
        if (!final) e = word_prefix<R, LA>(f, sh[k], sq[k], sv[k]);
        else if (!word_end<R, LA>(f, fw, sh[k], sq[k], sv[k], e, w)) continue;
        const U key = e > NINF ? KT::enc(e) : (U) 0;
        const unsigned long long p = f.pair(sh[k], sq[k]);
        if (key && (key > bkey || (key == bkey && p < bpair))) { bkey = key; bpair = p; bk = k; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const U ok = (U) __shfl_xor(bkey, o);
        const unsigned long long op = __shfl_xor(bpair, o);
        const int okk = __shfl_xor(bk, o);
        if (ok > bkey || (ok == bkey && op < bpair)) { bkey = ok; bpair = op; bk = okk; }
    }
    if (lane == 0) { wctl.rkey[tid >> 6] = bkey; wctl.rpair[tid >> 6] = bpair; wctl.rk[tid >> 6] = bk; }
    __syncthreads();
    bkey = (U) wctl.rkey[0]; bpair = wctl.rpair[0]; bk = wctl.rk[0];
    for (int s = 1; s < kBT / 64; ++s) {
        const U ok = (U) wctl.rkey[s];
        if (ok > bkey || (ok == bkey && wctl.rpair[s] < bpair)) { bkey = ok; bpair = wctl.rpair[s]; bk = wctl.rk[s]; }
    }
}

// The path that ends in slot bk of frame len-1, through the [.][K] lists bq / bh / bs, into pb / st / ls [T] (-1 behind len);
// the score from the winner's own sum (the key folds -0 into +0); the words of its separator edges and, with `final`, the word
// of the last step; the tokens; -1 behind everything.  The whole workgroup calls it, after word_best_end.
template <typename R, bool LA = false>
__device__ __forceinline__ void word_backtrace(const BeamWordFrame<R, LA> &f, const R *fw, bool final, const int *sh, const int *sq,
                                               const R *sv, int bk, const int *bq, const int *bh, const int *bs, int len, int T,
                                               R *score, long long *pb, long long *tk, long long *st, long long *ls,
                                               long long *wd, long long *tlen, long long *wlen) {
    WordCtl &wctl = *f.wctl;
    const int tid = threadIdx.x, K = f.K;
    for (int t = len + tid; t < T; t += kBT) { pb[t] = -1; st[t] = -1; ls[t] = -1; }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        R e = sv[bk];
        int wfin = -1;
        if (final) (void) word_end<R, LA>(f, fw, sh[bk], sq[bk], sv[bk], e, wfin);
        else e = word_prefix<R, LA>(f, sh[bk], sq[bk], sv[bk]);
        *score = e;
        int k = bk;
        for (int t = len - 1; t >= 0; --t) {
            if (k < 0 || k >= K) break;                      // (cannot happen: every kept pair stored its source's slot)
            const int q = bq[(int64_t) t * K + k];
            ls[t] = bh[(int64_t) t * K + k];
            k = bs[(int64_t) t * K + k];
            pb[t] = f.label[q];
            st[t] = f.state[q];
        }
        // a separator edge is the one way into the separator's product state: its frames are those whose label is the separator
        // behind another label, and the word is the one that ends in the node before
        int nw = 0;
        for (int t = 1; t < len; ++t)
            if (pb[t] == f.sep && pb[t - 1] != f.sep) wd[nw++] = f.wos[st[t - 1]];
        if (wfin >= 0) wd[nw++] = wfin;
        *wlen = nw;
        wctl.rk[0] = nw;
    }
    __threadfence();
    __syncthreads();
    for (int t = wctl.rk[0] + tid; t < T; t += kBT) wd[t] = -1;
    if (tid < 64) collapse_tokens(pb, len, T, tk, tlen, tid);
}

// The table of a frame has C slots, the power of two >= 2 * cap.
inline int word_table_bits(int cap) {
    int bits = 1;
    while (((size_t) 1 << bits) < 2 * (size_t) cap) ++bits;
    return bits;
}

}  // namespace

}  // namespace asg
