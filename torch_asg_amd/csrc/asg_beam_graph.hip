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
__device__ void collapse_tokens(const long long *pb, int len, int T, long long *tk, long long *tl, int lane) {
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
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
    const int Q = g.Q, N = P.N, T = P.T;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *tr = (const R *) P.transition;
    const R *sw = (const R *) g.start_w, *fw = (const R *) g.final_w, *ow = (const R *) bg.ow;
    const int2 *oarc = (const int2 *) bg.oarc;
    long long *pb = path + (int64_t) b * T, *tk = tokens + (int64_t) b * T, *st = states + (int64_t) b * T;
    // the utterance's workspace (beam_graph_layout)
    char *wb = work + (size_t) b * per_utt;
    const size_t a256 = 255;
    size_t off = 0;
    int *bq = (int *) (wb + off);  off += ((size_t) T * K * 4 + a256) & ~a256;       // [T][K] product state of each slot
    int *bs = (int *) (wb + off);  off += ((size_t) T * K * 4 + a256) & ~a256;       // [T][K] its source's slot at t-1
    unsigned long long *arg = (unsigned long long *) (wb + off);  off += ((size_t) Q * 8 + a256) & ~a256;
    U *val = (U *) (wb + off);     off += ((size_t) Q * sizeof(U) + a256) & ~a256;
    U *ckey = (U *) (wb + off);    off += ((size_t) cap * sizeof(U) + a256) & ~a256;
    int *tl = (int *) (wb + off);
    // cnt_off != 0 (asg_beam_loss.hip): |A_t| of every frame goes to int32 [T] at that offset of the utterance's workspace
    int *cnt = cnt_off ? (int *) (wb + cnt_off) : nullptr;
    if (cnt) for (int t = tid; t < T; t += kBT) cnt[t] = 0;
    // fin_off != 0 (asg_beam_nbest.hip): |A_{len-1}| goes to the int32 at that offset and the values of that set, slot-aligned
    // with bq[len-1], behind it from byte 8 on
    int *fin_n = fin_off ? (int *) (wb + fin_off) : nullptr;
    auto TR = [&](int i, int j) -> R {
        if constexpr (TRL) return trs[i * N + j];
        else return tr[(int64_t) i * P.ts0 + (int64_t) j * P.ts1];
    };
    const unsigned long long ARG_NONE = ~0ull;

    if (len < 1) {
        for (int t = tid; t < T; t += kBT) { pb[t] = -1; tk[t] = -1; st[t] = -1; }
        if (tid == 0) { scores[b] = NINF; tlen[b] = 0; if (fin_n) *fin_n = 0; }
        return;
    }
    if constexpr (TRL)
        for (int x = tid; x < N * N; x += kBT) trs[x] = tr[(int64_t) (x / N) * P.ts0 + (int64_t) (x % N) * P.ts1];
    if (len >= 2)
        for (int q = tid; q < Q; q += kBT) { dev_store(val + q, (U) 0); dev_store(arg + q, ARG_NONE); }
    if (tid == 0) { ctl.na = 0; ctl.n = 0; }
    __syncthreads();

    // subgroup of G lanes per active state: wide when the beam is narrow
    int G = 1;
    while (G < 64 && G * 2 * K <= kBT) G *= 2;

    for (int t = 0; t < len; ++t) {
        const R *xt = in + (int64_t) t * P.is0;
        const int na = ctl.na;
        if (t >= 1 && na == 0) break;                       // an empty beam stays empty
        // ================================================================ candidates
        if (t == 0) {
            const int ns = bg.num_start;
            for (int j = tid; j < ns; j += kBT) tl[j] = bg.start_q[j];
            if (tid == 0) ctl.n = ns;
        } else {
            for (int phase = 0; phase < 2; ++phase) {
                for (int k0 = 0; k0 < na; k0 += kBT / G) {
                    const int k = k0 + tid / G, lg = tid % G;
                    const bool act = k < na;
                    int qs = 0, j = 0, e = 0, e1 = 0;
                    R v = NINF;
                    if (act) {
                        qs = cur_q[k]; v = cur_v[k]; j = g.label[qs];
                        e = bg.orow[qs] + lg; e1 = bg.orow[qs + 1];
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
                const R base = t == 0 ? sw[q] : KT::dec(dev_load(val + q));
                const R c = base + xt[(int64_t) g.label[q] * P.is2];
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
            bool first = true;
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
                first = false;
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
                    if (first) {                              // everything that passes lo: taken whole when it fits
                        for (int x = 0; x < 4; ++x) total += h[4 * lane + x];
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) total += __shfl_xor(total, o);
                    }
                    if (first && total <= K) {
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
                first = false;
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
            int *bqt = bq + (int64_t) t * K, *bst = bs + (int64_t) t * K;
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
                    bst[slot] = t == 0 ? -1 : (int) (dev_load(arg + q) & ((1ull << kSlotBits) - 1ull));
                }
                if (j < n && t >= 1) { dev_store(val + q, (U) 0); dev_store(arg + q, ARG_NONE); }
            }
        }
        if (tid == 0) ctl.n = 0;
        __syncthreads();
        if (cnt && tid == 0) cnt[t] = ctl.na < K ? ctl.na : K;
    }

    // ---- score: the largest v + final_w over the last active set, the smallest q on a tie
    const int na = ctl.na;
    if (fin_n) {
        R *fin_v = (R *) (wb + fin_off + 8);
        for (int k = tid; k < na && k < K; k += kBT) fin_v[k] = cur_v[k];
        if (tid == 0) *fin_n = na < K ? na : K;
    }
    U bkey = 0;
    int bqq = 0x7FFFFFFF, bk = -1;
    for (int k = tid; k < na; k += kBT) {
        const int q = cur_q[k];
        const R s = cur_v[k] + fw[q];
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
    if (bkey == 0) {                                        // an empty beam, or no active state with a finite final weight
        for (int t = tid; t < T; t += kBT) { pb[t] = -1; tk[t] = -1; st[t] = -1; }
        if (tid == 0) { scores[b] = NINF; tlen[b] = 0; }
        return;
    }
    // the score itself, from the winner's own sum (the key folds -0 into +0)
    if (tid == 0) scores[b] = cur_v[bk] + fw[bqq];
    for (int t = len + tid; t < T; t += kBT) { pb[t] = -1; st[t] = -1; }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        int k = bk;
        for (int t = len - 1; t >= 0; --t) {
            if (k < 0 || k >= K) break;                      // (cannot happen: every kept state stored its source's slot)
            const int q = bq[(int64_t) t * K + k];
            k = bs[(int64_t) t * K + k];
            pb[t] = g.label[q];
            st[t] = g.state[q];
        }
    }
    __threadfence();
    __syncthreads();
    if (tid < 64) collapse_tokens(pb, len, T, tk, tlen + b, tid);
}

inline size_t a256(size_t x) { return (x + 255) / 256 * 256; }

inline size_t beam_per_utt(int elem, int T, int Q, int K, int cap) {
    return 2 * a256((size_t) T * K * 4) + a256((size_t) Q * 8) + a256((size_t) Q * elem) + a256((size_t) cap * elem) +
           a256((size_t) cap * 4);
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
    return (size_t) B * beam_per_utt(elem, T, Q, K, cap);
}

template <typename R>
hipError_t launch_beam_graph(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta, void *work,
                             void *scores, long long *path, long long *tokens, long long *tlen, long long *states,
                             hipStream_t stream, size_t stride, size_t cnt_off, size_t fin_off) {
    const int N = P.N;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const size_t per = stride ? stride : beam_per_utt(sizeof(R), P.T, G.Q, K, cap);
    const size_t beam = kFixedLds + (size_t) K * (sizeof(R) + 4) + 8;
    const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
    const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
    static_assert(sizeof(Ctl<unsigned long long>) <= kFixedLds, "control block");
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
