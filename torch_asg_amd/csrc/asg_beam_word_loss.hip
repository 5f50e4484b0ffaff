// torch_asg_amd/csrc/asg_beam_word_loss.hip -- the BEAM-PRUNED normaliser of an ASG criterion composed with a LEXICON and a WORD
// n-gram LM, on gfx950: asg_beam_loss.hip's log-semiring pass over the PAIRS (LM history h, lexicon product state q) that the
// search of asg_beam_word.hip keeps, plus the pairs every alignment of the target runs through, and its gradients.  The
// specification is include/asg_hip.h::asg_beam_words_full_forward; tests/beam_word_loss_ref.py restates it in numpy.
//
// Forward, four launches on one stream:
//   1  beam_word_loss_search: the frame of asg_beam_word_frame.h in a loop of its own (the same device text as beam_word_kernel,
//      so the same kept sets bit for bit) that leaves |A_t| of every frame beside the [T][K] lists bq / bh; no end, no backtrace;
//   2  beam_word_loss_targets: one thread per utterance walks the lexicon's outgoing rows along the merged target, the LM walk
//      on every separator edge included -> the forced pairs as 64-bit keys h << qbits | q; hdr[0] = n (0: nothing is forced);
//   3  beam_word_loss_sets: one workgroup per (utterance, frame) -- utterances in x, frames strided over y -- sorts the keys of A_t
//      with those of F_t in LDS (bitonic over the power of two its own count needs), blanks the duplicates and sorts again:
//      U[t][0 .. nu[t]) ascending in pair order;
//   4  beam_word_loss_fwd: one 1024-thread workgroup per utterance walks the frames.  There is no incoming-edge list over pairs
//      (the histories that reach (h', q') through a word cannot be listed without inverting the LM), so alpha PUSHES: U_t lies in
//      LDS, G lanes per pair of U_{t-1} stride over the outgoing row of its q (lane 0 adds the stay, a separator edge walks the
//      LM), find the target in U_t by binary search and -- pass 1 -- raise its maximum with an integer atomicMax on the
//      order-preserving key, -- pass 2 -- add exp(c - max) to its sum as a 64-bit fixed-point integer with 48 fractional bits (a
//      target has at most |U_{t-1}| + 1 < 2^14 candidates of at most 1 each: no overflow).  Integer max and add are associative:
//      the order the lanes arrive in cannot change a bit.  alpha = (max + log(sum)) + emission goes to the workspace ([T][M] when
//      a gradient is wanted, else two rows).
// Backward, two launches: beam_word_loss_bwd (beta PULLS: a pair's own outgoing row is a gather against U_{t+1} in LDS, no
// atomics on values; it owns the label posteriors and the (i, j) counts, summed as 64-bit fixed-point integers as in
// asg_beam_loss.hip, the counts in LDS while the [N][N] tile fits, else in the utterance's scratch) and
// beam_word_loss_tr_reduce (the utterances in ascending order).  NO FLOAT ATOMICS anywhere.  Every output, padding row and
// scratch word that is read is written by these kernels: no memset, so both directions can be captured and replayed.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"  // the frame of the search, the LM walk and the end of a pair

namespace asg {

namespace {

constexpr int kWL = 1024;                       // forward / backward workgroup
constexpr int kWS = 256;                        // set / reduction workgroups
constexpr size_t kWLHead = 256;                 // reduction slots in front of the dynamic LDS
constexpr size_t kWLLds = 160 * 1024;
constexpr double kWGammaScale = 4611686018427387904.0;       // 2^62
constexpr double kWSumScale = 281474976710656.0;              // 2^48: a target's sum of exp(c - max) over < 2^14 candidates

template <typename R> __device__ __forceinline__ R wexp(R x);
template <> __device__ __forceinline__ float wexp<float>(float x) { return expf(x); }
template <> __device__ __forceinline__ double wexp<double>(double x) { return ::exp(x); }
template <typename R> __device__ __forceinline__ R wlog(R x);
template <> __device__ __forceinline__ float wlog<float>(float x) { return logf(x); }
template <> __device__ __forceinline__ double wlog<double>(double x) { return ::log(x); }
template <typename R> __device__ __forceinline__ R wmax(R a, R b) { return b > a ? b : a; }

__device__ __forceinline__ unsigned long long w_fixed(double p, double scale) {
    return p > 0.0 ? (unsigned long long) (p * scale) : 0ull;
}

// position of pair p in the ascending list a[0 .. n), -1 if absent
__device__ __forceinline__ int find_pair(const unsigned long long *a, int n, unsigned long long p) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < p) lo = mid + 1; else hi = mid;
    }
    return (lo < n && a[lo] == p) ? lo : -1;
}

template <typename R> __device__ __forceinline__ R wgroup_max(R v, int G) {
    for (int o = 1; o < G; o <<= 1) v = wmax(v, (R) __shfl_xor(v, o));
    return v;
}
template <typename R> __device__ __forceinline__ R wgroup_sum(R v, int G) {
    for (int o = 1; o < G; o <<= 1) v += (R) __shfl_xor(v, o);
    return v;
}
template <typename R>
__device__ R wwg_max(R v, R *red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wgroup_max(v, 64);
    if (lane == 0) red[w] = v;
    __syncthreads();
    v = red[0];
    for (int s = 1; s < kWL / 64; ++s) v = wmax(v, red[s]);
    __syncthreads();
    return v;
}
template <typename R>
__device__ R wwg_sum(R v, R *red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wgroup_sum(v, 64);
    if (lane == 0) red[w] = v;
    __syncthreads();
    v = red[0];
    for (int s = 1; s < kWL / 64; ++s) v += red[s];
    __syncthreads();
    return v;
}

// lanes per source pair: the largest power of two <= 64 with G * m <= 1024
__device__ __forceinline__ int wsubgroup(int m) {
    int G = 1;
    while (G < 64 && G * 2 * m <= kWL) G *= 2;
    return G;
}

// The read-only part of a BeamWordFrame for the kernels that only walk the graph and the LM.
template <typename R>
__device__ __forceinline__ void bind_walk(BeamWordFrame<R> &f, const GraphArgs &g, const BeamGraphArgs &bg, const WordLmArgs &lm) {
    bind_graph<R, false>(f, g, bg, lm, 1, 1, 1);
}

// ---------------------------------------------------------------------------------------------------------------------
// 1: the search.  beam_word_kernel's frame loop; cnt[t] = |A_t| for t < len.
// ---------------------------------------------------------------------------------------------------------------------
template <typename R, bool TRL>
__global__ void __launch_bounds__(kBT) beam_word_loss_search(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, int K, R theta,
                                                             int cap, int tbits, char *work, size_t per_utt, size_t cnt_off) {
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
    const int len = clamp_len(P.in_len, b, T);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *tr = (const R *) P.transition;
    BeamWordFrame<R> f;
    f.ctl = &ctl; f.wctl = &wctl; f.cur_v = cur_v; f.cur_q = cur_q; f.cur_h = cur_h; f.trs = trs; f.tr = tr;
    f.ts0 = P.ts0; f.ts1 = P.ts1; f.N = N; f.theta = theta;
    bind_graph<R, false>(f, g, bg, lm, K, cap, tbits);
    int *bq, *bh, *bs;
    char *wb = work + (size_t) b * per_utt;
    f.bind_work(wb, T, bq, bh, bs);
    int *cnt = (int *) (wb + cnt_off);
    if (len < 1) return;
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
        beam_word_frame<R, TRL>(f, t == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bh, bs, t);
        if (tid == 0) cnt[t] = ctl.na < K ? ctl.na : K;
    }
    for (int u = t + tid; u < len; u += kBT) cnt[u] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// 2: the walk of the merged target through the lexicon and the LM.  -> n pairs into key[0 .. n) (when key is not null) and the
// lexicon + LM score of the target, end terms included; n = 0 and -inf when a label lies outside [0, N), an arc is missing, an
// LM step is rejected, the path ends mid-word or its end is -inf.  One thread.
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__device__ int walk_target(const BeamWordFrame<R> &f, const R *fw, const Problem &P, int b, int tl, int max_n,
                           unsigned long long *key, R &score) {
    const R NINF = Num<R>::ninf();
    score = NINF;
    int n = 0, q = -1, h = f.lstart;
    long long prev = -1;
    R s = (R) 0;
    for (int k = 0; k < tl; ++k) {
        const long long y = P.targets[(int64_t) b * P.gs0 + (int64_t) k * P.gs1];
        if (y == prev) continue;
        if (y < 0 || y >= P.N) return 0;
        int q2 = -1;
        if (q < 0) {
            for (int j = 0; j < f.num_start; ++j)
                if (f.label[f.start_q[j]] == (int) y) { q2 = f.start_q[j]; break; }
            if (q2 < 0) return 0;
            s = f.sw[q2];
        } else {
            int e = f.orow[q];
            const int e1 = f.orow[q + 1];
            for (; e < e1; ++e)
                if (f.oarc[e].y == (int) y) break;
            if (e >= e1) return 0;
            q2 = f.oarc[e].x;
            R w = f.ow[e];
            if ((int) y == f.sep) {
                int h2;
                R a;
                if (!f.step(h, f.wos[f.state[q]], h2, a)) return 0;
                h = h2;
                w = w + a;
            }
            s = s + w;
        }
        if (n >= max_n) return 0;                          // (cannot happen: max_n >= tl)
        if (key) key[n] = f.pair(h, q2);
        ++n;
        q = q2;
        prev = y;
    }
    if (n == 0) return 0;
    R e;
    int w;
    if (!word_end<R>(f, fw, h, q, (R) 0, e, w) || !(e > NINF)) return 0;
    score = s + e;
    return n;
}

template <typename R>
__global__ void __launch_bounds__(64) beam_word_loss_targets(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm,
                                                             BeamWordLossLayout lay, char *work) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= P.B) return;
    char *wb = work + (size_t) b * lay.per;
    int *hdr = (int *) (wb + lay.hdr);
    int n = 0;
    if (P.targets && lay.nf > 0) {
        BeamWordFrame<R> f;
        bind_walk<R>(f, g, bg, lm);
        const int len = clamp_len(P.in_len, b, P.T);
        const int64_t l = P.tg_len ? P.tg_len[b] : P.S;
        const int tl = (int) (l < 0 ? 0 : (l > P.S ? P.S : l));
        R score;
        if (tl >= 1 && tl <= len)                          // (otherwise the target has no alignment)
            n = walk_target<R>(f, (const R *) g.final_w, P, b, tl, lay.nf, (unsigned long long *) (wb + lay.key), score);
    }
    hdr[0] = n;
}

template <typename R>
__global__ void __launch_bounds__(64) beam_word_target_scores(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, R *out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= P.B) return;
    BeamWordFrame<R> f;
    bind_walk<R>(f, g, bg, lm);
    const int64_t l = P.tg_len ? P.tg_len[b] : P.S;
    const int tl = (int) (l < 0 ? 0 : (l > P.S ? P.S : l));
    R score;
    (void) walk_target<R>(f, (const R *) g.final_w, P, b, tl, tl, nullptr, score);
    out[b] = score;
}

// ---------------------------------------------------------------------------------------------------------------------
// 3: U_t = A_t united with F_t, ascending in pair order, without duplicates.  Block x = utterance; the blocks of y stride over
// the frames (gridDim.y <= 65535).  Dynamic LDS: u64 [P2], P2 a power of two >= M; a frame sorts only the p2 <= P2 slots its
// own |A_t| + |F_t| needs.  A pair key is below 2^50: bit 63 flags a duplicate, all other bits set pads.
// ---------------------------------------------------------------------------------------------------------------------
__device__ void bitonic_sort64(unsigned long long *v, int P2) {
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = threadIdx.x; x < P2; x += kWS) {
                const int y = x ^ j;
                if (y > x) {
                    const unsigned long long a = v[x], c = v[y];
                    const bool up = (x & k) == 0;
                    if ((a > c) == up) { v[x] = c; v[y] = a; }
                }
            }
            __syncthreads();
        }
}

__global__ void __launch_bounds__(kWS) beam_word_loss_sets(Problem P, BeamWordLossLayout lay, int K, int qbits, int P2, char *work) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int count;
    unsigned long long *v = (unsigned long long *) lds;
    const int b = blockIdx.x, tid = threadIdx.x, T = P.T, M = lay.M;
    char *wb = work + (size_t) b * lay.per;
    int *nu = (int *) (wb + lay.nu);
    const int len = clamp_len(P.in_len, b, T);
    const unsigned long long *fk = (const unsigned long long *) (wb + lay.key);
    const int n = ((const int *) (wb + lay.hdr))[0];
    const unsigned long long FLAG = 1ull << 63, BIG = ~FLAG;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        if (t >= len) { if (tid == 0) nu[t] = 0; continue; }
        const int *bq = (const int *) (wb + lay.bq) + (int64_t) t * K, *bh = (const int *) (wb + lay.bh) + (int64_t) t * K;
        int na = ((const int *) (wb + lay.cnt))[t];
        na = na < 0 ? 0 : (na > K ? K : na);
        // F_t = { p_k : k - 1 <= t and n - k <= len - 1 - t }, k = 1 .. n
        int k0 = n - (len - 1 - t), k1 = t + 1;
        if (k0 < 1) k0 = 1;
        if (k1 > n) k1 = n;
        int nf = k1 >= k0 ? k1 - k0 + 1 : 0;
        if (na + nf > M) nf = M - na;                                           // (cannot happen: n <= lay.nf)
        int p2 = 2;
        while (p2 < na + nf) p2 *= 2;                                           // <= P2: na + nf <= M <= P2
        for (int x = tid; x < p2; x += kWS) {
            unsigned long long p = BIG;
            if (x < na) p = ((unsigned long long) (unsigned) bh[x] << qbits) | (unsigned) bq[x];
            else if (x < na + nf) p = fk[k0 - 1 + (x - na)];
            v[x] = p;
        }
        if (tid == 0) count = 0;
        __syncthreads();
        bitonic_sort64(v, p2);
        // duplicates: flag them in bit 63 (the neighbour's comparison masks it), then blank them and count the rest
        for (int x = tid; x < p2; x += kWS) {
            const unsigned long long a = v[x] & BIG;
            if (x > 0 && a != BIG && a == (v[x - 1] & BIG)) atomicOr(&v[x], FLAG);
        }
        __syncthreads();
        int c = 0;
        for (int x = tid; x < p2; x += kWS) {
            if (v[x] & FLAG) v[x] = BIG;
            else if (v[x] != BIG) ++c;
        }
        if (c) atomicAdd(&count, c);
        __syncthreads();
        bitonic_sort64(v, p2);
        const int m = count;
        unsigned long long *U = (unsigned long long *) (wb + lay.U) + (int64_t) t * M;
        for (int x = tid; x < m; x += kWS) U[x] = v[x];
        if (tid == 0) nu[t] = m;
        __syncthreads();                                                        // v and count are the next frame's
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 4: alpha over the U_t, and Z_K.  Dynamic LDS: [reduction slots][ut u64 M][sm u64 M][mk key M].
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kWL) beam_word_loss_fwd(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm,
                                                          BeamWordLossLayout lay, int store, char *work, R *scores) {
    using KT = Key<R>;
    using KU = typename KT::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    R *red = (R *) lds;
    const int M = lay.M;
    unsigned long long *ut = (unsigned long long *) (lds + kWLHead);      // [M] U_t
    unsigned long long *sm = ut + M;                                      // [M] sum of exp(c - max), 48 fractional bits
    KU *mk = (KU *) (sm + M);                                             // [M] max candidate as a key, 0: none
    const int tid = threadIdx.x, b = blockIdx.x, T = P.T;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    if (len < 1) { if (tid == 0) scores[b] = NINF; return; }
    char *wb = work + (size_t) b * lay.per;
    const unsigned long long *U = (const unsigned long long *) (wb + lay.U);
    const int *nu = (const int *) (wb + lay.nu);
    R *A = (R *) (wb + lay.A);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *trm = (const R *) P.transition;
    const R *fw = (const R *) g.final_w;
    BeamWordFrame<R> f;
    bind_walk<R>(f, g, bg, lm);
    const unsigned long long qmask = (1ull << f.qbits) - 1ull;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };

    int mp = nu[0];
    for (int x = tid; x < mp; x += kWL) {
        const unsigned long long p = U[x];
        const int q = (int) (p & qmask), h = (int) (p >> f.qbits);
        dev_store(A + x, h == f.lstart ? f.sw[q] + in[(int64_t) f.label[q] * P.is2] : NINF);
    }
    __threadfence();
    __syncthreads();
    for (int t = 1; t < len; ++t) {
        const int mt = nu[t];
        const unsigned long long *Up = U + (int64_t) (t - 1) * M, *Ut = U + (int64_t) t * M;
        const R *Ap = A + (int64_t) (store ? t - 1 : ((t - 1) & 1)) * M;
        R *Arow = A + (int64_t) (store ? t : (t & 1)) * M;
        const R *xt = in + (int64_t) t * P.is0;
        for (int x = tid; x < mt; x += kWL) { ut[x] = Ut[x]; sm[x] = 0ull; mk[x] = (KU) 0; }
        __syncthreads();
        const int G = wsubgroup(mp), per = kWL / G;
        for (int pass = 0; pass < 2; ++pass) {
            for (int k0 = 0; k0 < mp; k0 += per) {
                const int k = k0 + tid / G, lg = tid % G;
                if (k >= mp) continue;
                const R a = dev_load(Ap + k);
                if (!(a > NINF)) continue;
                const unsigned long long p = Up[k];
                const int qs = (int) (p & qmask), hs = (int) (p >> f.qbits);
                const int j = f.label[qs];
                auto offer = [&](unsigned long long tp, R c) {
                    if (!(c > NINF)) return;
                    const int pos = find_pair(ut, mt, tp);
                    if (pos < 0) return;
                    if (pass == 0) atomicMax(mk + pos, KT::enc(c));
                    else {
                        const unsigned long long fx = w_fixed((double) wexp(c - KT::dec(mk[pos])), kWSumScale);
                        if (fx) atomicAdd(sm + pos, fx);
                    }
                };
                if (lg == 0) offer(p, a + tr(j, j));
                const int e1 = f.orow[qs + 1];
                for (int e = f.orow[qs] + lg; e < e1; e += G) {
                    const int2 arc = f.oarc[e];
                    int th = hs;
                    R w = f.ow[e];
                    if (arc.y == f.sep) {                             // a word ends: the LM moves
                        R add;
                        int h2;
                        if (!f.step(hs, f.wos[f.state[qs]], h2, add)) continue;
                        th = h2;
                        w = w + add;
                    }
                    offer(f.pair(th, arc.x), (a + tr(arc.y, j)) + w);
                }
            }
            __syncthreads();
        }
        for (int x = tid; x < mt; x += kWL) {
            const KU key = mk[x];
            R v = NINF;
            if (key != 0 && sm[x] != 0ull) {
                const R s = (R) ((double) sm[x] * (1.0 / kWSumScale));
                v = (KT::dec(key) + wlog(s)) + xt[(int64_t) f.label[(int) (ut[x] & qmask)] * P.is2];
            }
            dev_store(Arow + x, v);
        }
        __threadfence();
        __syncthreads();
        mp = mt;
    }
    // Z_K over the last lattice set: every kind of end through word_end
    const unsigned long long *Ul = U + (int64_t) (len - 1) * M;
    const R *Al = A + (int64_t) (store ? len - 1 : ((len - 1) & 1)) * M;
    auto end_of = [&](int x) -> R {
        const unsigned long long p = Ul[x];
        R e;
        int w;
        const R a = dev_load(Al + x);
        if (!(a > NINF) || !word_end<R>(f, fw, (int) (p >> f.qbits), (int) (p & qmask), a, e, w)) return NINF;
        return e;
    };
    R m = NINF;
    for (int x = tid; x < mp; x += kWL) m = wmax(m, end_of(x));
    m = wwg_max(m, red);
    R Z = NINF;
    if (m > NINF) {
        R s = R(0);
        for (int x = tid; x < mp; x += kWL) {
            const R e = end_of(x);
            if (e > NINF) s += wexp(e - m);
        }
        s = wwg_sum(s, red);
        Z = m + wlog(s);
    }
    if (tid == 0) scores[b] = Z;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward.  Dynamic LDS: [reduction slots][nq u64 M][nb R M][gi u64 N][tile u64 N*N if TL].
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wtile_shift(int len) {       // fractional bits of an utterance's (i, j) counts
    int c = 0;
    while ((1 << c) < len && c < 30) ++c;
    return 62 - c;
}

__host__ __device__ inline size_t wbwd_front(int elem, int M) { return ((size_t) M * (8 + elem) + 15) & ~(size_t) 15; }

template <typename R, bool TL>
__global__ void __launch_bounds__(kWL) beam_word_loss_bwd(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm,
                                                          BeamWordLossLayout lay, const char *work, const R *Zs, const R *gs, R *gin,
                                                          char *scratch, size_t sper) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int M = lay.M, N = P.N, T = P.T;
    unsigned long long *nq = (unsigned long long *) (lds + kWLHead);      // [M] U_t
    R *nb = (R *) (nq + M);                                               // [M] beta[t] of U_t
    unsigned long long *gi = (unsigned long long *) (lds + kWLHead + wbwd_front(sizeof(R), M));
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t B = P.B;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    const R Z = Zs[b], gb = gs[b];
    const bool ok = len >= 1 && Z > NINF;
    char *sb = scratch + (size_t) b * sper;
    R *Bv = (R *) sb;                                                          // [2][M]
    unsigned long long *gtile = (unsigned long long *) (sb + a256(2 * (size_t) M * sizeof(R)));
    unsigned long long *tile = TL ? gi + N : gtile;
    const int t0 = ok ? len : 0;
    for (int64_t x = tid; x < (int64_t) (T - t0) * N; x += kWL) gin[((int64_t) (t0 + x / N) * B + b) * N + x % N] = R(0);
    for (int x = tid; x < N * N; x += kWL) tile[x] = 0ull;
    if (!ok) {
        if (TL) for (int x = tid; x < N * N; x += kWL) gtile[x] = 0ull;
        return;
    }
    for (int x = tid; x < N; x += kWL) gi[x] = 0ull;
    const char *wb = work + (size_t) b * lay.per;
    const unsigned long long *U = (const unsigned long long *) (wb + lay.U);
    const int *nu = (const int *) (wb + lay.nu);
    const R *A = (const R *) (wb + lay.A);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *trm = (const R *) P.transition;
    const R *fw = (const R *) g.final_w;
    BeamWordFrame<R> f;
    bind_walk<R>(f, g, bg, lm);
    const unsigned long long qmask = (1ull << f.qbits) - 1ull;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };
    const double tscale = (double) (1ull << wtile_shift(len));

    int mt = nu[len - 1];
    for (int x = tid; x < mt; x += kWL) {
        const unsigned long long p = U[(int64_t) (len - 1) * M + x];
        R e;
        int w;
        nq[x] = p;
        nb[x] = word_end<R>(f, fw, (int) (p >> f.qbits), (int) (p & qmask), (R) 0, e, w) ? e : NINF;
    }
    __threadfence();
    __syncthreads();
    for (int t = len - 1; t >= 0; --t) {
        const R *At = A + (int64_t) t * M;
        for (int x = tid; x < mt; x += kWL) {
            const R gam = wexp((At[x] + nb[x]) - Z);
            const unsigned long long fx = w_fixed((double) gam, kWGammaScale);
            if (fx) atomicAdd(&gi[f.label[(int) (nq[x] & qmask)]], fx);
        }
        __syncthreads();
        for (int i = tid; i < N; i += kWL) {
            gin[((int64_t) t * B + b) * N + i] = gb * (R) ((double) gi[i] * (1.0 / kWGammaScale));
            gi[i] = 0ull;
        }
        if (t == 0) break;
        const int mp = nu[t - 1];
        const unsigned long long *Up = U + (int64_t) (t - 1) * M;
        const R *Ap = A + (int64_t) (t - 1) * M;
        R *Brow = Bv + (int64_t) ((t - 1) & 1) * M;
        const R *xt = in + (int64_t) t * P.is0;
        const int G = wsubgroup(mp), per = kWL / G;
        for (int k0 = 0; k0 < mp; k0 += per) {
            const int k = k0 + tid / G, lg = tid % G;
            const bool act = k < mp;
            const unsigned long long pp = act ? Up[k] : 0ull;
            const int qp = (int) (pp & qmask), hp = (int) (pp >> f.qbits);
            const int ip = act ? f.label[qp] : 0;
            const int e0 = act ? f.orow[qp] : 0, e1 = act ? f.orow[qp + 1] : 0;
            // every surviving candidate out of the pair that this lane owns: fn(value, label of the target)
            auto visit = [&](auto fn) {
                if (!act) return;
                if (lg == 0) {
                    const int pos = find_pair(nq, mt, pp);
                    if (pos >= 0) fn((nb[pos] + tr(ip, ip)) + xt[(int64_t) ip * P.is2], ip);
                }
                for (int e = e0 + lg; e < e1; e += G) {
                    const int2 arc = f.oarc[e];
                    int th = hp;
                    R w = f.ow[e];
                    if (arc.y == f.sep) {
                        R add;
                        int h2;
                        if (!f.step(hp, f.wos[f.state[qp]], h2, add)) continue;
                        th = h2;
                        w = w + add;
                    }
                    const int pos = find_pair(nq, mt, f.pair(th, arc.x));
                    if (pos >= 0) fn(((nb[pos] + tr(arc.y, ip)) + w) + xt[(int64_t) arc.y * P.is2], arc.y);
                }
            };
            R mx = NINF;
            visit([&](R c, int) { mx = wmax(mx, c); });
            mx = wgroup_max(mx, G);
            R s = R(0);
            if (mx > NINF) {
                const R a = Ap[k < mp ? k : 0];
                visit([&](R c, int i) {
                    if (!(c > NINF)) return;
                    s += wexp(c - mx);
                    const unsigned long long fx = w_fixed((double) wexp((a + c) - Z), tscale);
                    if (fx) atomicAdd(&tile[(int64_t) i * N + ip], fx);
                });
            }
            s = wgroup_sum(s, G);
            if (act && lg == 0) dev_store(Brow + k, mx > NINF ? mx + wlog(s) : NINF);
        }
        __threadfence();
        __syncthreads();
        for (int x = tid; x < mp; x += kWL) { nq[x] = Up[x]; nb[x] = dev_load(Brow + x); }
        mt = mp;
        __syncthreads();
    }
    if (TL) {
        __syncthreads();
        for (int x = tid; x < N * N; x += kWL) gtile[x] = tile[x];
    }
}

// grad_transition[i][j] (+)= sum over the utterances, ascending, of grad_scores[b] * tile_b[i][j]
template <typename R>
__global__ void __launch_bounds__(kWS) beam_word_loss_tr_reduce(Problem P, int M, const char *scratch, size_t sper, const R *Zs,
                                                                const R *gs, int accumulate, R *gtr) {
    const int x = blockIdx.x * kWS + threadIdx.x, N = P.N;
    if (x >= N * N) return;
    R s = accumulate ? gtr[x] : R(0);
    const size_t toff = a256(2 * (size_t) M * sizeof(R));
    for (int b = 0; b < P.B; ++b) {
        const int len = clamp_len(P.in_len, b, P.T);
        if (len < 1 || !(Zs[b] > Num<R>::ninf())) continue;
        const unsigned long long v = ((const unsigned long long *) (scratch + (size_t) b * sper + toff))[x];
        s += gs[b] * (R) ((double) v / (double) (1ull << wtile_shift(len)));
    }
    gtr[x] = s;
}

inline size_t wfwd_lds(int elem, int M) { return kWLHead + (size_t) M * (16 + elem); }
inline size_t wbwd_lds(int elem, int M, int N, bool tl) {
    return kWLHead + wbwd_front(elem, M) + (size_t) N * 8 + (tl ? (size_t) N * N * 8 : 0);
}

// a launch whose LDS -- dynamic plus the kernel's own `fixed` static bytes -- passes 64 KiB has to ask for it
inline void wset_lds(const void *fn, size_t dyn, size_t fixed = 0) {
    if (dyn + fixed > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);
}

}  // namespace

BeamWordLossLayout beam_word_loss_layout(int elem, int T, int K, int cap, int nf, bool store) {
    BeamWordLossLayout l{};
    l.nf = nf;
    l.M = K + nf;
    const BeamWordWorkLayout w = beam_word_work_layout(elem, T, K, cap, word_table_bits(cap));   // the search's own part, in front
    l.bq = w.bq;
    l.bh = w.bh;
    size_t off = w.end;
    l.cnt = off; off += a256((size_t) T * 4);
    l.nu = off;  off += a256((size_t) T * 4);
    l.hdr = off; off += 256;
    l.key = off; off += a256((size_t) nf * 8);
    l.U = off;   off += a256((size_t) T * l.M * 8);
    l.A = off;   off += a256((size_t) (store ? T : 2) * l.M * elem);
    l.per = off;
    return l;
}

size_t beam_word_loss_work_bytes(int elem, int T, int B, int K, int cap, int nf, bool store) {
    return (size_t) B * beam_word_loss_layout(elem, T, K, cap, nf, store).per;
}

size_t beam_word_loss_scratch_per(int elem, int M, int N) { return a256(2 * (size_t) M * elem) + a256((size_t) N * N * 8); }

// THE bound on M = K + nf: a frame's lattice set with the maximum and the sum of every member (forward), and with its beta
// and the label posteriors (backward), stays in 160 KiB of LDS.
bool beam_word_loss_fits(int elem, int M, int N) {
    return wfwd_lds(elem, M) <= kWLLds && wbwd_lds(elem, M, N, false) <= kWLLds;
}

template <typename R>
hipError_t launch_beam_word_loss_forward(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, int K,
                                         double theta, bool store, void *work, void *scores, hipStream_t stream) {
    const int T = P.T, B = P.B, N = P.N;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const int tbits = word_table_bits(cap);
    const int nf = P.targets ? (P.S < T ? P.S : T) : 0;
    const BeamWordLossLayout lay = beam_word_loss_layout(sizeof(R), T, K, cap, nf, store);
    char *w = (char *) work;
    {
        const size_t beam = kFixedLds + (size_t) K * (sizeof(R) + 8);
        const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
        const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
        if (trl) {
            wset_lds((const void *) beam_word_loss_search<R, true>, dyn);
            hipLaunchKernelGGL((beam_word_loss_search<R, true>), dim3(B), dim3(kBT), dyn, stream, P, G, BG, LM, K, (R) theta, cap,
                               tbits, w, lay.per, lay.cnt);
        } else {
            wset_lds((const void *) beam_word_loss_search<R, false>, dyn);
            hipLaunchKernelGGL((beam_word_loss_search<R, false>), dim3(B), dim3(kBT), dyn, stream, P, G, BG, LM, K, (R) theta, cap,
                               tbits, w, lay.per, lay.cnt);
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((beam_word_loss_targets<R>), dim3((B + 63) / 64), dim3(64), 0, stream, P, G, BG, LM, lay, w);
    int P2 = 2;
    while (P2 < lay.M) P2 *= 2;
    int qbits = 1;
    while (((int64_t) 1 << qbits) < G.Q) ++qbits;                                // (bits_of on the host)
    wset_lds((const void *) beam_word_loss_sets, (size_t) P2 * 8, sizeof(int));
    hipLaunchKernelGGL(beam_word_loss_sets, dim3(B, T < 65535 ? T : 65535), dim3(kWS), (size_t) P2 * 8, stream, P, lay, K, qbits,
                       P2, w);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t dyn = wfwd_lds(sizeof(R), lay.M);
    wset_lds((const void *) beam_word_loss_fwd<R>, dyn);
    hipLaunchKernelGGL((beam_word_loss_fwd<R>), dim3(B), dim3(kWL), dyn, stream, P, G, BG, LM, lay, (int) store, w, (R *) scores);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_word_loss_backward(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, int K,
                                          const void *work, const void *scores, const void *grad_scores, void *grad_inputs,
                                          void *grad_transition, void *scratch, bool accumulate, hipStream_t stream) {
    const int T = P.T, B = P.B, N = P.N;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const int nf = P.targets ? (P.S < T ? P.S : T) : 0;
    const BeamWordLossLayout lay = beam_word_loss_layout(sizeof(R), T, K, cap, nf, true);
    const size_t sper = beam_word_loss_scratch_per(sizeof(R), lay.M, N);
    const bool tl = wbwd_lds(sizeof(R), lay.M, N, true) <= kWLLds;
    const size_t dyn = wbwd_lds(sizeof(R), lay.M, N, tl);
    if (tl) {
        wset_lds((const void *) beam_word_loss_bwd<R, true>, dyn);
        hipLaunchKernelGGL((beam_word_loss_bwd<R, true>), dim3(B), dim3(kWL), dyn, stream, P, G, BG, LM, lay, (const char *) work,
                           (const R *) scores, (const R *) grad_scores, (R *) grad_inputs, (char *) scratch, sper);
    } else {
        wset_lds((const void *) beam_word_loss_bwd<R, false>, dyn);
        hipLaunchKernelGGL((beam_word_loss_bwd<R, false>), dim3(B), dim3(kWL), dyn, stream, P, G, BG, LM, lay, (const char *) work,
                           (const R *) scores, (const R *) grad_scores, (R *) grad_inputs, (char *) scratch, sper);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((beam_word_loss_tr_reduce<R>), dim3((N * N + kWS - 1) / kWS), dim3(kWS), 0, stream, P, lay.M,
                       (const char *) scratch, sper, (const R *) scores, (const R *) grad_scores, (int) accumulate,
                       (R *) grad_transition);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_word_target_scores(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                          void *out, hipStream_t stream) {
    hipLaunchKernelGGL((beam_word_target_scores<R>), dim3((P.B + 63) / 64), dim3(64), 0, stream, P, G, BG, LM, (R *) out);
    return hipGetLastError();
}

#define ASG_WORD_LOSS_INST(R)                                                                                                    \
    template hipError_t launch_beam_word_loss_forward<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &,             \
                                                         const WordLmArgs &, int, double, bool, void *, void *, hipStream_t);   \
    template hipError_t launch_beam_word_loss_backward<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &,            \
                                                          const WordLmArgs &, int, const void *, const void *, const void *,    \
                                                          void *, void *, void *, bool, hipStream_t);                           \
    template hipError_t launch_beam_word_target_scores<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &,            \
                                                          const WordLmArgs &, void *, hipStream_t);
ASG_WORD_LOSS_INST(float)
ASG_WORD_LOSS_INST(double)
#undef ASG_WORD_LOSS_INST

}  // namespace asg
