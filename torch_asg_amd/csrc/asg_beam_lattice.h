// torch_asg_amd/csrc/asg_beam_lattice.h -- the LATTICE PASS behind the search that the two beam-pruned losses share
// (asg_beam_loss.hip over int product states, asg_beam_word_loss.hip over 64-bit pairs h << qbits | q).  Both
// units compile this one text:
//   - the small helpers: exp / log / max, the fixed-point conversion, the butterflies and workgroup reductions, `subgroup`,
//     `find_sorted`, `tile_shift`, `set_lds`, the LDS and scratch sizes of the backward;
//   - beam_loss_sets<Pol>: U_t = A_t united with F_t, ascending, without duplicates.  Pol, a kernel argument, holds the family's
//     layout and says what a key is: `Key`, `kFlag` (the bit that marks a duplicate; every other bit set is the pad),
//     `kept(wb, t, x)` (key x of A_t from the search's rows) and `forced(wb)` (the keys of the target, in target order);
//   - lattice_z: Z_K = logsumexp over the last set of an end term handed in as a callable (the tail of both alpha kernels);
//   - beam_loss_bwd<R, TL, Lat>: beta, the label posteriors and the (i, j) counts.  Lat is bound once from the kernel's
//     argument pack Lat::Args (which ends in the family's layout, `lay`) and supplies `Key`, `label(key)`, `end(key, e)` and
//     `for_each_out(key, lg, G, fn)`: fn(target key, w, target label) for the outgoing edges that lane lg of G owns, where
//     w() gives the edge weight -- a callable, so that the weight of an edge whose target is not kept is never loaded;
//   - beam_loss_tr_reduce<R> and the body of the backward launcher.
// asg_beam_word_conf_pull.h includes it for the small helpers alone: the beta pull of the two confidence calls
// is a text of its own.
// The two alpha kernels are different algorithms (a pull through incoming rows, a push with integer atomics) and stay in
// their units, as do the searches and the target walks.
#pragma once
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"     // clamp_len, a256
#include "asg_beam_frame.h"      // dev_load, dev_store

namespace asg {

namespace {

constexpr int kBL = 1024;                       // forward / backward workgroup
constexpr int kBS = 256;                        // target walk / set / reduction workgroups
constexpr size_t kBLHead = 256;                 // reduction slots in front of the dynamic LDS
constexpr size_t kBLLds = 160 * 1024;
constexpr double kGammaScale = 4611686018427387904.0;        // 2^62

template <typename R> __device__ __forceinline__ R bexp(R x);
template <> __device__ __forceinline__ float bexp<float>(float x) { return expf(x); }
template <> __device__ __forceinline__ double bexp<double>(double x) { return ::exp(x); }
template <typename R> __device__ __forceinline__ R blog(R x);
template <> __device__ __forceinline__ float blog<float>(float x) { return logf(x); }
template <> __device__ __forceinline__ double blog<double>(double x) { return ::log(x); }
template <typename R> __device__ __forceinline__ R bmax(R a, R b) { return b > a ? b : a; }

__device__ __forceinline__ unsigned long long to_fixed(double p, double scale) {
    return p > 0.0 ? (unsigned long long) (p * scale) : 0ull;
}

// position of key q in the ascending list a[0 .. n), -1 if absent
template <typename KeyT> __device__ __forceinline__ int find_sorted(const KeyT *a, int n, KeyT q) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < q) lo = mid + 1; else hi = mid;
    }
    return (lo < n && a[lo] == q) ? lo : -1;
}

// sum / max over the G lanes of a subgroup (G a power of two <= 64, subgroups aligned): every lane gets the same bits
template <typename R> __device__ __forceinline__ R group_max(R v, int G) {
    for (int o = 1; o < G; o <<= 1) v = bmax(v, (R) __shfl_xor(v, o));
    return v;
}
template <typename R> __device__ __forceinline__ R group_sum(R v, int G) {
    for (int o = 1; o < G; o <<= 1) v += (R) __shfl_xor(v, o);
    return v;
}

template <typename R>
__device__ R wg_max(R v, R *red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = group_max(v, 64);
    if (lane == 0) red[w] = v;
    __syncthreads();
    v = red[0];
    for (int s = 1; s < kBL / 64; ++s) v = bmax(v, red[s]);
    __syncthreads();
    return v;
}
template <typename R>
__device__ R wg_sum(R v, R *red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = group_sum(v, 64);
    if (lane == 0) red[w] = v;
    __syncthreads();
    v = red[0];
    for (int s = 1; s < kBL / 64; ++s) v += red[s];
    __syncthreads();
    return v;
}

// lanes per member of a set of m: the largest power of two <= 64 with G * m <= 1024
__device__ __forceinline__ int subgroup(int m) {
    int G = 1;
    while (G < 64 && G * 2 * m <= kBL) G *= 2;
    return G;
}

__device__ __forceinline__ int tile_shift(int len) {        // fractional bits of an utterance's (i, j) counts
    int c = 0;
    while ((1 << c) < len && c < 30) ++c;
    return 62 - c;
}

// a launch whose LDS -- dynamic plus the kernel's own `fixed` static bytes -- passes 64 KiB has to ask for it
inline void set_lds(const void *fn, size_t dyn, size_t fixed = 0) {
    if (dyn + fixed > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);
}

// ---------------------------------------------------------------------------------------------------------------------
// U_t = A_t united with F_t, ascending, without duplicates.  Block x = utterance; the blocks of y stride over the frames
// (gridDim.y <= 65535), so neither B nor T meets a grid limit the other launches do not have.  Dynamic LDS: Key [P2], P2 a
// power of two >= max(M, 2); a frame sorts only the p2 <= P2 slots its own |A_t| + |F_t| needs.  The sorted unique set does not
// depend on how many pads were sorted with it.
// ---------------------------------------------------------------------------------------------------------------------
// (bitonic_sort_wg: ascending sort of v[0 .. P2), P2 a power of two, by a whole workgroup of WG threads -- kBS here, kBL in the
// catch-up of the lattice-keeping streams, asg_beam_stream_lat.h)
template <typename KeyT, int WG>
__device__ void bitonic_sort_wg(KeyT *v, int P2) {
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = threadIdx.x; x < P2; x += WG) {
                const int y = x ^ j;
                if (y > x) {
                    const KeyT a = v[x], c = v[y];
                    const bool up = (x & k) == 0;
                    if ((a > c) == up) { v[x] = c; v[y] = a; }
                }
            }
            __syncthreads();
        }
}

template <typename Pol>
__global__ void __launch_bounds__(kBS) beam_loss_sets(Problem P, Pol pol, char *work) {
    using KeyT = typename Pol::Key;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int count;
    KeyT *v = (KeyT *) lds;
    const int b = blockIdx.x, tid = threadIdx.x, T = P.T, M = pol.lay.M, K = pol.K;
    char *wb = work + (size_t) b * pol.lay.per;
    int *nu = (int *) (wb + pol.lay.nu);
    const int len = clamp_len(P.in_len, b, T);
    const KeyT *fk = pol.forced(wb);
    const int n = ((const int *) (wb + pol.lay.hdr))[0];
    constexpr KeyT FLAG = Pol::kFlag, BIG = ~FLAG;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        if (t >= len) { if (tid == 0) nu[t] = 0; continue; }
        int na = ((const int *) (wb + pol.lay.cnt))[t];
        na = na < 0 ? 0 : (na > K ? K : na);
        // F_t = { key_k : k - 1 <= t and n - k <= len - 1 - t }, k = 1 .. n
        int k0 = n - (len - 1 - t), k1 = t + 1;
        if (k0 < 1) k0 = 1;
        if (k1 > n) k1 = n;
        int nf = k1 >= k0 ? k1 - k0 + 1 : 0;
        if (na + nf > M) nf = M - na;                                           // (cannot happen: n <= lay.nf)
        int p2 = 2;
        while (p2 < na + nf) p2 *= 2;                                           // <= P2: na + nf <= M <= P2
        for (int x = tid; x < p2; x += kBS) v[x] = x < na ? pol.kept(wb, t, x) : (x < na + nf ? fk[k0 - 1 + (x - na)] : BIG);
        if (tid == 0) count = 0;
        __syncthreads();
        bitonic_sort_wg<KeyT, kBS>(v, p2);
        // duplicates: flag them in the top bit (the neighbour's comparison masks it), then blank them and count the rest
        for (int x = tid; x < p2; x += kBS) {
            const KeyT a = v[x] & BIG;
            if (x > 0 && a != BIG && a == (v[x - 1] & BIG)) atomicOr(&v[x], FLAG);
        }
        __syncthreads();
        int c = 0;
        for (int x = tid; x < p2; x += kBS) {
            if (v[x] & FLAG) v[x] = BIG;
            else if (v[x] != BIG) ++c;
        }
        if (c) atomicAdd(&count, c);
        __syncthreads();
        bitonic_sort_wg<KeyT, kBS>(v, p2);
        const int m = count;
        KeyT *U = (KeyT *) (wb + pol.lay.U) + (int64_t) t * M;
#pragma nounroll                                                                // (unrolled 16 times it costs the int keys 32 VGPRs)
        for (int x = tid; x < m; x += kBS) U[x] = v[x];
        if (tid == 0) nu[t] = m;
        __syncthreads();                                                        // v and count are the next frame's
    }
}

template <typename Pol>
hipError_t launch_beam_loss_sets(const Problem &P, const Pol &pol, char *work, hipStream_t stream) {
    int P2 = 2;
    while (P2 < pol.lay.M) P2 *= 2;
    const size_t dyn = (size_t) P2 * sizeof(typename Pol::Key);
    set_lds((const void *) beam_loss_sets<Pol>, dyn, sizeof(int));             // (64 KiB of slots beside its `int count`)
    hipLaunchKernelGGL(beam_loss_sets<Pol>, dim3(P.B, P.T < 65535 ? P.T : 65535), dim3(kBS), dyn, stream, P, pol, work);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Z_K = logsumexp over the m members of the last set of end(x) (-inf: member x has no end).  The whole workgroup calls it.
// ---------------------------------------------------------------------------------------------------------------------
template <typename R, typename End>
__device__ __forceinline__ R lattice_z(int m, R *red, End end) {
    const R NINF = Num<R>::ninf();
    R mx = NINF;
    for (int x = threadIdx.x; x < m; x += kBL) mx = bmax(mx, end(x));
    mx = wg_max(mx, red);
    R Z = NINF;
    if (mx > NINF) {
        R s = R(0);
        for (int x = threadIdx.x; x < m; x += kBL) s += bexp(end(x) - mx);    // (exp(-inf - mx) is 0)
        s = wg_sum(s, red);
        Z = mx + blog(s);
    }
    return Z;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward.  Dynamic LDS: [reduction slots][nb R M and nq Key M, the 8-byte keys in front, the 4-byte keys behind, so that
// neither array is misaligned by an odd M][gi u64 N][tile u64 N*N if TL].  Scratch of an utterance: beta [2][M], the tile.
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline size_t bwd_front(int elem, int key, int M) { return ((size_t) M * (elem + key) + 15) & ~(size_t) 15; }
inline size_t bwd_lds(int elem, int key, int M, int N, bool tl) {
    return kBLHead + bwd_front(elem, key, M) + (size_t) N * 8 + (tl ? (size_t) N * N * 8 : 0);
}

template <typename R, bool TL, typename Lat>
__global__ void __launch_bounds__(kBL) beam_loss_bwd(Problem P, typename Lat::Args args, const char *work, const R *Zs, const R *gs,
                                                     R *gin, char *scratch, size_t sper) {
    using KeyT = typename Lat::Key;
    constexpr bool kKeysFirst = sizeof(KeyT) == 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int M = args.lay.M, N = P.N, T = P.T;
    R *nb = (R *) (lds + kBLHead + (kKeysFirst ? (size_t) M * sizeof(KeyT) : 0));          // [M] beta[t] of U_t
    KeyT *nq = (KeyT *) (lds + kBLHead + (kKeysFirst ? 0 : (size_t) M * sizeof(R)));       // [M] U_t
    unsigned long long *gi = (unsigned long long *) (lds + kBLHead + bwd_front(sizeof(R), sizeof(KeyT), M));
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
    for (int64_t x = tid; x < (int64_t) (T - t0) * N; x += kBL) gin[((int64_t) (t0 + x / N) * B + b) * N + x % N] = R(0);
    for (int x = tid; x < N * N; x += kBL) tile[x] = 0ull;
    if (!ok) {
        if (TL) for (int x = tid; x < N * N; x += kBL) gtile[x] = 0ull;
        return;
    }
    for (int x = tid; x < N; x += kBL) gi[x] = 0ull;
    const char *wb = work + (size_t) b * args.lay.per;
    const KeyT *U = (const KeyT *) (wb + args.lay.U);
    const int *nu = (const int *) (wb + args.lay.nu);
    const R *A = (const R *) (wb + args.lay.A);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *trm = (const R *) P.transition;
    Lat lat;
    lat.bind(args);
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };
    const double tscale = (double) (1ull << tile_shift(len));

    int mt = nu[len - 1];
    for (int x = tid; x < mt; x += kBL) {
        const KeyT p = U[(int64_t) (len - 1) * M + x];
        R e;
        lat.end(p, e);
        nq[x] = p;
        nb[x] = e;
    }
    __threadfence();
    __syncthreads();
    for (int t = len - 1; t >= 0; --t) {
        const R *At = A + (int64_t) t * M;
        for (int x = tid; x < mt; x += kBL) {
            const R gam = bexp((At[x] + nb[x]) - Z);
            const unsigned long long f = to_fixed((double) gam, kGammaScale);
            if (f) atomicAdd(&gi[lat.label(nq[x])], f);
        }
        __syncthreads();
        for (int i = tid; i < N; i += kBL) {
            gin[((int64_t) t * B + b) * N + i] = gb * (R) ((double) gi[i] * (1.0 / kGammaScale));
            gi[i] = 0ull;
        }
        if (t == 0) break;
        const int mp = nu[t - 1];
        const KeyT *Up = U + (int64_t) (t - 1) * M;
        const R *Ap = A + (int64_t) (t - 1) * M;
        R *Brow = Bv + (int64_t) ((t - 1) & 1) * M;
        const R *xt = in + (int64_t) t * P.is0;
        const int G = subgroup(mp), per = kBL / G;
        for (int k0 = 0; k0 < mp; k0 += per) {
            const int k = k0 + tid / G, lg = tid % G;
            const bool act = k < mp;
            const KeyT pp = act ? Up[k] : (KeyT) 0;
            const int ip = act ? lat.label(pp) : 0;
            // every surviving candidate out of pp that this lane owns: f(value, label of the target)
            auto visit = [&](auto f) {
                if (!act) return;
                if (lg == 0) {
                    const int pos = find_sorted(nq, mt, pp);
                    if (pos >= 0) f((nb[pos] + tr(ip, ip)) + xt[(int64_t) ip * P.is2], ip);
                }
                lat.for_each_out(pp, lg, G, [&](KeyT tp, auto w, int i) {
                    const int pos = find_sorted(nq, mt, tp);
                    if (pos >= 0) f(((nb[pos] + tr(i, ip)) + w()) + xt[(int64_t) i * P.is2], i);
                });
            };
            R mx = NINF;
            visit([&](R c, int) { mx = bmax(mx, c); });
            mx = group_max(mx, G);
            R s = R(0);
            if (mx > NINF) {
                const R a = Ap[k];
                visit([&](R c, int i) {
                    s += bexp(c - mx);
                    const unsigned long long f = to_fixed((double) bexp((a + c) - Z), tscale);
                    if (f) atomicAdd(&tile[(int64_t) i * N + ip], f);
                });
            }
            s = group_sum(s, G);
            if (act && lg == 0) dev_store(Brow + k, mx > NINF ? mx + blog(s) : NINF);
        }
        __threadfence();
        __syncthreads();
        for (int x = tid; x < mp; x += kBL) { nq[x] = Up[x]; nb[x] = dev_load(Brow + x); }
        mt = mp;
        __syncthreads();
    }
    if (TL) {
        __syncthreads();
        for (int x = tid; x < N * N; x += kBL) gtile[x] = tile[x];
    }
}

// grad_transition[i][j] (+)= sum over the utterances, ascending, of grad_scores[b] * tile_b[i][j]
template <typename R>
__global__ void __launch_bounds__(kBS) beam_loss_tr_reduce(Problem P, int M, const char *scratch, size_t sper, const R *Zs, const R *gs,
                                                          int accumulate, R *gtr) {
    const int x = blockIdx.x * kBS + threadIdx.x, N = P.N;
    if (x >= N * N) return;
    R s = accumulate ? gtr[x] : R(0);
    const size_t toff = a256(2 * (size_t) M * sizeof(R));
    for (int b = 0; b < P.B; ++b) {
        const int len = clamp_len(P.in_len, b, P.T);
        if (len < 1 || !(Zs[b] > Num<R>::ninf())) continue;
        const unsigned long long v = ((const unsigned long long *) (scratch + (size_t) b * sper + toff))[x];
        s += gs[b] * (R) ((double) v / (double) (1ull << tile_shift(len)));
    }
    gtr[x] = s;
}

// The backward of a family: beam_loss_bwd<R, TL, Lat> with the tile in LDS while it fits, then the reduction.
template <typename R, typename Lat>
hipError_t launch_lattice_backward(const Problem &P, const typename Lat::Args &args, const void *work, const void *scores,
                                   const void *grad_scores, void *grad_inputs, void *grad_transition, void *scratch,
                                   bool accumulate, hipStream_t stream) {
    constexpr int key = sizeof(typename Lat::Key);
    const int B = P.B, N = P.N, M = args.lay.M;
    const size_t sper = beam_loss_scratch_per(sizeof(R), M, N);
    const bool tl = bwd_lds(sizeof(R), key, M, N, true) <= kBLLds;
    const size_t dyn = bwd_lds(sizeof(R), key, M, N, tl);
    auto bwd = tl ? beam_loss_bwd<R, true, Lat> : beam_loss_bwd<R, false, Lat>;
    set_lds((const void *) bwd, dyn);
    hipLaunchKernelGGL(bwd, dim3(B), dim3(kBL), dyn, stream, P, args, (const char *) work, (const R *) scores,
                       (const R *) grad_scores, (R *) grad_inputs, (char *) scratch, sper);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((beam_loss_tr_reduce<R>), dim3((N * N + kBS - 1) / kBS), dim3(kBS), 0, stream, P, M, (const char *) scratch,
                       sper, (const R *) scores, (const R *) grad_scores, (int) accumulate, (R *) grad_transition);
    return hipGetLastError();
}

}  // namespace

}  // namespace asg
