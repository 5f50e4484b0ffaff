// torch_asg_amd/csrc/asg_beam_loss.hip -- the BEAM-PRUNED normaliser of an ASG criterion composed with a token automaton, on
// gfx950: the log-semiring pass of asg_graph_loss.hip restricted, frame by frame, to the product states the beam search of
// asg_beam_graph.hip keeps (plus the states every alignment of the target runs through), and its gradients.  The specification
// is include/asg_hip.h::asg_beam_graph_full_forward; tests/beam_loss_ref.py restates it in numpy.
//
// Forward, four launches on one stream:
//   1  beam_graph_kernel as the decoder runs it (the same device code, so the same active sets A_t bit for bit), asked to
//      leave |A_t| of every frame beside its [T][K] list of kept product states;
//   2  beam_loss_targets: one workgroup per utterance walks the automaton along the merged target (one thread, n dependent
//      loads), then finds every product state q_k = (y_k, s_k) by binary search over the (state, label) order of the states;
//   3  beam_loss_sets: one workgroup per (frame, utterance) sorts A_t with the forced states F_t of the frame in LDS (bitonic),
//      blanks the duplicates and sorts again: U[t][0 .. nu[t]) ascending;
//   4  beam_loss_fwd: one 1024-thread workgroup per utterance walks the frames with U_{t-1} and its alphas in LDS.  G lanes per
//      target q pull through q's incoming CSR row and find each source in U_{t-1} by binary search in LDS; when the row is
//      longer than |U_{t-1}| (the root of a lexicon trie) they walk U_{t-1} instead and binary-search each kept source in the
//      row.  Max pass, then sum pass; partial results of the G lanes meet in a fixed butterfly.  The alpha of a frame goes to
//      the workspace ([T][M] when a gradient is wanted, else two rows) and comes back into LDS with device-scope loads.
// Backward, two launches: beam_loss_bwd (the mirror image through the outgoing CSR against U_{t+1} in LDS; it owns beta, the
// label posteriors and the posteriors of every stay and edge) and beam_loss_tr_reduce.
// NO FLOAT ATOMICS: posteriors are summed as 64-bit fixed-point integers (integer adds are associative, so the order the
// lanes arrive in cannot change a bit): a frame's label posteriors in LDS with 62 fractional bits (their sum is 1), the
// expected (i, j) counts of an utterance in a [N][N] tile -- in LDS while it fits, else in the utterance's scratch -- with
// 62 - ceil(log2(len)) fractional bits (a cell holds at most len - 1).  The tiles become grad_transition in a last launch that
// adds the utterances in ascending order.  Work and memory per frame follow |U_t| and the edges of the kept states, never Q
// or E (the Q-sized slot arrays are the beam search's own).  Every output, padding row and scratch word that is read is
// written by these kernels: no memset, so both directions can be captured and replayed.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"     // a256, beam_work_layout: the beam search's own part lies at the front of the workspace

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

template <typename U> __device__ __forceinline__ U bl_load(const U *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename U> __device__ __forceinline__ void bl_store(U *p, U v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int bl_len(const int64_t *in_len, int b, int T) {
    if (!in_len) return T;
    const int64_t l = in_len[b];
    return (int) (l < 0 ? 0 : (l > T ? T : l));
}

__device__ __forceinline__ unsigned long long to_fixed(double p, double scale) {
    return p > 0.0 ? (unsigned long long) (p * scale) : 0ull;
}

// position of q in the ascending list a[0 .. n), -1 if absent
__device__ __forceinline__ int find_in(const int *a, int n, int q) {
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

__device__ __forceinline__ int subgroup(int m) {
    int G = 1;
    while (G < 64 && G * 2 * m <= kBL) G *= 2;
    return G;
}

// ---------------------------------------------------------------------------------------------------------------------
// 2: the forced product states q_1 .. q_n of every utterance; hdr[0] = n (0: nothing is forced).
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBS) beam_loss_targets(Problem P, GraphArgs g, BeamLossArgs L, BeamLossLayout lay, char *work) {
    __shared__ int sn, bad;
    const int b = blockIdx.x, tid = threadIdx.x, N = P.N, S = P.S;
    char *wb = work + (size_t) b * lay.per;
    int *hdr = (int *) (wb + lay.hdr), *qk = (int *) (wb + lay.qk);
    long long *key = (long long *) (wb + lay.key);
    const int len = bl_len(P.in_len, b, P.T);
    if (tid == 0) {
        int n = 0;
        if (P.targets && lay.nf > 0) {
            const int64_t l = P.tg_len ? P.tg_len[b] : S;
            const int tl = (int) (l < 0 ? 0 : (l > S ? S : l));
            if (tl >= 1 && tl <= len) {                   // (otherwise the target has no alignment)
                int st = L.start;
                long long prev = -1;
                for (int k = 0; k < tl; ++k) {
                    const long long y = P.targets[(int64_t) b * P.gs0 + (int64_t) k * P.gs1];
                    if (y == prev) continue;
                    const int nx = (y < 0 || y >= N) ? -1 : L.next[(int64_t) st * N + y];
                    if (nx < 0) { n = 0; break; }
                    key[n++] = (long long) nx * N + y;
                    st = nx;
                    prev = y;
                }
            }
        }
        sn = n;
        bad = 0;
    }
    __threadfence();
    __syncthreads();
    const int n = sn, Q = g.Q;
    for (int k = tid; k < n; k += kBS) {
        const long long want = bl_load(key + k);
        int lo = 0, hi = Q;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((long long) g.state[mid] * N + g.label[mid] < want) lo = mid + 1; else hi = mid;
        }
        if (lo >= Q || (long long) g.state[lo] * N + g.label[lo] != want) { atomicOr(&bad, 1); lo = 0; }
        qk[k] = lo;
    }
    __syncthreads();
    if (tid == 0) hdr[0] = bad ? 0 : n;
}

// the automaton must also ACCEPT the target: final_w of the last forced state
template <typename R>
__global__ void __launch_bounds__(64) beam_loss_accept(GraphArgs g, BeamLossLayout lay, char *work, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    char *wb = work + (size_t) b * lay.per;
    int *hdr = (int *) (wb + lay.hdr);
    const int *qk = (const int *) (wb + lay.qk);
    const int n = hdr[0];
    if (n > 0 && !(((const R *) g.final_w)[qk[n - 1]] > Num<R>::ninf())) hdr[0] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// 3: U_t = A_t united with F_t, ascending, without duplicates.  Block (t, b); dynamic LDS: int [P2], P2 a power of two >= M.
// ---------------------------------------------------------------------------------------------------------------------
__device__ void bitonic_sort(int *v, int P2) {
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = threadIdx.x; x < P2; x += kBS) {
                const int y = x ^ j;
                if (y > x) {
                    const int a = v[x], c = v[y];
                    const bool up = (x & k) == 0;
                    if ((a > c) == up) { v[x] = c; v[y] = a; }
                }
            }
            __syncthreads();
        }
}

__global__ void __launch_bounds__(kBS) beam_loss_sets(Problem P, BeamLossLayout lay, int K, int P2, char *work) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int count;
    int *v = (int *) lds;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, T = P.T, M = lay.M;
    char *wb = work + (size_t) b * lay.per;
    int *nu = (int *) (wb + lay.nu);
    const int len = bl_len(P.in_len, b, T);
    if (t >= len) { if (tid == 0) nu[t] = 0; return; }
    const int *bq = (const int *) wb + (int64_t) t * K;                       // the beam search's [T][K] kept states
    const int *qk = (const int *) (wb + lay.qk);
    int na = ((const int *) (wb + lay.cnt))[t];
    na = na < 0 ? 0 : (na > K ? K : na);
    const int n = ((const int *) (wb + lay.hdr))[0];
    // F_t = { q_k : k - 1 <= t and n - k <= len - 1 - t }, k = 1 .. n
    int k0 = n - (len - 1 - t), k1 = t + 1;
    if (k0 < 1) k0 = 1;
    if (k1 > n) k1 = n;
    int nf = k1 >= k0 ? k1 - k0 + 1 : 0;
    if (na + nf > M) nf = M - na;                                               // (cannot happen: n <= lay.nf)
    const int BIG = 0x7FFFFFFF;
    for (int x = tid; x < P2; x += kBS) v[x] = x < na ? bq[x] : (x < na + nf ? qk[k0 - 1 + (x - na)] : BIG);
    if (tid == 0) count = 0;
    __syncthreads();
    bitonic_sort(v, P2);
    // duplicates: flag them in the sign bit (the neighbour's comparison masks it), then blank them and count the rest
    for (int x = tid; x < P2; x += kBS) {
        const int a = v[x] & BIG;
        if (x > 0 && a != BIG && a == (v[x - 1] & BIG)) atomicOr(&v[x], (int) 0x80000000);
    }
    __syncthreads();
    int c = 0;
    for (int x = tid; x < P2; x += kBS) {
        if (v[x] < 0) v[x] = BIG;
        else if (v[x] != BIG) ++c;
    }
    if (c) atomicAdd(&count, c);
    __syncthreads();
    bitonic_sort(v, P2);
    const int m = count;
    int *U = (int *) (wb + lay.U) + (int64_t) t * M;
    for (int x = tid; x < m; x += kBS) U[x] = v[x];
    if (tid == 0) nu[t] = m;
}

// ---------------------------------------------------------------------------------------------------------------------
// 4: alpha over the U_t, and Z_K.  Dynamic LDS: [reduction slots][pq int M][pa R M].
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kBL) beam_loss_fwd(Problem P, GraphArgs g, BeamLossLayout lay, int store, char *work, R *scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    R *red = (R *) lds;
    const int M = lay.M;
    R *pa = (R *) (lds + kBLHead);                       // [M] alpha[t-1] of U_{t-1}
    int *pq = (int *) (pa + M);                          // [M] U_{t-1}
    const int tid = threadIdx.x, b = blockIdx.x, T = P.T;
    const R NINF = Num<R>::ninf();
    const int len = bl_len(P.in_len, b, T);
    if (len < 1) { if (tid == 0) scores[b] = NINF; return; }
    char *wb = work + (size_t) b * lay.per;
    const int *U = (const int *) (wb + lay.U), *nu = (const int *) (wb + lay.nu);
    R *A = (R *) (wb + lay.A);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *trm = (const R *) P.transition;
    const R *sw = (const R *) g.start_w, *fw = (const R *) g.final_w, *ew = (const R *) g.edge_w;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };

    int mp = nu[0];
    for (int x = tid; x < mp; x += kBL) {
        const int q = U[x];
        const R a = sw[q] + in[(int64_t) g.label[q] * P.is2];
        pq[x] = q;
        pa[x] = a;
        if (store) A[x] = a;
    }
    __syncthreads();
    for (int t = 1; t < len; ++t) {
        const int mt = nu[t];
        const int *Ut = U + (int64_t) t * M;
        R *Arow = A + (int64_t) (store ? t : (t & 1)) * M;
        const R *xt = in + (int64_t) t * P.is0;
        const int G = subgroup(mt), per = kBL / G;
        for (int k0 = 0; k0 < mt; k0 += per) {
            const int k = k0 + tid / G, lg = tid % G;
            const bool act = k < mt;
            const int q = act ? Ut[k] : 0;
            const int i = act ? g.label[q] : 0;
            const int e0 = act ? g.row[q] : 0, e1 = act ? g.row[q + 1] : 0;
            const bool by_row = e1 - e0 <= mp;
            // every surviving candidate of q that this lane owns, in ascending source order: f(value)
            auto visit = [&](auto f) {
                if (!act) return;
                if (lg == 0) {
                    const int pos = find_in(pq, mp, q);
                    if (pos >= 0) f(pa[pos] + tr(i, i));
                }
                if (by_row) {
                    for (int e = e0 + lg; e < e1; e += G) {
                        const int pos = find_in(pq, mp, g.src[e]);
                        if (pos >= 0) f((pa[pos] + tr(i, g.src_label[e])) + ew[e]);
                    }
                } else {
                    for (int p = lg; p < mp; p += G) {
                        const int pos = find_in(g.src + e0, e1 - e0, pq[p]);
                        if (pos >= 0) f((pa[p] + tr(i, g.src_label[e0 + pos])) + ew[e0 + pos]);
                    }
                }
            };
            R mx = NINF;
            visit([&](R c) { mx = bmax(mx, c); });
            mx = group_max(mx, G);
            R s = R(0);
            if (mx > NINF) visit([&](R c) { s += bexp(c - mx); });
            s = group_sum(s, G);
            if (act && lg == 0) {
                const R x = mx > NINF ? (mx + blog(s)) + xt[(int64_t) i * P.is2] : NINF;
                bl_store(Arow + k, x);
            }
        }
        __threadfence();
        __syncthreads();
        for (int x = tid; x < mt; x += kBL) { pq[x] = Ut[x]; pa[x] = bl_load(Arow + x); }
        mp = mt;
        __syncthreads();
    }
    R m = NINF;
    for (int x = tid; x < mp; x += kBL) m = bmax(m, pa[x] + fw[pq[x]]);
    m = wg_max(m, red);
    R Z = NINF;
    if (m > NINF) {
        R s = R(0);
        for (int x = tid; x < mp; x += kBL) s += bexp((pa[x] + fw[pq[x]]) - m);
        s = wg_sum(s, red);
        Z = m + blog(s);
    }
    if (tid == 0) scores[b] = Z;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward.  Dynamic LDS: [reduction slots][nb R M][nq int M][gi u64 N][tile u64 N*N if TL].
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int tile_shift(int len) {        // fractional bits of an utterance's (i, j) counts
    int c = 0;
    while ((1 << c) < len && c < 30) ++c;
    return 62 - c;
}

template <typename R, bool TL>
__global__ void __launch_bounds__(kBL) beam_loss_bwd(Problem P, GraphArgs g, BeamGraphArgs bg, BeamLossLayout lay, const char *work,
                                                     const R *Zs, const R *gs, R *gin, char *scratch, size_t sper) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int M = lay.M, N = P.N, T = P.T;
    R *nb = (R *) (lds + kBLHead);                       // [M] beta[t] of U_t
    int *nq = (int *) (nb + M);                          // [M] U_t
    unsigned long long *gi = (unsigned long long *) (lds + kBLHead + (((size_t) M * (sizeof(R) + 4) + 15) & ~(size_t) 15));
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t B = P.B;
    const R NINF = Num<R>::ninf();
    const int len = bl_len(P.in_len, b, T);
    const R Z = Zs[b], gb = gs[b];
    const bool ok = len >= 1 && Z > NINF;
    char *sb = scratch + (size_t) b * sper;
    R *Bv = (R *) sb;                                                          // [2][M]
    unsigned long long *gtile = (unsigned long long *) (sb + ((2 * (size_t) M * sizeof(R) + 255) & ~(size_t) 255));
    unsigned long long *tile = TL ? gi + N : gtile;
    const int t0 = ok ? len : 0;
    for (int64_t x = tid; x < (int64_t) (T - t0) * N; x += kBL) gin[((int64_t) (t0 + x / N) * B + b) * N + x % N] = R(0);
    for (int x = tid; x < N * N; x += kBL) tile[x] = 0ull;
    if (!ok) {
        if (TL) for (int x = tid; x < N * N; x += kBL) gtile[x] = 0ull;
        return;
    }
    for (int x = tid; x < N; x += kBL) gi[x] = 0ull;
    const char *wb = work + (size_t) b * lay.per;
    const int *U = (const int *) (wb + lay.U), *nu = (const int *) (wb + lay.nu);
    const R *A = (const R *) (wb + lay.A);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *trm = (const R *) P.transition;
    const R *fw = (const R *) g.final_w, *ow = (const R *) bg.ow;
    const int2 *oarc = (const int2 *) bg.oarc;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };
    const double tscale = (double) (1ull << tile_shift(len));

    int mt = nu[len - 1];
    for (int x = tid; x < mt; x += kBL) {
        const int q = U[(int64_t) (len - 1) * M + x];
        nq[x] = q;
        nb[x] = fw[q];
    }
    __threadfence();
    __syncthreads();
    for (int t = len - 1; t >= 0; --t) {
        const R *At = A + (int64_t) t * M;
        for (int x = tid; x < mt; x += kBL) {
            const R gam = bexp((At[x] + nb[x]) - Z);
            const unsigned long long f = to_fixed((double) gam, kGammaScale);
            if (f) atomicAdd(&gi[g.label[nq[x]]], f);
        }
        __syncthreads();
        for (int i = tid; i < N; i += kBL) {
            gin[((int64_t) t * B + b) * N + i] = gb * (R) ((double) gi[i] * (1.0 / kGammaScale));
            gi[i] = 0ull;
        }
        if (t == 0) break;
        const int mp = nu[t - 1];
        const int *Up = U + (int64_t) (t - 1) * M;
        const R *Ap = A + (int64_t) (t - 1) * M;
        R *Brow = Bv + (int64_t) ((t - 1) & 1) * M;
        const R *xt = in + (int64_t) t * P.is0;
        const int G = subgroup(mp), per = kBL / G;
        for (int k0 = 0; k0 < mp; k0 += per) {
            const int k = k0 + tid / G, lg = tid % G;
            const bool act = k < mp;
            const int qp = act ? Up[k] : 0;
            const int ip = act ? g.label[qp] : 0;
            const int e0 = act ? bg.orow[qp] : 0, e1 = act ? bg.orow[qp + 1] : 0;
            // every surviving candidate out of qp that this lane owns: f(value, label of the target)
            auto visit = [&](auto f) {
                if (!act) return;
                if (lg == 0) {
                    const int pos = find_in(nq, mt, qp);
                    if (pos >= 0) f((nb[pos] + tr(ip, ip)) + xt[(int64_t) ip * P.is2], ip);
                }
                for (int e = e0 + lg; e < e1; e += G) {
                    const int2 a = oarc[e];
                    const int pos = find_in(nq, mt, a.x);
                    if (pos >= 0) f(((nb[pos] + tr(a.y, ip)) + ow[e]) + xt[(int64_t) a.y * P.is2], a.y);
                }
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
            if (act && lg == 0) bl_store(Brow + k, mx > NINF ? mx + blog(s) : NINF);
        }
        __threadfence();
        __syncthreads();
        for (int x = tid; x < mp; x += kBL) { nq[x] = Up[x]; nb[x] = bl_load(Brow + x); }
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
    const size_t toff = (2 * (size_t) M * sizeof(R) + 255) & ~(size_t) 255;
    for (int b = 0; b < P.B; ++b) {
        const int len = bl_len(P.in_len, b, P.T);
        if (len < 1 || !(Zs[b] > Num<R>::ninf())) continue;
        const unsigned long long v = ((const unsigned long long *) (scratch + (size_t) b * sper + toff))[x];
        s += gs[b] * (R) ((double) v / (double) (1ull << tile_shift(len)));
    }
    gtr[x] = s;
}

inline size_t bwd_lds(int elem, int M, int N, bool tl) {
    return kBLHead + (((size_t) M * (elem + 4) + 15) & ~(size_t) 15) + (size_t) N * 8 + (tl ? (size_t) N * N * 8 : 0);
}

// a launch whose LDS -- dynamic plus the kernel's own `fixed` static bytes -- passes 64 KiB has to ask for it
inline void set_lds(const void *fn, size_t dyn, size_t fixed = 0) {
    if (dyn + fixed > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);
}

}  // namespace

BeamLossLayout beam_loss_layout(int elem, int T, int Q, int K, int cap, int nf, bool store) {
    BeamLossLayout l{};
    l.nf = nf;
    l.M = K + nf;
    size_t off = beam_work_layout(elem, T, Q, K, cap).end;                 // the beam search's own part, at the front
    l.cnt = off; off += a256((size_t) T * 4);
    l.nu = off;  off += a256((size_t) T * 4);
    l.hdr = off; off += 256;
    l.key = off; off += a256((size_t) nf * 8);
    l.qk = off;  off += a256((size_t) nf * 4);
    l.U = off;   off += a256((size_t) T * l.M * 4);
    l.A = off;   off += a256((size_t) (store ? T : 2) * l.M * elem);
    l.per = off;
    return l;
}

// behind the utterances: what the beam search writes besides its sets (scores [B], path / tokens / states [3][B][T], lengths [B])
size_t beam_loss_tail_bytes(int T, int B) { return 2 * a256((size_t) B * 8) + a256((size_t) 3 * B * T * 8); }

size_t beam_loss_work_bytes(int elem, int T, int B, int Q, int K, int cap, int nf, bool store) {
    return (size_t) B * beam_loss_layout(elem, T, Q, K, cap, nf, store).per + beam_loss_tail_bytes(T, B);
}

size_t beam_loss_scratch_per(int elem, int M, int N) { return a256(2 * (size_t) M * elem) + a256((size_t) N * N * 8); }

bool beam_loss_fits(int elem, int M, int N) {
    return kBLHead + (size_t) M * (elem + 4) <= kBLLds && bwd_lds(elem, M, N, false) <= kBLLds;
}

template <typename R>
hipError_t launch_beam_loss_forward(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const BeamLossArgs &L, int K,
                                    double theta, bool store, void *work, void *scores, hipStream_t stream) {
    const int T = P.T, B = P.B;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const int nf = P.targets ? (P.S < T ? P.S : T) : 0;
    const BeamLossLayout lay = beam_loss_layout(sizeof(R), T, G.Q, K, cap, nf, store);
    char *w = (char *) work, *tail = w + (size_t) B * lay.per;
    R *bsc = (R *) tail;
    long long *btl = (long long *) (tail + a256((size_t) B * 8));
    long long *bpa = (long long *) (tail + 2 * a256((size_t) B * 8));
    hipError_t e = launch_beam_graph<R>(P, G, BG, K, theta, work, bsc, bpa, bpa + (size_t) B * T, btl, bpa + 2 * (size_t) B * T,
                                        stream, lay.per, lay.cnt);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beam_loss_targets, dim3(B), dim3(kBS), 0, stream, P, G, L, lay, w);
    hipLaunchKernelGGL((beam_loss_accept<R>), dim3((B + 63) / 64), dim3(64), 0, stream, G, lay, w, B);
    int P2 = 1;
    while (P2 < lay.M) P2 *= 2;
    set_lds((const void *) beam_loss_sets, (size_t) P2 * 4, sizeof(int));    // (M > 8192: 64 KiB of slots beside its `int count`)
    hipLaunchKernelGGL(beam_loss_sets, dim3(T, B), dim3(kBS), (size_t) P2 * 4, stream, P, lay, K, P2, w);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t dyn = kBLHead + (size_t) lay.M * (sizeof(R) + 4);
    set_lds((const void *) beam_loss_fwd<R>, dyn);
    hipLaunchKernelGGL((beam_loss_fwd<R>), dim3(B), dim3(kBL), dyn, stream, P, G, lay, (int) store, w, (R *) scores);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_loss_backward(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, const void *work,
                                     const void *scores, const void *grad_scores, void *grad_inputs, void *grad_transition,
                                     void *scratch, bool accumulate, hipStream_t stream) {
    const int T = P.T, B = P.B, N = P.N;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const int nf = P.targets ? (P.S < T ? P.S : T) : 0;
    const BeamLossLayout lay = beam_loss_layout(sizeof(R), T, G.Q, K, cap, nf, true);
    const size_t sper = beam_loss_scratch_per(sizeof(R), lay.M, N);
    const bool tl = bwd_lds(sizeof(R), lay.M, N, true) <= kBLLds;
    const size_t dyn = bwd_lds(sizeof(R), lay.M, N, tl);
    if (tl) {
        set_lds((const void *) beam_loss_bwd<R, true>, dyn);
        hipLaunchKernelGGL((beam_loss_bwd<R, true>), dim3(B), dim3(kBL), dyn, stream, P, G, BG, lay, (const char *) work,
                           (const R *) scores, (const R *) grad_scores, (R *) grad_inputs, (char *) scratch, sper);
    } else {
        set_lds((const void *) beam_loss_bwd<R, false>, dyn);
        hipLaunchKernelGGL((beam_loss_bwd<R, false>), dim3(B), dim3(kBL), dyn, stream, P, G, BG, lay, (const char *) work,
                           (const R *) scores, (const R *) grad_scores, (R *) grad_inputs, (char *) scratch, sper);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((beam_loss_tr_reduce<R>), dim3((N * N + kBS - 1) / kBS), dim3(kBS), 0, stream, P, lay.M,
                       (const char *) scratch, sper, (const R *) scores, (const R *) grad_scores, (int) accumulate,
                       (R *) grad_transition);
    return hipGetLastError();
}

template hipError_t launch_beam_loss_forward<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const BeamLossArgs &,
                                                    int, double, bool, void *, void *, hipStream_t);
template hipError_t launch_beam_loss_forward<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const BeamLossArgs &,
                                                     int, double, bool, void *, void *, hipStream_t);
template hipError_t launch_beam_loss_backward<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, const void *,
                                                     const void *, const void *, void *, void *, void *, bool, hipStream_t);
template hipError_t launch_beam_loss_backward<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, const void *,
                                                      const void *, const void *, void *, void *, void *, bool, hipStream_t);

}  // namespace asg
