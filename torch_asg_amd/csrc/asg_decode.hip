// torch_asg_amd/csrc/asg_decode.hip -- Viterbi decoding over the FULLY-CONNECTED ASG lattice on gfx950: the best label path
// under the transition matrix, and its tokens (consecutive repeats collapsed).  wav2letter's viterbiPath; a TODO of the
// reference (README.md:33).  The max-plus recursion of the loss's full-lattice alpha chain:
//   v[0][i] = I[0][i];   v[t][i] = (max_j (v[t-1][j] + Tr[i][j])) + I[t][i];   score = max_i v[len-1][i]
//   path[len-1] = argmax_i v[len-1][i];   path[t-1] = argmax_j (v[t-1][j] + Tr[path[t]][j])
// Adds and maxes only (no multiply, so nothing to fuse): every value is exact up to the same roundings as a plain CPU
// restatement in the same dtype, and every argmax takes the SMALLEST index on a tie -- results are bit-identical to it.
//
// Resident route (float N <= 256, double N <= 128): ONE launch, one workgroup per utterance, the transition matrix in VGPRs.
//   Thread (q, i) owns row i and the K slice [q*NP, q*NP + NP) of it (KS slices; KS = 1: one wavefront, no barriers).  The
//   previous frame's vector is broadcast through LDS; only the max is on the serial chain.  The back-pointers of a frame
//   (uint8, work[b][t][N]) are the first index of the max in each slice, reduced over the slices one frame LATER (the read
//   sits behind the next frame's barrier).  Then the same workgroup backtraces 64 frames at a time from LDS copies of the
//   back-pointer rows and collapses the path into tokens (ballot + popcount per 64-frame block).
// Streaming route (larger alphabets): one launch per frame of a max-plus "GEMM"  V_t[B,N] = maxplus(V_{t-1}, Tr^T) + I_t.
//   A workgroup takes 64 rows x UB utterances; its eight wavefronts split K and meet in LDS.  Only the V_t values are
//   stored (work: Tr^T padded with -inf, then V[T][B][PAD]); the backtrace kernel recomputes the argmax of the ONE row on
//   the path at each frame with the same additions, and writes path, tokens and token lengths.
#include "asg_common.h"
#include "asg_kernels.h"

namespace asg {

namespace {

__device__ __forceinline__ float vmax(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double vmax(double a, double b) { return fmax(a, b); }

__device__ __forceinline__ int clamp_len(const int64_t *in_len, int b, int T) {
    if (!in_len) return T;
    const int64_t l = in_len[b];
    return (int) (l < 0 ? 0 : (l > T ? T : l));
}

// (value, index) argmax across a wavefront: larger value wins, the smaller index on a tie.  Result in every lane.
template <typename R>
__device__ __forceinline__ void wave_argmax(R &v, int &j) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const R ov = __shfl_xor(v, o);
        const int oj = __shfl_xor(j, o);
        if (ov > v || (ov == v && oj < j)) { v = ov; j = oj; }
    }
}

// One wavefront: tokens[0..T) of one utterance from its finished path[0..len) in device memory (made visible by the caller),
// -1 behind them, and the token count.  Per 64-frame block: keep = (label differs from the previous frame's), ballot, popcount.
__device__ void collapse_tokens(const long long *pb, int len, int T, long long *tk, long long *tl, int lane) {
    int base = 0;
    long long carry = -1;                       // label of the frame before the block
    for (int c0 = 0; c0 < len; c0 += 64) {
        const int t = c0 + lane;
        const long long cur = t < len ? __builtin_nontemporal_load(pb + t) : -1;
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

// ---------------------------------------------------------------------------------------------------------------------
// Resident route.  KS slices of NP columns; rows RW = 64 * KS (threads = KS * RW).  KS = 1: N <= NP <= 64.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kEPFMax = 8;     // emission prefetch depth (frames)
constexpr int kBTF = 64;       // backtrace block (frames)

template <typename R, int NP, int KS>
__global__ void __launch_bounds__(64 * KS * KS) decode_resident_kernel(Problem P, unsigned char *bp, R *scores, long long *path,
                                                                      long long *tokens, long long *tlen) {
    constexpr int RW = 64 * KS, NT = RW * KS;
    constexpr bool KEEP = KS == 1 && sizeof(R) * NP <= 256;
    constexpr int kEPF = kEPFMax;
    __shared__ R vbuf[2][RW];
    __shared__ R part[KS > 1 ? KS : 1][RW];
    __shared__ unsigned short bpart[KS > 1 ? KS : 1][RW];
    __shared__ unsigned char stage[kBTF][RW];
    __shared__ int pth[kBTF];
    __shared__ R best_sh;
    __shared__ int arg_sh;
    const int tid = threadIdx.x, lane = tid & 63;
    const int q = tid / RW, i = tid % RW;
    const int b = blockIdx.x;
    const int T = P.T, N = P.N;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    long long *pb = path + (int64_t) b * T;
    long long *tk = tokens + (int64_t) b * T;
    unsigned char *bpb = bp + (int64_t) b * T * N;
    const R *tr = (const R *) P.transition;
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1 + (int64_t) (i < N ? i : 0) * P.is2;
    // KS > 1 (up to 1024 threads, 128 VGPRs each): only the threads that own a row's emission load it
    const bool ld = KS == 1 || (q == 0 && i < N);

    // this thread's slice of row i of the transition matrix (-inf outside the alphabet: never the max of a real row)
    R trr[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int j = q * NP + k;
        trr[k] = (i < N && j < N) ? tr[(int64_t) i * P.ts0 + (int64_t) j * P.ts1] : NINF;
    }
    // one wavefront: the emission loads are unconditional (rows past the alphabet read row 0, frames past the utterance its
    // last frame): no branches around them, so the waits for the prefetch ring stay counted instead of draining every load
    const R e0 = in[0];
    if (len >= 1 && q == 0) vbuf[1][i] = i < N ? e0 : NINF;
    R ring[kEPF];
#pragma unroll
    for (int k = 0; k < kEPF; ++k) ring[k] = ld ? in[(int64_t) min(1 + k, max(len - 1, 0)) * P.is0] : R(0);
    if (KS > 1) __syncthreads(); else __builtin_amdgcn_wave_barrier();

    for (int t0 = 1; t0 < len; t0 += kEPF) {
        R nxt[kEPF];
#pragma unroll
        for (int k = 0; k < kEPF; ++k)
            nxt[k] = ld ? in[(int64_t) min(t0 + kEPF + k, len - 1) * P.is0] : R(0);
#pragma unroll
        for (int f = 0; f < kEPF; ++f) {
            const int t = t0 + f;
            if (t < len) {                                          // uniform
                const R *vp = vbuf[t & 1] + q * NP;
                // the serial chain: the candidates into two max3 chains.  KEEP: the candidates stay in VGPRs for the
                // back-pointer; otherwise they are formed again from the same LDS line (no room next to the matrix), and the
                // broadcast reads are issued in groups of four so that they do not all wait in VGPRs at once.
                R c[KEEP ? NP : 4];
                R m0 = NINF, m1 = NINF;
#pragma unroll
                for (int k = 0; k < NP; k += 4) {
                    if (!KEEP && k % 16 == 0) __builtin_amdgcn_sched_barrier(0);
                    const V4<R> v4 = *reinterpret_cast<const V4<R> *>(vp + k);
                    const int o = KEEP ? k : 0;
                    c[o] = v4.x + trr[k]; c[o + 1] = v4.y + trr[k + 1]; c[o + 2] = v4.z + trr[k + 2]; c[o + 3] = v4.w + trr[k + 3];
                    m0 = vmax(vmax(m0, c[o]), c[o + 1]);
                    m1 = vmax(vmax(m1, c[o + 2]), c[o + 3]);
                }
                R m = vmax(m0, m1);
                if constexpr (KS > 1) {
                    part[q][i] = m;
                    // back-pointers of the PREVIOUS frame: its slices' first indices are complete (barrier at the top of this frame)
                    if (q == 0 && t >= 2 && i < N) {
                        int best = bpart[0][i];
#pragma unroll
                        for (int s = 1; s < KS; ++s) best = min(best, (int) bpart[s][i]);
                        bpb[(int64_t) (t - 1) * N + i] = (unsigned char) best;
                    }
                    __syncthreads();
#pragma unroll
                    for (int s = 0; s < KS; ++s) m = vmax(m, part[s][i]);
                }
                const R vn = m + (i < N ? ring[f] : R(0));
                if (q == 0) vbuf[(t + 1) & 1][i] = vn;
                // first index of the max in this slice.  Nothing of the next frame depends on it, but with KS = 1 it sits in
                // the same wavefront's instruction stream between this frame's max and the next broadcast, so it adds its
                // ~2 x NP VALU instructions to every frame; with KS > 1 the other slices' waves overlap it
                int k1 = 0xFFFF;
                if constexpr (!KEEP) {
#pragma unroll
                    for (int k = NP - 4; k >= 0; k -= 4) {
                        const V4<R> v4 = *reinterpret_cast<const V4<R> *>(vp + k);
                        k1 = (v4.w + trr[k + 3] == m) ? q * NP + k + 3 : k1;
                        k1 = (v4.z + trr[k + 2] == m) ? q * NP + k + 2 : k1;
                        k1 = (v4.y + trr[k + 1] == m) ? q * NP + k + 1 : k1;
                        k1 = (v4.x + trr[k] == m) ? q * NP + k : k1;
                    }
                } else {
#pragma unroll
                    for (int k = NP - 1; k >= 0; --k) k1 = (c[k] == m) ? k : k1;
                }
                if constexpr (KS > 1) {
                    bpart[q][i] = (unsigned short) k1;
                    __syncthreads();
                } else {
                    if (i < N) bpb[(int64_t) t * N + i] = (unsigned char) k1;
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kEPF; ++k) ring[k] = nxt[k];
    }
    if constexpr (KS > 1) {
        if (q == 0 && len >= 2 && i < N) {
            int best = bpart[0][i];
#pragma unroll
            for (int s = 1; s < KS; ++s) best = min(best, (int) bpart[s][i]);
            bpb[(int64_t) (len - 1) * N + i] = (unsigned char) best;
        }
    }
    // ---- score: first index of the max of v[len-1] (in vbuf[len & 1])
    if (tid < 64) {
        R bv = NINF;
        int bj = 0x7FFFFFFF;
        if (len >= 1) {
            for (int j = lane; j < N; j += 64) {
                const R x = vbuf[len & 1][j];
                if (x > bv || bj == 0x7FFFFFFF) { bv = x; bj = j; }
            }
        }
        wave_argmax(bv, bj);
        if (lane == 0) { best_sh = bv; arg_sh = bj; }
    }
    __threadfence();                 // the back-pointer stores of every wavefront, visible to the loads below
    __syncthreads();
    const R best = best_sh;
    if (len < 1 || !(best > NINF) || best != best) {                // nothing to decode, or no finite path
        for (int t = tid; t < T; t += NT) { pb[t] = -1; tk[t] = -1; }
        if (tid == 0) { scores[b] = NINF; tlen[b] = 0; }
        return;
    }
    if (tid == 0) scores[b] = best;
    for (int t = len + tid; t < T; t += NT) pb[t] = -1;
    // ---- backtrace, kBTF frames at a time: the block's back-pointer rows (contiguous in work) go to LDS with coalesced
    // loads, one thread walks them, everyone stores the labels
    int s = arg_sh;
    for (int c0 = ((len - 1) / kBTF) * kBTF; c0 >= 0; c0 -= kBTF) {
        const int nf = min(kBTF, len - c0);
        const unsigned char *src = bpb + (int64_t) c0 * N;
        for (int x = tid; x < nf * N; x += NT) stage[x / N][x % N] = __builtin_nontemporal_load(src + x);
        __syncthreads();
        if (tid == 0) {
            for (int f = nf - 1; f >= 0; --f) {
                pth[f] = s;
                if (c0 + f >= 1) s = min((int) stage[f][s], N - 1);
            }
        }
        __syncthreads();
        if (tid < nf) pb[c0 + tid] = pth[tid];
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    if (tid < 64) collapse_tokens(pb, len, T, tk, tlen + b, lane);
}

// ---------------------------------------------------------------------------------------------------------------------
// Streaming route.
// ---------------------------------------------------------------------------------------------------------------------
// trT[k][i] = Tr[i][k] for k, i < N; -inf in the padding up to PAD (a multiple of 64).
template <typename R>
__global__ void __launch_bounds__(256) decode_transpose_kernel(Problem P, R *trT, int PAD) {
    __shared__ R tile[64][65];
    const int i0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const R *tr = (const R *) P.transition;
    const R NINF = Num<R>::ninf();
    for (int r = ty; r < 64; r += 4) {               // row i0 + r, column k0 + tx
        const int i = i0 + r, k = k0 + tx;
        tile[r][tx] = (i < P.N && k < P.N) ? tr[(int64_t) i * P.ts0 + (int64_t) k * P.ts1] : NINF;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) trT[(int64_t) (k0 + r) * PAD + i0 + tx] = tile[tx][r];
}

constexpr int kSW = 8;         // wavefronts per frame workgroup (the K split)

// Frame t of all utterances: V[t][b][i] for 64 rows x UB utterances per workgroup.  V[t][b][i] for i in [N, PAD) is -inf.
template <typename R, int UB>
__global__ void __launch_bounds__(64 * kSW) decode_frame_kernel(Problem P, const R *__restrict__ trT, const R *__restrict__ Vp,
                                                                 R *__restrict__ Vt, int t, int PAD, int nrt, int ngr) {
    __shared__ R red[kSW][UB][64];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (uniform: V is read with s_load)
    // blocks that share a row tile are 8 apart (same XCD under round-robin placement: the tile is read from one L2)
    const int id = blockIdx.x;
    const int hi = id / (8 * ngr), rem = id % (8 * ngr);
    const int g = rem / 8, rt = hi * 8 + rem % 8;
    if (rt >= nrt) return;
    const int i = rt * 64 + lane;
    const int B = P.B, N = P.N;
    const R NINF = Num<R>::ninf();
    const R *in = (const R *) P.inputs;
    if (t == 0) {
        for (int u = w; u < UB; u += kSW) {
            const int bb = g * UB + u;
            if (bb < B) Vt[(int64_t) bb * PAD + i] = i < N ? in[(int64_t) bb * P.is1 + (int64_t) i * P.is2] : NINF;
        }
        return;
    }
    R acc[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) acc[u] = NINF;
    const int KC = PAD / kSW;                         // a multiple of 8
    const int k0 = w * KC;
    for (int k = k0; k < k0 + KC; k += 4) {
        R tv[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) tv[x] = trT[(int64_t) (k + x) * PAD + i];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int bb = min(g * UB + u, B - 1);
            const V4<R> v4 = *reinterpret_cast<const V4<R> *>(Vp + (int64_t) bb * PAD + k);      // wave-uniform
            acc[u] = vmax(vmax(acc[u], v4.x + tv[0]), v4.y + tv[1]);
            acc[u] = vmax(vmax(acc[u], v4.z + tv[2]), v4.w + tv[3]);
        }
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) red[w][u][lane] = acc[u];
    __syncthreads();
    for (int u = w; u < UB; u += kSW) {
        const int bb = g * UB + u;
        if (bb >= B) continue;
        R m = red[0][u][lane];
#pragma unroll
        for (int s = 1; s < kSW; ++s) m = vmax(m, red[s][u][lane]);
        R *dst = Vt + (int64_t) bb * PAD + i;
        *dst = i < N ? m + in[(int64_t) t * P.is0 + (int64_t) bb * P.is1 + (int64_t) i * P.is2] : NINF;
    }
}

constexpr int kBT = 256;       // backtrace workgroup

// (value, index) argmax across the workgroup; result in every thread.  red_v / red_j: kBT / 64 slots.
template <typename R>
__device__ __forceinline__ void block_argmax(R &v, int &j, R *red_v, int *red_j) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    wave_argmax(v, j);
    if (lane == 0) { red_v[w] = v; red_j[w] = j; }
    __syncthreads();
    v = red_v[0]; j = red_j[0];
#pragma unroll
    for (int s = 1; s < kBT / 64; ++s) {
        const R ov = red_v[s];
        const int oj = red_j[s];
        if (ov > v || (ov == v && oj < j)) { v = ov; j = oj; }
    }
    __syncthreads();
}

template <typename R>
__global__ void __launch_bounds__(kBT) decode_backtrace_kernel(Problem P, const R *V, int PAD, R *scores, long long *path,
                                                               long long *tokens, long long *tlen) {
    __shared__ R red_v[kBT / 64];
    __shared__ int red_j[kBT / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int b = blockIdx.x;
    const int T = P.T, B = P.B, N = P.N;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    long long *pb = path + (int64_t) b * T;
    long long *tk = tokens + (int64_t) b * T;
    const R *tr = (const R *) P.transition;
    R best = NINF;
    int s = 0x7FFFFFFF;
    if (len >= 1) {
        const R *row = V + ((int64_t) (len - 1) * B + b) * PAD;
        for (int j = tid; j < N; j += kBT) {
            const R x = row[j];
            if (x > best || s == 0x7FFFFFFF) { best = x; s = j; }
        }
    }
    block_argmax(best, s, red_v, red_j);
    if (len < 1 || !(best > NINF) || best != best) {
        for (int t = tid; t < T; t += kBT) { pb[t] = -1; tk[t] = -1; }
        if (tid == 0) { scores[b] = NINF; tlen[b] = 0; }
        return;
    }
    if (tid == 0) { scores[b] = best; pb[len - 1] = s; }
    for (int t = len + tid; t < T; t += kBT) pb[t] = -1;
    for (int t = len - 1; t >= 1; --t) {
        const R *row = V + ((int64_t) (t - 1) * B + b) * PAD;
        const R *trow = tr + (int64_t) s * P.ts0;
        R v = NINF;
        int j1 = 0x7FFFFFFF;
        for (int j = tid; j < N; j += kBT) {
            const R x = row[j] + trow[(int64_t) j * P.ts1];              // the forward kernel's addition, bit for bit
            if (x > v || j1 == 0x7FFFFFFF) { v = x; j1 = j; }
        }
        block_argmax(v, j1, red_v, red_j);
        s = min(j1, N - 1);                 // (only NaN emissions leave no index: they are unspecified, never out of bounds)
        if (tid == 0) pb[t - 1] = s;
    }
    __threadfence();
    __syncthreads();
    if (tid < 64) collapse_tokens(pb, len, T, tk, tlen + b, lane);
}

inline int pad64(int n) { return (n + 63) / 64 * 64; }

}  // namespace

bool decode_resident(int elem, int N) { return N <= (elem == 8 ? 128 : 256); }

size_t decode_work_bytes(int elem, int T, int B, int N) {
    if (decode_resident(elem, N)) return (size_t) B * T * N;
    const size_t pad = (size_t) pad64(N);
    return (pad * pad * elem + 255) / 256 * 256 + (size_t) T * B * pad * elem;
}

template <typename R>
hipError_t launch_decode(const Problem &P, void *work, void *scores, long long *path, long long *tokens, long long *tlen,
                         hipStream_t stream) {
    const int N = P.N;
    if (decode_resident(sizeof(R), N)) {
        unsigned char *bp = (unsigned char *) work;
#define ASG_DECODE_RES(NP, KS)                                                                                              \
    hipLaunchKernelGGL((decode_resident_kernel<R, NP, KS>), dim3(P.B), dim3(64 * KS * KS), 0, stream, P, bp, (R *) scores,  \
                       path, tokens, tlen)
        // one wavefront: the slice is the alphabet rounded up to 8 (every padded column is a candidate on the chain)
        if (N <= 8) ASG_DECODE_RES(8, 1);
        else if (N <= 16) ASG_DECODE_RES(16, 1);
        else if (N <= 24) ASG_DECODE_RES(24, 1);
        else if (N <= 32) ASG_DECODE_RES(32, 1);
        else if (N <= 40) ASG_DECODE_RES(40, 1);
        else if (N <= 48) ASG_DECODE_RES(48, 1);
        else if (N <= 56) ASG_DECODE_RES(56, 1);
        else if (N <= 64) ASG_DECODE_RES(64, 1);
        else if (N <= 128) ASG_DECODE_RES(64, 2);
        else if constexpr (sizeof(R) == 4) ASG_DECODE_RES(64, 4);
#undef ASG_DECODE_RES
        return hipGetLastError();
    }
    const int PAD = pad64(N);
    R *trT = (R *) work;
    R *V = (R *) ((char *) work + ((size_t) PAD * PAD * sizeof(R) + 255) / 256 * 256);
    hipLaunchKernelGGL((decode_transpose_kernel<R>), dim3(PAD / 64, PAD / 64), dim3(256), 0, stream, P, trT, PAD);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int nrt = PAD / 64;
    // utterances per workgroup: float32 4 / 8 / 16 by batch; float64 always 8 (its LDS partials at 16 would take 64 KiB)
    const int UB = sizeof(R) == 8 ? 8 : (P.B <= 4 ? 4 : (P.B <= 8 ? 8 : 16));
    const int ngr = (P.B + UB - 1) / UB;
    const int nblk = (nrt + 7) / 8 * 8 * ngr;
    for (int t = 0; t < P.T; ++t) {
        const R *Vp = V + (size_t) (t > 0 ? t - 1 : 0) * P.B * PAD;      // V[t-1] (not read at t = 0)
        R *Vt = V + (size_t) t * P.B * PAD;
        if constexpr (sizeof(R) == 8) {
            hipLaunchKernelGGL((decode_frame_kernel<R, 8>), dim3(nblk), dim3(64 * kSW), 0, stream, P, trT, Vp, Vt, t, PAD, nrt, ngr);
        } else {
            if (UB == 4)
                hipLaunchKernelGGL((decode_frame_kernel<R, 4>), dim3(nblk), dim3(64 * kSW), 0, stream, P, trT, Vp, Vt, t, PAD, nrt, ngr);
            else if (UB == 8)
                hipLaunchKernelGGL((decode_frame_kernel<R, 8>), dim3(nblk), dim3(64 * kSW), 0, stream, P, trT, Vp, Vt, t, PAD, nrt, ngr);
            else
                hipLaunchKernelGGL((decode_frame_kernel<R, 16>), dim3(nblk), dim3(64 * kSW), 0, stream, P, trT, Vp, Vt, t, PAD, nrt, ngr);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((decode_backtrace_kernel<R>), dim3(P.B), dim3(kBT), 0, stream, P, (const R *) V, PAD, (R *) scores, path,
                       tokens, tlen);
    return hipGetLastError();
}
template hipError_t launch_decode<float>(const Problem &, void *, void *, long long *, long long *, long long *, hipStream_t);
template hipError_t launch_decode<double>(const Problem &, void *, void *, long long *, long long *, long long *, hipStream_t);

}  // namespace asg
