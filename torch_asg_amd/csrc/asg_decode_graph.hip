// torch_asg_amd/csrc/asg_decode_graph.hip -- exact Viterbi decoding over the ASG lattice COMPOSED with a deterministic
// weighted automaton over tokens (a token-level language model), on gfx950.  The product graph is compiled on the host
// (torch_asg_amd/graph.py): Q product states q = (label i, automaton state s'), sorted by (s', i), and per target q a CSR row
// of incoming edges q' = (j, s) -> q (j != i), ascending by source, each carrying the folded arc weight arcw[s][i].
//   v[0][q] = start_w[q] + I[0][i]
//   v[t][q] = best(stay: v[t-1][q] + Tr[i][i];  edge q' -> q: (v[t-1][q'] + Tr[i][j]) + arcw) + I[t][i]
//   score   = max_q (v[len-1][q] + final_w[q]);  backtrace through the winners' source indices.
// "best" is the largest value; on a tie the SMALLEST SOURCE INDEX (the stay's source is q itself).  Adds and maxes only, in
// the dtype of the problem: results are bit-identical to the numpy restatement (tests/graph_decode_ref.py), and with a
// one-state automaton to asg_decode.hip.
//
// Resident route (graph_decode_resident: both Viterbi vectors and the frame's emissions in LDS, N <= 1024, E <= 32768; or
// wherever it fits with ASG_FLAG_DECODE_GRAPH_RESIDENT): ONE launch, one
// 1024-thread workgroup per utterance.  Each frame, subgroups of G lanes take one target each: the stay in lane 0, the CSR row
// strided over the lanes (coalesced loads of the edge arrays from L2, which every utterance shares), then a (value, source)
// reduction over the subgroup.  The transition matrix sits in LDS when it fits.  Back-pointers (int32 source indices) go to
// work[b][t][Q]; a barrier separates frames.  The final argmax, the backtrace (back-pointer rows staged through LDS, up to
// 64 frames at a time) and the token collapse follow in the same launch.
// Streaming route (larger graphs, or ASG_FLAG_DECODE_GRAPH_STREAMING): one launch per frame; a wavefront takes one target
// and 64 utterances (lanes), so the edge arrays are read with wave-uniform loads and the Viterbi vectors, ping-ponged in
// global memory as [2][Q][B], with coalesced ones.  Back-pointers go to work[t][Q][B].  A last launch per utterance takes the
// argmax, walks the back-pointers and collapses the tokens.  No grid-wide waits: the per-frame launches are what order the
// frames, so the route is capturable and assumes no co-residency.
#include "asg_common.h"
#include "asg_kernels.h"

namespace asg {

namespace {

constexpr int kRT = 1024;        // resident workgroup
constexpr int kScratch = 512;    // resident LDS bytes in front of the vectors: reduction slots + the backtrace's frame labels
constexpr int kStageF = 64;      // backtrace frames staged at a time (at most)
constexpr int kFT = 256;         // streaming frame / finish workgroups

__device__ __forceinline__ int clamp_len(const int64_t *in_len, int b, int T) {
    if (!in_len) return T;
    const int64_t l = in_len[b];
    return (int) (l < 0 ? 0 : (l > T ? T : l));
}

// The candidate comparator: the larger value wins, the smaller source index on a tie.
template <typename R>
__device__ __forceinline__ void take(R &bv, int &bs, R c, int s) {
    if (c > bv || (c == bv && s < bs)) { bv = c; bs = s; }
}

// (value, index) argmax over the workgroup (blockDim.x = NT); result in every thread.  rv / rj: NT / 64 slots.
template <typename R, int NT>
__device__ __forceinline__ void block_argmax(R &v, int &j, R *rv, int *rj) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) take(v, j, (R) __shfl_xor(v, o), __shfl_xor(j, o));
    if (lane == 0) { rv[w] = v; rj[w] = j; }
    __syncthreads();
    v = rv[0]; j = rj[0];
#pragma unroll
    for (int s = 1; s < NT / 64; ++s) take(v, j, rv[s], rj[s]);
    __syncthreads();
}

// One wavefront: tokens[0..T) of one utterance from its finished path[0..len) in device memory (made visible by the caller),
// -1 behind them, and the token count (the convention of asg_decode.hip's collapse_tokens).
__device__ void collapse_tokens(const long long *pb, int len, int T, long long *tk, long long *tl, int lane) {
    int base = 0;
    long long carry = -1;                       // label of the frame before the block
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

// No path (len == 0, or no finite score): score -inf, everything -1, no tokens.
template <typename R>
__device__ void write_no_path(int b, int T, int NT, R *scores, long long *pb, long long *tk, long long *st, long long *tlen) {
    for (int t = threadIdx.x; t < T; t += NT) { pb[t] = -1; tk[t] = -1; st[t] = -1; }
    if (threadIdx.x == 0) { scores[b] = Num<R>::ninf(); tlen[b] = 0; }
}

// ---------------------------------------------------------------------------------------------------------------------
// Resident route.  Dynamic LDS: [scratch 512 B][v 2*Q][em 2*N][tr N*N if TRL]; after the forward pass the region behind the
// scratch holds the staged back-pointer rows (F frames of Q int32).
// ---------------------------------------------------------------------------------------------------------------------
template <typename R, int G, bool TRL>
__global__ void __launch_bounds__(kRT) graph_resident_kernel(Problem P, GraphArgs g, int *bp, int F, R *scores, long long *path,
                                                             long long *tokens, long long *tlen, long long *states) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    R *red_v = (R *) lds;                                  // [16]
    int *red_j = (int *) (lds + 16 * sizeof(R));           // [16]
    int *pth = (int *) (lds + 256);                        // [kStageF]
    R *v = (R *) (lds + kScratch);                         // [2][Q]
    const int Q = g.Q, N = P.N, T = P.T;
    R *em = v + 2 * (int64_t) Q;                           // [2][N]
    R *trs = em + 2 * N;                                   // [N][N]
    int *stage = (int *) (lds + kScratch);                 // [F][Q] (after the forward pass)
    const int tid = threadIdx.x, b = blockIdx.x;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *tr = (const R *) P.transition;
    const R *sw = (const R *) g.start_w, *fw = (const R *) g.final_w, *ew = (const R *) g.edge_w;
    int *bpb = bp + (int64_t) b * T * Q;
    long long *pb = path + (int64_t) b * T, *tk = tokens + (int64_t) b * T, *st = states + (int64_t) b * T;
    auto TR = [&](int i, int j) -> R {
        if constexpr (TRL) return trs[i * N + j];
        else return tr[(int64_t) i * P.ts0 + (int64_t) j * P.ts1];
    };

    if constexpr (TRL)
        for (int x = tid; x < N * N; x += kRT) trs[x] = tr[(int64_t) (x / N) * P.ts0 + (int64_t) (x % N) * P.ts1];
    if (len >= 1) {
        for (int q = tid; q < Q; q += kRT) v[q] = sw[q] + in[(int64_t) g.label[q] * P.is2];
        if (len >= 2 && tid < N) em[N + tid] = in[P.is0 + (int64_t) tid * P.is2];
    }
    __syncthreads();

    const int sub = tid / G, lg = tid % G;
    for (int t = 1; t < len; ++t) {
        const R *vp = v + (int64_t) ((t - 1) & 1) * Q;
        R *vn = v + (int64_t) (t & 1) * Q;
        const R *et = em + (t & 1) * N;
        // the next frame's emissions: loaded now, stored into the other buffer (read last at frame t-1) behind the compute
        const bool pre = t + 1 < len && tid < N;
        R nx = R(0);
        if (pre) nx = in[(int64_t) (t + 1) * P.is0 + (int64_t) tid * P.is2];
        int *bpt = bpb + (int64_t) t * Q;
        // a subgroup's lanes share q: they enter and leave the loop together, so the shuffles below see only active lanes
        for (int q = sub; q < Q; q += kRT / G) {
            const int i = g.label[q];
            const int e0 = g.row[q], e1 = g.row[q + 1];
            R bv = NINF;
            int bs = 0x7FFFFFFF;
            if (lg == 0) { bv = vp[q] + TR(i, i); bs = q; }
#pragma unroll 4
            for (int e = e0 + lg; e < e1; e += G) {
                const int s = g.src[e];
                const R c = (vp[s] + TR(i, g.src_label[e])) + ew[e];
                take(bv, bs, c, s);
            }
#pragma unroll
            for (int o = 1; o < G; o <<= 1) take(bv, bs, (R) __shfl_xor(bv, o), __shfl_xor(bs, o));
            if (lg == 0) { vn[q] = bv + et[i]; bpt[q] = bs; }
        }
        if (pre) em[((t + 1) & 1) * N + tid] = nx;
        __syncthreads();
    }

    // ---- score: first q of the max of v[len-1][q] + final_w[q]
    R best = NINF;
    int bq = 0x7FFFFFFF;
    if (len >= 1) {
        const R *vl = v + (int64_t) ((len - 1) & 1) * Q;
        for (int q = tid; q < Q; q += kRT) take(best, bq, vl[q] + fw[q], q);
    }
    block_argmax<R, kRT>(best, bq, red_v, red_j);
    if (len < 1 || !(best > NINF) || best != best) {
        write_no_path(b, T, kRT, scores, pb, tk, st, tlen);
        return;
    }
    if (tid == 0) scores[b] = best;
    for (int t = len + tid; t < T; t += kRT) { pb[t] = -1; st[t] = -1; }
    __threadfence();                 // the back-pointer stores of every wavefront, visible to the loads below
    __syncthreads();
    // ---- backtrace, F frames at a time: the block's back-pointer rows (contiguous in work) go to LDS with coalesced loads,
    // one thread walks them, everyone stores the labels and states
    int q = bq;
    for (int c0 = ((len - 1) / F) * F; c0 >= 0; c0 -= F) {
        const int nf = min(F, len - c0);
        const int *srcp = bpb + (int64_t) c0 * Q;
        for (int x = tid; x < nf * Q; x += kRT) stage[x] = srcp[x];
        __syncthreads();
        if (tid == 0) {
            for (int f = nf - 1; f >= 0; --f) {
                pth[f] = q;
                if (c0 + f >= 1) q = stage[f * Q + q];
            }
        }
        __syncthreads();
        if (tid < nf) { const int qq = pth[tid]; pb[c0 + tid] = g.label[qq]; st[c0 + tid] = g.state[qq]; }
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    if (tid < 64) collapse_tokens(pb, len, T, tk, tlen + b, tid);
}

// ---------------------------------------------------------------------------------------------------------------------
// Streaming route.
// ---------------------------------------------------------------------------------------------------------------------
// Frame t: wavefront w of block x takes target q = 4x + w, lane l utterance b = 64y + l.  V: [2][Q][B]; bp: [T][Q][B].
template <typename R>
__global__ void __launch_bounds__(kFT) graph_frame_kernel(Problem P, GraphArgs g, int *bp, const R *__restrict__ Vp,
                                                          R *__restrict__ Vt, int t) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int q = blockIdx.x * (kFT / 64) + w;
    const int b = blockIdx.y * 64 + lane;
    const int Q = g.Q, B = P.B;
    if (q >= Q || b >= B || t >= clamp_len(P.in_len, b, P.T)) return;
    const int i = g.label[q];
    const R x = ((const R *) P.inputs)[(int64_t) t * P.is0 + (int64_t) b * P.is1 + (int64_t) i * P.is2];
    if (t == 0) {
        Vt[(int64_t) q * B + b] = ((const R *) g.start_w)[q] + x;
        return;
    }
    const R *tr = (const R *) P.transition, *ew = (const R *) g.edge_w;
    const R *tri = tr + (int64_t) i * P.ts0;
    R bv = Vp[(int64_t) q * B + b] + tri[(int64_t) i * P.ts1];
    int bs = q;
    const int e0 = g.row[q], e1 = g.row[q + 1];
#pragma unroll 4
    for (int e = e0; e < e1; ++e) {
        const int s = g.src[e];
        const R c = (Vp[(int64_t) s * B + b] + tri[(int64_t) g.src_label[e] * P.ts1]) + ew[e];
        take(bv, bs, c, s);
    }
    Vt[(int64_t) q * B + b] = bv + x;
    bp[((int64_t) t * Q + q) * B + b] = bs;
}

template <typename R>
__global__ void __launch_bounds__(kFT) graph_finish_kernel(Problem P, GraphArgs g, const int *bp, const R *V, R *scores,
                                                           long long *path, long long *tokens, long long *tlen,
                                                           long long *states) {
    __shared__ R red_v[kFT / 64];
    __shared__ int red_j[kFT / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Q = g.Q, B = P.B, T = P.T;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    const R *fw = (const R *) g.final_w;
    long long *pb = path + (int64_t) b * T, *tk = tokens + (int64_t) b * T, *st = states + (int64_t) b * T;
    R best = NINF;
    int bq = 0x7FFFFFFF;
    if (len >= 1) {
        const R *vl = V + (int64_t) ((len - 1) & 1) * Q * B + b;
        for (int q = tid; q < Q; q += kFT) take(best, bq, vl[(int64_t) q * B] + fw[q], q);
    }
    block_argmax<R, kFT>(best, bq, red_v, red_j);
    if (len < 1 || !(best > NINF) || best != best) {
        write_no_path(b, T, kFT, scores, pb, tk, st, tlen);
        return;
    }
    if (tid == 0) {
        scores[b] = best;
        int q = bq;
        for (int t = len - 1; t >= 0; --t) {
            pb[t] = g.label[q];
            st[t] = g.state[q];
            if (t >= 1) q = bp[((int64_t) t * Q + q) * B + b];
        }
    }
    for (int t = len + tid; t < T; t += kFT) { pb[t] = -1; st[t] = -1; }
    __threadfence();
    __syncthreads();
    if (tid < 64) collapse_tokens(pb, len, T, tk, tlen + b, tid);
}

inline size_t resident_lds(int elem, int N, int Q, bool with_tr) {
    return kScratch + (2 * (size_t) Q + 2 * (size_t) N + (with_tr ? (size_t) N * N : 0)) * elem;
}
constexpr size_t kResidentVec = 128 * 1024;     // the two Viterbi vectors + emissions, at most
constexpr size_t kLdsMax = 160 * 1024;
// Edges per frame above which the streaming route wins although the graph fits: the resident route walks every edge of an
// utterance on one CU (~0.5 ns per edge and frame), the streaming route pays ~15 us per frame launch
constexpr int kResidentEdges = 1 << 15;

inline int pow2_floor(int x) { int p = 1; while (p * 2 <= x) p *= 2; return p; }

}  // namespace

static bool resident_fits(int elem, int N, int Q) {
    return N <= kRT && resident_lds(elem, N, Q, false) - kScratch <= kResidentVec;
}

bool graph_decode_resident(int elem, int N, int Q, int E) {
    return resident_fits(elem, N, Q) && E <= kResidentEdges;
}

size_t graph_decode_work_bytes(int elem, int T, int B, int Q) {
    const size_t bp = (size_t) T * B * Q * 4;
    return (bp + 255) / 256 * 256 + 2 * (size_t) Q * B * elem;
}

template <typename R>
hipError_t launch_decode_graph(const Problem &P, const GraphArgs &G, int route, void *work, void *scores, long long *path,
                               long long *tokens, long long *tlen, long long *states, hipStream_t stream) {
    const int Q = G.Q, N = P.N, B = P.B, T = P.T;
    int *bp = (int *) work;
    R *sc = (R *) scores;
    if (Q == 0) {                    // no product state: every utterance has no path (the finish kernel reads no vector)
        hipLaunchKernelGGL((graph_finish_kernel<R>), dim3(B), dim3(kFT), 0, stream, P, G, bp, (const R *) nullptr, sc, path,
                           tokens, tlen, states);
        return hipGetLastError();
    }
    if (route == 2 ? resident_fits(sizeof(R), N, Q) : (route == 0 && graph_decode_resident(sizeof(R), N, Q, G.E))) {
        const bool trl = resident_lds(sizeof(R), N, Q, true) <= kLdsMax;
        const size_t dyn = resident_lds(sizeof(R), N, Q, trl);
        const int F = (int) min((size_t) kStageF, (dyn - kScratch) / ((size_t) Q * 4));
        // subgroup per target: wide enough to cover the row in about two strides, narrow enough to keep the workgroup busy
        const int avg = (int) (((int64_t) G.E + Q - 1) / Q);
        const int fill = pow2_floor(max(kRT / Q, 1));
        const int want = min(fill, max(avg / 2, 1));
        const int sg = want >= 64 ? 64 : (want >= 16 ? 16 : 4);
#define ASG_GRAPH_RES(GS, TRL)                                                                                              \
    do {                                                                                                                    \
        const void *fn = (const void *) graph_resident_kernel<R, GS, TRL>;                                                 \
        if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);      \
        hipLaunchKernelGGL((graph_resident_kernel<R, GS, TRL>), dim3(B), dim3(kRT), dyn, stream, P, G, bp, F, sc, path,   \
                           tokens, tlen, states);                                                                          \
    } while (0)
        if (trl) {
            if (sg == 64) ASG_GRAPH_RES(64, true); else if (sg == 16) ASG_GRAPH_RES(16, true); else ASG_GRAPH_RES(4, true);
        } else {
            if (sg == 64) ASG_GRAPH_RES(64, false); else if (sg == 16) ASG_GRAPH_RES(16, false); else ASG_GRAPH_RES(4, false);
        }
#undef ASG_GRAPH_RES
        return hipGetLastError();
    }
    R *V = (R *) ((char *) work + ((size_t) T * B * Q * 4 + 255) / 256 * 256);
    const dim3 grid((Q + kFT / 64 - 1) / (kFT / 64), (B + 63) / 64);
    for (int t = 0; t < T; ++t) {
        const R *Vp = V + (size_t) ((t + 1) & 1) * Q * B;
        R *Vt = V + (size_t) (t & 1) * Q * B;
        hipLaunchKernelGGL((graph_frame_kernel<R>), grid, dim3(kFT), 0, stream, P, G, bp, Vp, Vt, t);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((graph_finish_kernel<R>), dim3(B), dim3(kFT), 0, stream, P, G, bp, (const R *) V, sc, path, tokens,
                       tlen, states);
    return hipGetLastError();
}
template hipError_t launch_decode_graph<float>(const Problem &, const GraphArgs &, int, void *, void *, long long *,
                                               long long *, long long *, long long *, hipStream_t);
template hipError_t launch_decode_graph<double>(const Problem &, const GraphArgs &, int, void *, void *, long long *,
                                                long long *, long long *, long long *, hipStream_t);

}  // namespace asg
