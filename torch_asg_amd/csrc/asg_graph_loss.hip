// torch_asg_amd/csrc/asg_graph_loss.hip -- the log-semiring counterpart of asg_decode_graph.hip: the full score of the ASG
// lattice COMPOSED with a deterministic weighted automaton over tokens (the normaliser of a criterion whose token prior is that
// automaton), its gradients w.r.t. the emissions and the transition matrix, and the automaton's score of each target sequence.
// Product graph as in asg_decode_graph.hip; TokenGraph.compile_loss (torch_asg_amd/graph.py) adds the outgoing-edge CSR, the
// label and label-pair groupings and the automaton tables.
//   alpha[0][q]    = start_w[q] + I[0][i]
//   alpha[t][q]    = lse(stay: alpha[t-1][q] + tr[i][i];  edge e from q': (alpha[t-1][q'] + tr[i][j]) + edge_w[e]) + I[t][i]
//   Z              = lse_q(alpha[len-1][q] + final_w[q])
//   beta[len-1][q] = final_w[q]
//   beta[t-1][q']  = lse(stay: (beta[t][q'] + tr[i'][i']) + I[t][i'];  edge e to q: ((beta[t][q] + tr[i][i']) + edge_w[e]) + I[t][i])
// Every lse is max-then-sum over its candidates in a FIXED order -- the stay first, then the edges ascending (by source for
// alpha, by target for beta) -- and -inf, never NaN, when every candidate is -inf.  With g = grad_scores[b]:
//   grad_inputs[t][b][i]  = g * sum_{q of label i, ascending} exp((alpha[t][q] + beta[t][q]) - Z)          (0 for t >= len)
//   grad_transition[i][j] = sum over the stays (i == j) or the edges of that label pair, ascending, of
//                           sum_b g_b * acc[x][b],   acc[x][b] = sum_{t >= 1} exp((alpha[t-1][q'] + candidate_x) - Z)
// No float atomics: acc[x][b] of the stay of q' and of every edge leaving q' is owned by ONE thread -- the one that pulls
// beta into q' -- and a last launch reduces them per label pair (a wavefront per pair, lanes over utterances, a fixed
// butterfly).  Each route is therefore bit-identical run to run.  An utterance with len == 0 or Z == -inf contributes zeros.
//
// Resident route (both vectors in LDS: 2*Q*e <= 128 KiB, and E <= kLossResidentEdges = 4096; or wherever the vectors fit with
// ASG_FLAG_GRAPH_LOSS_RESIDENT): one 1024-thread workgroup per utterance, one thread per product state, a barrier per frame.
// Streaming route (otherwise, or ASG_FLAG_GRAPH_LOSS_STREAMING): one launch per frame and direction; a wavefront takes one
// product state and 64 utterances (lanes), as graph_frame_kernel does; the vectors live in global memory.
// alpha is stored as work[t][q][b] on both routes when asked, so the backward kernels of both routes read it the same way.
// Every output element and padding frame is written by a kernel (no memset): a warm call can be captured and replayed.
#include "asg_common.h"
#include "asg_kernels.h"

namespace asg {

namespace {

constexpr int kLT = 1024;                       // resident workgroup
constexpr int kLF = 256;                        // streaming frame / finish / reduction / walk workgroups
constexpr int kLScratch = 256;                  // resident LDS bytes in front of the vectors (reduction slots)
constexpr size_t kLossResidentVec = 128 * 1024;
// Edges above which the streaming route is taken although the vectors fit: the resident route walks every edge of an
// utterance on one CU, the streaming route pays a launch per frame.  Measured at T = 400, B = 64, N = 40:
// E = 1560 resident 18.6 ms vs streaming 20.8 ms forward+backward; E = 63960 resident 229 ms vs streaming 27.7 ms
constexpr int64_t kLossResidentEdges = 1 << 12;

template <typename R> __device__ __forceinline__ R lexp(R x);
template <> __device__ __forceinline__ float lexp<float>(float x) { return expf(x); }
template <> __device__ __forceinline__ double lexp<double>(double x) { return ::exp(x); }
template <typename R> __device__ __forceinline__ R llog(R x);
template <> __device__ __forceinline__ float llog<float>(float x) { return logf(x); }
template <> __device__ __forceinline__ double llog<double>(double x) { return ::log(x); }
template <typename R> __device__ __forceinline__ R rmax(R a, R b) { return b > a ? b : a; }

__device__ __forceinline__ int loss_len(const int64_t *in_len, int b, int T) {
    if (!in_len) return T;
    const int64_t l = in_len[b];
    return (int) (l < 0 ? 0 : (l > T ? T : l));
}

// Workgroup max / sum (blockDim.x = NT), a fixed tree; result in every thread.  red: NT / 64 slots.
template <typename R, int NT>
__device__ R block_max_r(R v, R *red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = rmax(v, (R) __shfl_xor(v, o));
    if (lane == 0) red[w] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int s = 1; s < NT / 64; ++s) v = rmax(v, red[s]);
    __syncthreads();
    return v;
}
template <typename R, int NT>
__device__ R block_sum_r(R v, R *red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += (R) __shfl_xor(v, o);
    if (lane == 0) red[w] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int s = 1; s < NT / 64; ++s) v += red[s];
    __syncthreads();
    return v;
}

// Z = lse_q(last(q) + final_w[q]) over the workgroup; called by every thread.
template <typename R, int NT, typename V>
__device__ R final_lse(int Q, V last, const R *fw, R *red) {
    const R NINF = Num<R>::ninf();
    R m = NINF;
    for (int q = threadIdx.x; q < Q; q += NT) m = rmax(m, last(q) + fw[q]);
    m = block_max_r<R, NT>(m, red);
    if (!(m > NINF)) return NINF;
    R s = R(0);
    for (int q = threadIdx.x; q < Q; q += NT) s += lexp((last(q) + fw[q]) - m);
    s = block_sum_r<R, NT>(s, red);
    return m + llog(s);
}

// alpha[t][q] without the emission: vp(q') = alpha[t-1][q'], tr(i, j) = transition[i][j].
template <typename R, typename V, typename TRF>
__device__ __forceinline__ R alpha_lse(const GraphArgs &g, int q, int i, V vp, TRF tr) {
    const R *ew = (const R *) g.edge_w;
    const int e0 = g.row[q], e1 = g.row[q + 1];
    const R stay = vp(q) + tr(i, i);
    R m = stay;
    for (int e = e0; e < e1; ++e) m = rmax(m, (vp(g.src[e]) + tr(i, g.src_label[e])) + ew[e]);
    if (!(m > Num<R>::ninf())) return Num<R>::ninf();
    R s = lexp(stay - m);
    for (int e = e0; e < e1; ++e) s += lexp(((vp(g.src[e]) + tr(i, g.src_label[e])) + ew[e]) - m);
    return m + llog(s);
}

// beta[t-1][qp] from bt(q) = beta[t][q]; em(i) = I[t][i].  Adds the posteriors exp((a + candidate) - Z) of the stay of qp and of
// every edge leaving it to their accumulators accb[x * B] (a = alpha[t-1][qp]).
template <typename R, typename V, typename TRF, typename EMF>
__device__ __forceinline__ R beta_lse(const GraphArgs &g, const GraphLossArgs &L, int qp, V bt, TRF tr, EMF em, R a, R Z,
                                      R *accb, int64_t B) {
    const R *ew = (const R *) g.edge_w;
    const R NINF = Num<R>::ninf();
    const int ip = g.label[qp];
    const int k0 = L.orow[qp], k1 = L.orow[qp + 1];
    const R stay = (bt(qp) + tr(ip, ip)) + em(ip);
    R m = stay;
    for (int k = k0; k < k1; ++k) {
        const int e = L.oedge[k], q = L.tgt[e], i = g.label[q];
        m = rmax(m, ((bt(q) + tr(i, ip)) + ew[e]) + em(i));
    }
    const bool any = m > NINF;
    R s = any ? lexp(stay - m) : R(0);
    accb[(int64_t) qp * B] += lexp((a + stay) - Z);
    for (int k = k0; k < k1; ++k) {
        const int e = L.oedge[k], q = L.tgt[e], i = g.label[q];
        const R c = ((bt(q) + tr(i, ip)) + ew[e]) + em(i);
        if (any) s += lexp(c - m);
        accb[((int64_t) g.Q + e) * B] += lexp((a + c) - Z);
    }
    return any ? m + llog(s) : NINF;
}

// sum over the product states of label i of exp((alpha[t][q] + beta[t][q]) - Z), ascending q.  At(q) = alpha[t][q].
template <typename R, typename VA, typename VB>
__device__ __forceinline__ R label_post(const GraphLossArgs &L, int i, VA At, VB bt, R Z) {
    R s = R(0);
    for (int k = L.lrow[i], k1 = L.lrow[i + 1]; k < k1; ++k) {
        const int q = L.lq[k];
        s += lexp((At(q) + bt(q)) - Z);
    }
    return s;
}

// zero the accumulators a thread owns: the stay of qp and every edge leaving it
template <typename R>
__device__ __forceinline__ void zero_owned(const GraphArgs &g, const GraphLossArgs &L, int qp, R *accb, int64_t B) {
    accb[(int64_t) qp * B] = R(0);
    for (int k = L.orow[qp], k1 = L.orow[qp + 1]; k < k1; ++k) accb[((int64_t) g.Q + L.oedge[k]) * B] = R(0);
}

// ---------------------------------------------------------------------------------------------------------------------
// Resident route.  Dynamic LDS: [reduction slots 256 B][v 2*Q].
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kLT) graph_loss_fwd_resident(Problem P, GraphArgs g, R *A, R *scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    R *red = (R *) lds;
    R *v = (R *) (lds + kLScratch);
    const int Q = g.Q, T = P.T, tid = threadIdx.x, b = blockIdx.x;
    const int64_t B = P.B;
    const int len = loss_len(P.in_len, b, T);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *trm = (const R *) P.transition;
    const R *sw = (const R *) g.start_w, *fw = (const R *) g.final_w;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };
    if (len >= 1) {
        for (int q = tid; q < Q; q += kLT) {
            const R x = sw[q] + in[(int64_t) g.label[q] * P.is2];
            v[q] = x;
            if (A) A[(int64_t) q * B + b] = x;
        }
    }
    __syncthreads();
    for (int t = 1; t < len; ++t) {
        const R *vp = v + (int64_t) ((t - 1) & 1) * Q;
        R *vn = v + (int64_t) (t & 1) * Q;
        for (int q = tid; q < Q; q += kLT) {
            const int i = g.label[q];
            const R x = alpha_lse<R>(g, q, i, [&](int s) { return vp[s]; }, tr) + in[(int64_t) t * P.is0 + (int64_t) i * P.is2];
            vn[q] = x;
            if (A) A[((int64_t) t * Q + q) * B + b] = x;
        }
        __syncthreads();
    }
    R Z = Num<R>::ninf();
    if (len >= 1) {
        const R *vl = v + (int64_t) ((len - 1) & 1) * Q;
        Z = final_lse<R, kLT>(Q, [&](int q) { return vl[q]; }, fw, red);
    }
    if (tid == 0) scores[b] = Z;
}

template <typename R>
__global__ void __launch_bounds__(kLT) graph_loss_bwd_resident(Problem P, GraphArgs g, GraphLossArgs L, const R *A, const R *Zs,
                                                               const R *gs, R *gin, R *acc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    R *bv = (R *) (lds + kLScratch);
    const int Q = g.Q, T = P.T, N = P.N, tid = threadIdx.x, b = blockIdx.x;
    const int64_t B = P.B;
    const int len = loss_len(P.in_len, b, T);
    const R Z = Zs[b], gb = gs[b];
    const bool ok = len >= 1 && Z > Num<R>::ninf();
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *trm = (const R *) P.transition;
    const R *fw = (const R *) g.final_w;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };
    R *accb = acc + b;
    for (int qp = tid; qp < Q; qp += kLT) zero_owned(g, L, qp, accb, B);
    const int t0 = ok ? len : 0;                      // rows from t0 on are zero
    for (int64_t x = tid; x < (int64_t) (T - t0) * N; x += kLT)
        gin[((int64_t) (t0 + x / N) * B + b) * N + x % N] = R(0);
    if (!ok) return;                                  // (uniform over the workgroup)
    for (int q = tid; q < Q; q += kLT) bv[(int64_t) ((len - 1) & 1) * Q + q] = fw[q];
    __syncthreads();
    for (int t = len - 1; t >= 0; --t) {
        const R *bt = bv + (int64_t) (t & 1) * Q;
        const R *At = A + (int64_t) t * Q * B + b;
        for (int i = tid; i < N; i += kLT)
            gin[((int64_t) t * B + b) * N + i] =
                gb * label_post<R>(L, i, [&](int q) { return At[(int64_t) q * B]; }, [&](int q) { return bt[q]; }, Z);
        if (t >= 1) {
            R *bn = bv + (int64_t) ((t - 1) & 1) * Q;
            const R *Ap = A + (int64_t) (t - 1) * Q * B + b;
            auto em = [&](int i) -> R { return in[(int64_t) t * P.is0 + (int64_t) i * P.is2]; };
            for (int qp = tid; qp < Q; qp += kLT)
                bn[qp] = beta_lse<R>(g, L, qp, [&](int q) { return bt[q]; }, tr, em, Ap[(int64_t) qp * B], Z, accb, B);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Streaming route.  Frame kernels: wavefront w of block x takes product state (or label) k = 4x + w, lane l utterance
// b = 64y + l.  Vectors [Q][B].
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kLF) graph_loss_fwd_frame(Problem P, GraphArgs g, const R *__restrict__ Vp, R *__restrict__ Vt,
                                                           int t) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int q = blockIdx.x * (kLF / 64) + w;
    const int b = blockIdx.y * 64 + lane;
    const int Q = g.Q;
    const int64_t B = P.B;
    if (q >= Q || b >= B || t >= loss_len(P.in_len, b, P.T)) return;
    const int i = g.label[q];
    const R x = ((const R *) P.inputs)[(int64_t) t * P.is0 + (int64_t) b * P.is1 + (int64_t) i * P.is2];
    if (t == 0) {
        Vt[(int64_t) q * B + b] = ((const R *) g.start_w)[q] + x;
        return;
    }
    const R *trm = (const R *) P.transition;
    auto tr = [&](int ii, int j) -> R { return trm[(int64_t) ii * P.ts0 + (int64_t) j * P.ts1]; };
    Vt[(int64_t) q * B + b] = alpha_lse<R>(g, q, i, [&](int s) { return Vp[(int64_t) s * B + b]; }, tr) + x;
}

// Z per utterance from alpha[len-1]: row r of V at V + r * Q * B, r = len - 1 (stored) or (len - 1) & 1 (ping-pong).
template <typename R>
__global__ void __launch_bounds__(kLF) graph_loss_fwd_finish(Problem P, GraphArgs g, const R *V, int store, R *scores) {
    __shared__ R red[kLF / 64];
    const int b = blockIdx.x, Q = g.Q;
    const int64_t B = P.B;
    const int len = loss_len(P.in_len, b, P.T);
    R Z = Num<R>::ninf();
    if (len >= 1) {
        const R *vl = V + (int64_t) (store ? len - 1 : (len - 1) & 1) * Q * B + b;
        Z = final_lse<R, kLF>(Q, [&](int q) { return vl[(int64_t) q * B]; }, (const R *) g.final_w, red);
    }
    if (threadIdx.x == 0) scores[b] = Z;
}

// Frame t of the backward pass: grad_inputs row t from beta[t], and beta[t-1] (with the posteriors of frame t) into Bn.
template <typename R>
__global__ void __launch_bounds__(kLF) graph_loss_bwd_frame(Problem P, GraphArgs g, GraphLossArgs L, const R *A,
                                                           const R *__restrict__ Bt, R *__restrict__ Bn, const R *Zs,
                                                           const R *gs, R *gin, R *acc, int t) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int k = blockIdx.x * (kLF / 64) + w;
    const int b = blockIdx.y * 64 + lane;
    const int Q = g.Q, N = P.N, T = P.T;
    const int64_t B = P.B;
    if (b >= B) return;
    const int len = loss_len(P.in_len, b, T);
    const R Z = Zs[b];
    const bool ok = len >= 1 && Z > Num<R>::ninf();
    R *accb = acc + b;
    const R *fw = (const R *) g.final_w;
    auto bt = [&](int q) -> R { return t == len - 1 ? fw[q] : Bt[(int64_t) q * B + b]; };
    if (k < Q && t == T - 1) zero_owned(g, L, k, accb, B);
    if (k < N) {
        R val = R(0);
        if (ok && t < len) {
            const R *At = A + (int64_t) t * Q * B + b;
            val = gs[b] * label_post<R>(L, k, [&](int q) { return At[(int64_t) q * B]; }, bt, Z);
        }
        gin[((int64_t) t * B + b) * N + k] = val;
    }
    if (k < Q && ok && t >= 1 && t < len) {
        const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
        const R *trm = (const R *) P.transition;
        auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };
        auto em = [&](int i) -> R { return in[(int64_t) t * P.is0 + (int64_t) i * P.is2]; };
        const R a = A[((int64_t) (t - 1) * Q + k) * B + b];
        Bn[(int64_t) k * B + b] = beta_lse<R>(g, L, k, bt, tr, em, a, Z, accb, B);
    }
}

// grad_transition[i][j]: a wavefront per (i, j), lanes over utterances; the stays of label i (i == j) or the edges of the pair
// (binary search in the sorted pair keys), ascending, then a fixed butterfly.  Block x = i, 4 * y + w = j.
template <typename R>
__global__ void __launch_bounds__(kLF) graph_loss_tr_reduce(GraphArgs g, GraphLossArgs L, const R *acc, const R *gs, int B, int N,
                                                           R *gtr) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int i = blockIdx.x, j = blockIdx.y * (kLF / 64) + w;
    if (j >= N) return;
    const int64_t Bl = B;
    R s = R(0);
    auto add = [&](int64_t x) {
        for (int b = lane; b < B; b += 64) s += gs[b] * acc[x * Bl + b];
    };
    if (i == j) {
        for (int k = L.lrow[i], k1 = L.lrow[i + 1]; k < k1; ++k) add(L.lq[k]);
    } else {
        const int64_t key = (int64_t) i * N + j;
        int lo = 0, hi = g.E;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (L.pkey[mid] < key) lo = mid + 1; else hi = mid;
        }
        for (int k = lo; k < g.E && L.pkey[k] == key; ++k) add((int64_t) g.Q + L.pedge[k]);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += (R) __shfl_xor(s, o);
    if (lane == 0) gtr[(int64_t) i * N + j] = s;
}

// A(collapse(targets[b][:tl])): the automaton walk of one utterance per thread; -inf when the automaton rejects it.
template <typename R>
__global__ void __launch_bounds__(kLF) graph_target_walk(Problem P, GraphLossArgs L, R *out) {
    const int b = blockIdx.x * kLF + threadIdx.x;
    if (b >= P.B) return;
    const int S = P.S, N = P.N;
    const int64_t l = P.tg_len ? P.tg_len[b] : S;
    const int tl = (int) (l < 0 ? 0 : (l > S ? S : l));
    const R *arcw = (const R *) L.arcw;
    int st = L.start;
    long long prev = -1;
    R s = R(0);
    bool ok = true;
    for (int k = 0; k < tl; ++k) {
        const long long y = P.targets[(int64_t) b * P.gs0 + (int64_t) k * P.gs1];
        if (y == prev) continue;                      // consecutive equal labels are one token
        if (y < 0 || y >= N) { ok = false; break; }
        const int64_t a = (int64_t) st * N + y;
        const int nx = L.next[a];
        if (nx < 0) { ok = false; break; }
        s = s + arcw[a];
        st = nx;
        prev = y;
    }
    out[b] = ok ? s + ((const R *) L.finw)[st] : Num<R>::ninf();
}

inline size_t loss_lds(int elem, int Q) { return kLScratch + 2 * (size_t) Q * elem; }
inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }

inline void set_lds(const void *fn, size_t dyn) {
    if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);
}

}  // namespace

bool graph_loss_resident(int route, int elem, int Q, int64_t E) {
    if (Q == 0) return true;                          // (no product state: the resident kernels only write the outputs)
    const bool fits = loss_lds(elem, Q) - kLScratch <= kLossResidentVec;
    if (route == 1) return false;
    if (route == 2) return fits;
    return fits && E <= kLossResidentEdges;
}

size_t graph_loss_work_bytes(int elem, int T, int B, int Q, bool store) {
    return (size_t) (store ? T : 2) * Q * B * elem;
}

size_t graph_loss_scratch_bytes(int elem, int B, int Q, int E) {
    return align256(2 * (size_t) Q * B * elem) + ((size_t) Q + E) * B * elem;
}

template <typename R>
hipError_t launch_graph_loss_forward(const Problem &P, const GraphArgs &G, int route, bool store, void *work, void *scores,
                                     hipStream_t stream) {
    const int Q = G.Q, B = P.B, T = P.T;
    R *V = (R *) work, *sc = (R *) scores;
    if (graph_loss_resident(route, sizeof(R), Q, G.E)) {
        const size_t dyn = loss_lds(sizeof(R), Q);
        set_lds((const void *) graph_loss_fwd_resident<R>, dyn);
        hipLaunchKernelGGL((graph_loss_fwd_resident<R>), dim3(B), dim3(kLT), dyn, stream, P, G, store ? V : (R *) nullptr, sc);
        return hipGetLastError();
    }
    const size_t QB = (size_t) Q * B;
    const dim3 grid((Q + kLF / 64 - 1) / (kLF / 64), (B + 63) / 64);
    for (int t = 0; t < T; ++t) {
        const R *Vp = t == 0 ? V : (store ? V + (size_t) (t - 1) * QB : V + (size_t) ((t + 1) & 1) * QB);
        R *Vt = store ? V + (size_t) t * QB : V + (size_t) (t & 1) * QB;
        hipLaunchKernelGGL((graph_loss_fwd_frame<R>), grid, dim3(kLF), 0, stream, P, G, Vp, Vt, t);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((graph_loss_fwd_finish<R>), dim3(B), dim3(kLF), 0, stream, P, G, (const R *) V, (int) store, sc);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_graph_loss_backward(const Problem &P, const GraphArgs &G, const GraphLossArgs &L, int route, const void *work,
                                      const void *scores, const void *grad_scores, void *grad_inputs, void *grad_transition,
                                      void *scratch, hipStream_t stream) {
    const int Q = G.Q, B = P.B, T = P.T, N = P.N;
    const R *A = (const R *) work, *Zs = (const R *) scores, *gs = (const R *) grad_scores;
    R *gin = (R *) grad_inputs, *gtr = (R *) grad_transition;
    const size_t QB = (size_t) Q * B;
    R *Bv = (R *) scratch;
    R *acc = (R *) ((char *) scratch + align256(2 * QB * sizeof(R)));
    if (graph_loss_resident(route, sizeof(R), Q, G.E)) {
        const size_t dyn = loss_lds(sizeof(R), Q);
        set_lds((const void *) graph_loss_bwd_resident<R>, dyn);
        hipLaunchKernelGGL((graph_loss_bwd_resident<R>), dim3(B), dim3(kLT), dyn, stream, P, G, L, A, Zs, gs, gin, acc);
    } else {
        const int K = Q > N ? Q : N;
        const dim3 grid((K + kLF / 64 - 1) / (kLF / 64), (B + 63) / 64);
        for (int t = T - 1; t >= 0; --t) {
            const R *Bt = Bv + (size_t) (t & 1) * QB;
            R *Bn = Bv + (size_t) ((t + 1) & 1) * QB;
            hipLaunchKernelGGL((graph_loss_bwd_frame<R>), grid, dim3(kLF), 0, stream, P, G, L, A, Bt, Bn, Zs, gs, gin, acc, t);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((graph_loss_tr_reduce<R>), dim3(N, (N + kLF / 64 - 1) / (kLF / 64)), dim3(kLF), 0, stream, G, L,
                       (const R *) acc, gs, B, N, gtr);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_graph_target_scores(const Problem &P, const GraphLossArgs &L, void *out, hipStream_t stream) {
    hipLaunchKernelGGL((graph_target_walk<R>), dim3((P.B + kLF - 1) / kLF), dim3(kLF), 0, stream, P, L, (R *) out);
    return hipGetLastError();
}

template hipError_t launch_graph_loss_forward<float>(const Problem &, const GraphArgs &, int, bool, void *, void *, hipStream_t);
template hipError_t launch_graph_loss_forward<double>(const Problem &, const GraphArgs &, int, bool, void *, void *, hipStream_t);
template hipError_t launch_graph_loss_backward<float>(const Problem &, const GraphArgs &, const GraphLossArgs &, int, const void *,
                                                      const void *, const void *, void *, void *, void *, hipStream_t);
template hipError_t launch_graph_loss_backward<double>(const Problem &, const GraphArgs &, const GraphLossArgs &, int, const void *,
                                                       const void *, const void *, void *, void *, void *, hipStream_t);
template hipError_t launch_graph_target_scores<float>(const Problem &, const GraphLossArgs &, void *, hipStream_t);
template hipError_t launch_graph_target_scores<double>(const Problem &, const GraphLossArgs &, void *, hipStream_t);

}  // namespace asg
