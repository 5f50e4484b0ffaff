// torch_asg_amd/csrc/asg_target_graph_hard.hip -- the BEST-PATH score of a per-utterance target graph as a training criterion
// (a Viterbi / hard numerator): asg_target_graph_viterbi.hip's score, bit for bit, and the gradient of that score, which is a
// one-hot over its own path.  v, bp, f_e, len and the tie rules (stay wins ties, first lowest-source edge, lowest end node)
// are asg_target_graph_viterbi.hip's, in the dtype of the problem.  With nodes[0..n-1] that path (n = len where the score is
// finite, else 0), labels[t] = l_{nodes[t]} and g = grad_scores[b]:
//   grad_inputs[t][b][i]  = g if t < n and i == labels[t], else 0
//   count_b[slot]         = number of t in [1, n) whose step nodes[t-1] -> nodes[t] is that slot: slot k (the stay on node k)
//                           when nodes[t] == nodes[t-1] == k, else slot Kmax + e, e the FIRST edge in incoming-CSR order of
//                           nodes[t] whose source is nodes[t-1]
//   grad_transition[i][j] = sum over the batch-wide list pslot of label pair (i, j), in list order (64 lanes striding the
//                           pair's segment, then the fixed xor butterfly: target_graph_tr_reduce's order), of g_b * count_b[slot]
// Parallel edges with one source and one target share a label pair, so which of them is counted never changes
// grad_transition.  An utterance whose score is -inf has zero gradient rows and zero counts.
//
// Forward: ONE launch, one workgroup per utterance, one thread per node, 64 / 256 / 1024 wide.  Without a gradient it is
// tgv_forward with the back-pointer stores compiled out, the fixed-tree max, and nothing else: no workspace.  With one, four
// phases in that workgroup:
//  1. tgv_forward (asg_target_graph_path.h), the max and the lowest end node that attains it.
//  2. the walk, asg_target_graph_viterbi.hip's: blocks of F frames staged into LDS through registers (tgv_fetch / tgv_put),
//     two buffers, lane 0 walks a block while the one before it is in flight.  A block's nodes leave its LDS line as 16 bits
//     into the workspace ([B][T]) and its labels as int32 ([B][T], -1 from n on): what the backward reads.  Writing the nodes
//     out keeps the count phase off the block loop: a step needs nodes[t] and nodes[t-1], and the latter of a block's first
//     frame is known only after the NEXT block is walked.
//  3. the counts: the staging is dead, its LDS becomes a histogram of Kmax + Emax ints (256 + (Kmax + Emax) * 4 <= the
//     forward's own 256 + 2 * Kmax * e + Emax * (e + 4), so the request stays tgv_lds).  One thread per frame resolves the slot
//     of its step -- a compare for the stay, else a scan of the target's incoming row for the first edge from the previous node
//     -- and adds 1 with an LDS INTEGER atomic.  Integer adds commute: equal bits run to run.
//  4. the histogram goes to the workspace, every element of [Kmax + Emax] written.
// Backward: a flat kernel over the 16-byte granules of [T,B,N] (one vector store each, guarded scalars in a first or last
// partial granule; 64-bit offsets) that writes g_b or 0 from the int32 labels, the zero-fill of [N,N], and a wavefront per used
// label pair over the int32 counts.  No float atomics, every output element written by a kernel (no memset), nothing
// synchronises: bit-identical run to run and capturable.
#include "asg_target_graph_path.h"

namespace asg {

namespace {

constexpr int kTghF = 256;                      // workgroup of the three backward kernels

inline size_t tgh_round16(size_t n) { return (n + 15) & ~(size_t) 15; }

// the parts of the workspace, each rounded up to 16 bytes: back-pointers, labels, counts, nodes
struct TghWork {
    size_t bp, lab, cnt, nod;
    TghWork(int T, int B, int Kmax, int64_t Emax)
        : bp(tgh_round16((size_t) B * T * Kmax * 2)), lab(tgh_round16((size_t) B * T * 4)),
          cnt(tgh_round16((size_t) B * ((size_t) Kmax + Emax) * 4)), nod(tgh_round16((size_t) B * T * 2)) {}
    size_t total() const { return bp + lab + cnt + nod; }
};

template <typename R, int W, bool STORE>
__global__ void __launch_bounds__(W) target_graph_hard_fwd(Problem P, TargetGraphArgs G, uint16_t *bp, R *scores, int *plab,
                                                           int *cnt, uint16_t *nod) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int F = Tgv<W>::F;
    R *red = (R *) lds;
    const R NINF = Num<R>::ninf();
    const int k = threadIdx.x, b = blockIdx.x, T = P.T, Kmax = G.Kmax;
    const TgView g = tg_view(G, b);
    const int len = g.K > 0 ? tg_len(P.in_len, b, T) : 0;
    // ---- 1. forward ----
    R m = NINF;
    int end = 0;
    if (len >= 1) {                                   // (uniform over the workgroup; asg_target_graph_path.h)
        const bool mine = k < g.K;
        const R c = tgv_forward<R, STORE>(P, G, g, b, len, lds, STORE ? bp + (int64_t) b * T * Kmax : nullptr);
        m = tg_reduce<R, W, true>(c, red);
        if (STORE) end = -tg_reduce<int, W, true>(mine && c == m ? -k : -(1 << 30), (int *) red);
    }
    if (k == 0) scores[b] = m;
    if (!STORE) return;
    const int slots = Kmax + G.Emax;
    int *lb = plab + (int64_t) b * T, *cb = cnt + (int64_t) b * slots;
    uint16_t *nb = nod + (int64_t) b * T;
    const int n = m > NINF ? len : 0;                 // frames that carry a path
    for (int t = n + k; t < T; t += W) lb[t] = -1;
    if (n == 0) {                                     // (uniform) this utterance adds zeros to grad_transition
        for (int s = k; s < slots; s += W) cb[s] = 0;
        return;
    }
    // ---- 2. the walk, block by block from the end ----
    __syncthreads();                                  // the rows of this workgroup are written; the forward's LDS is free
    {
        const uint16_t *bpb = bp + (int64_t) b * T * Kmax;
        const size_t cap = ((size_t) F * Kmax + 14) / 8;
        uint4 *stage = (uint4 *) (lds + kTgRed);      // two buffers of `cap` granules
        int *line = (int *) (stage + 2 * cap);        // two lines of F nodes
        uint4 r[Tgv<W>::NG];
        const int last = (n - 1) / F;
        {
            const uint16_t *rows = bpb + (int64_t) last * F * Kmax;
            tgv_fetch<W>(rows, (n - last * F) * Kmax, r);
            tgv_put<W>(rows, (n - last * F) * Kmax, r, stage);
        }
        __syncthreads();
        int cur = end, p = 0;
        for (int j = last; j >= 0; --j, p ^= 1) {
            const int lo = j * F, hi = (lo + F < n ? lo + F : n) - 1;
            const uint16_t *rows = bpb + (int64_t) lo * Kmax, *next = rows - (int64_t) F * Kmax;
            if (j > 0) tgv_fetch<W>(next, F * Kmax, r);            // block j-1: in flight while block j is walked
            if (k == 0) {
                const uint16_t *st = (const uint16_t *) (stage + (size_t) p * cap) + (((uintptr_t) rows & 15) >> 1);
                int *ln = line + p * F;
                for (int t = hi; t >= lo; --t) {
                    ln[t - lo] = cur;
                    if (t > 0) cur = st[(t - lo) * Kmax + cur];
                }
            }
            if (j > 0) tgv_put<W>(next, F * Kmax, r, stage + (size_t) (p ^ 1) * cap);
            __syncthreads();
            if (k <= hi - lo) {
                const int nd = line[p * F + k];
                nb[lo + k] = (uint16_t) nd;
                lb[lo + k] = g.label[nd];
            }
        }
    }
    // ---- 3. the counts ----
    __syncthreads();                                  // the nodes of this utterance are written; staging and lines are dead
    int *hist = (int *) (lds + kTgRed);
    for (int s = k; s < slots; s += W) hist[s] = 0;
    __syncthreads();
    for (int t = 1 + k; t < n; t += W) {
        const int a = nb[t - 1], c = nb[t];
        int slot = c;                                 // the stay
        if (a != c) {
            slot = -1;
            for (int e = g.row[c], e1 = g.row[c + 1]; e < e1; ++e)
                if (g.src[e] == a) { slot = Kmax + e; break; }
        }
        if (slot >= 0) atomicAdd(hist + slot, 1);
    }
    __syncthreads();
    // ---- 4. out ----
    for (int s = k; s < slots; s += W) cb[s] = hist[s];
}

// grad_inputs as a flat array of `total` elements from `gin`: granule q covers the elements [q * V - mis, q * V - mis + V), V =
// 16 / sizeof(R) and mis the elements by which gin lies behind a 16-byte boundary, so every interior granule is one aligned
// 16-byte store.  Element x = (t * B + b) * N + i.
template <typename R>
__global__ void __launch_bounds__(kTghF) target_graph_hard_gin(const int *plab, const R *gs, R *gin, int64_t total, int T, int B,
                                                               int N) {
    constexpr int V = 16 / (int) sizeof(R);
    const int mis = (int) (((uintptr_t) gin & 15) / sizeof(R));
    const int64_t lo = ((int64_t) blockIdx.x * kTghF + threadIdx.x) * V - mis;
    if (lo >= total) return;
    const int64_t x0 = lo < 0 ? 0 : lo;
    int64_t row = x0 / N;
    int i = (int) (x0 - row * N);
    R v[V];
    R gb = R(0);
    int lab = -1;
    bool fresh = true;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        v[j] = R(0);
        if (lo + j < 0 || lo + j >= total) continue;
        if (fresh) {                                  // a new row (t, b): its label and its g
            const int64_t t = row / B;
            const int bb = (int) (row - t * B);
            lab = plab[(int64_t) bb * T + t];
            gb = gs[bb];
            fresh = false;
        }
        v[j] = i == lab ? gb : R(0);
        if (++i == N) { i = 0; ++row; fresh = true; }
    }
    if (lo >= 0 && lo + V <= total) {
        uint4 u;
        __builtin_memcpy(&u, v, 16);
        *(uint4 *) (gin + lo) = u;
    } else {                                          // the first or the last granule: nothing outside the array is written
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (lo + j >= 0 && lo + j < total) gin[lo + j] = v[j];
    }
}

template <typename R>
__global__ void __launch_bounds__(kTghF) target_graph_hard_tr_zero(R *gtr, int64_t n) {
    const int64_t x = (int64_t) blockIdx.x * kTghF + threadIdx.x;
    if (x < n) gtr[x] = R(0);
}

// a wavefront per label pair that some graph of the batch uses, in target_graph_tr_reduce's order, over the integer counts
template <typename R>
__global__ void __launch_bounds__(kTghF) target_graph_hard_tr_reduce(TargetGraphArgs G, const int *cnt, const R *gs, R *gtr) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t pair = (int64_t) blockIdx.x * (kTghF / 64) + w;
    if (pair >= G.npairs) return;
    const int slots = G.Kmax + G.Emax;
    R s = R(0);
    for (int x = G.pseg[pair] + lane, x1 = G.pseg[pair + 1]; x < x1; x += 64) {
        const int at = G.pslot[x];                    // b * (Kmax + Emax) + slot
        s += gs[at / slots] * (R) cnt[at];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += (R) __shfl_xor(s, o);
    if (lane == 0) gtr[G.pkey[pair]] = s;
}

template <typename R, int W>
hipError_t tgh_forward(const Problem &P, const TargetGraphArgs &G, bool store, void *work, R *scores, hipStream_t stream) {
    if (!store) {
        const size_t dyn = tg_fwd_lds(sizeof(R), G.Kmax, G.Emax);
        tg_set_lds((const void *) target_graph_hard_fwd<R, W, false>, dyn);
        hipLaunchKernelGGL((target_graph_hard_fwd<R, W, false>), dim3(P.B), dim3(W), dyn, stream, P, G, (uint16_t *) nullptr,
                           scores, (int *) nullptr, (int *) nullptr, (uint16_t *) nullptr);
        return hipGetLastError();
    }
    const TghWork L(P.T, P.B, G.Kmax, G.Emax);
    char *w = (char *) work;
    const size_t dyn = tgv_lds(sizeof(R), G.Kmax, G.Emax);
    tg_set_lds((const void *) target_graph_hard_fwd<R, W, true>, dyn);
    hipLaunchKernelGGL((target_graph_hard_fwd<R, W, true>), dim3(P.B), dim3(W), dyn, stream, P, G, (uint16_t *) w, scores,
                       (int *) (w + L.bp), (int *) (w + L.bp + L.lab), (uint16_t *) (w + L.bp + L.lab + L.cnt));
    return hipGetLastError();
}

}  // namespace

size_t target_graph_hard_work_bytes(int T, int B, int Kmax, int64_t Emax, bool store) {
    return store ? TghWork(T, B, Kmax, Emax).total() : 0;
}

template <typename R>
hipError_t launch_target_graph_hard_forward(const Problem &P, const TargetGraphArgs &G, bool store, void *work, void *scores,
                                            hipStream_t stream) {
    if (G.Kmax <= 64) return tgh_forward<R, 64>(P, G, store, work, (R *) scores, stream);
    if (G.Kmax <= 256) return tgh_forward<R, 256>(P, G, store, work, (R *) scores, stream);
    return tgh_forward<R, 1024>(P, G, store, work, (R *) scores, stream);
}

template <typename R>
hipError_t launch_target_graph_hard_backward(const Problem &P, const TargetGraphArgs &G, const void *work,
                                             const void *grad_scores, void *grad_inputs, void *grad_transition,
                                             hipStream_t stream) {
    constexpr int V = 16 / (int) sizeof(R);
    const TghWork L(P.T, P.B, G.Kmax, G.Emax);
    const int *plab = (const int *) ((const char *) work + L.bp), *cnt = (const int *) ((const char *) work + L.bp + L.lab);
    const R *gs = (const R *) grad_scores;
    R *gin = (R *) grad_inputs, *gtr = (R *) grad_transition;
    const int64_t total = (int64_t) P.T * P.B * P.N, NN = (int64_t) P.N * P.N;
    const int64_t gran = (total + (int64_t) (((uintptr_t) gin & 15) / sizeof(R)) + V - 1) / V;
    hipError_t e;
    if (gran > 0) {
        hipLaunchKernelGGL((target_graph_hard_gin<R>), dim3((unsigned) ((gran + kTghF - 1) / kTghF)), dim3(kTghF), 0, stream,
                           plab, gs, gin, total, P.T, P.B, P.N);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL((target_graph_hard_tr_zero<R>), dim3((unsigned) ((NN + kTghF - 1) / kTghF)), dim3(kTghF), 0, stream, gtr, NN);
    if ((e = hipGetLastError()) != hipSuccess || G.npairs == 0) return e;
    hipLaunchKernelGGL((target_graph_hard_tr_reduce<R>), dim3((unsigned) ((G.npairs + kTghF / 64 - 1) / (kTghF / 64))), dim3(kTghF),
                       0, stream, G, cnt, gs, gtr);
    return hipGetLastError();
}

template hipError_t launch_target_graph_hard_forward<float>(const Problem &, const TargetGraphArgs &, bool, void *, void *,
                                                            hipStream_t);
template hipError_t launch_target_graph_hard_forward<double>(const Problem &, const TargetGraphArgs &, bool, void *, void *,
                                                             hipStream_t);
template hipError_t launch_target_graph_hard_backward<float>(const Problem &, const TargetGraphArgs &, const void *, const void *,
                                                             void *, void *, hipStream_t);
template hipError_t launch_target_graph_hard_backward<double>(const Problem &, const TargetGraphArgs &, const void *, const void *,
                                                              void *, void *, hipStream_t);

}  // namespace asg
