// torch_asg_amd/csrc/asg_target_graph_viterbi.hip -- the BEST path of a per-utterance target graph (asg_target_graph.hip sums
// over all of them): which alternative was spoken, where its tokens lie in time, the hard targets of a next stage.  Utterance
// b, node k of label l_k, len = clamp(input_lengths[b], 0, T), in the dtype of the problem, adds and compares only:
//   f_e        = tr[l_k][l_src_e] + edge_w[e]                        (rounded once, as the score folds it)
//   v[0][k]    = start_w[k] + I[0][l_k]
//   stay       = v[t-1][k] + tr[l_k][l_k];   cand_e = v[t-1][src_e] + f_e   (edges into k in incoming-CSR order: ascending source)
//   v[t][k]    = max(stay, cand_e ...) + I[t][l_k]
//   bp[t][k]   = k unless some cand_e > stay (strictly); then the source of the FIRST edge in that order that attains the maximum
//   score[b]   = max_k (v[len-1][k] + final_w[k]);  end node = the LOWEST k that attains it
//   nodes[len-1] = end;  nodes[t-1] = bp[t][nodes[t]];  labels[t] = l_{nodes[t]}
//   tokens / token_frames: labels[t] and t at t = 0 and at every t with nodes[t] != nodes[t-1], in order; token_lengths = their count
// "Stay wins ties" is asg_viterbi.hip's rule (come > stay): for a chain with edge weight 0 the scores are asg_viterbi's and
// the nodes its positions.  A score of -inf (len 0, empty graph, no finite path) walks nothing: every integer output is -1
// and token_lengths 0; so are the frames >= len and the tokens behind token_lengths.
//
// ONE launch, one workgroup per utterance, one thread per node, 64 / 256 / 1024 threads wide as the score's kernels; three
// phases in that workgroup:
//  1. forward: the score's prologue (f_e and the sources folded into LDS, tr[l_k][l_k] in a register), v ping-pongs between
//     two LDS vectors, the next emission is loaded before the barrier.  ONE pass over the incoming edges carries (best value,
//     best source) in registers -- no second pass, no transcendental -- and the winning source goes to work[b][t][k] as 16
//     bits (K <= 1024), a frame's row one coalesced store.  Then a workgroup max and a workgroup min over the nodes that
//     attain it, both in the fixed tree.
//  2. backtrace: the workgroup wrote those rows itself, so a barrier makes them readable.  The walk is serial but must not be
//     a chain of dependent GLOBAL loads: the frames are cut into blocks of F (64; 16 at 1024 threads), all threads stage a
//     block's F x Kmax rows into LDS (16-byte loads over the block's aligned interior, guarded 2-byte loads in its first and
//     last granule), lane 0 walks the block in LDS and leaves its nodes in an LDS line, and the workgroup writes nodes and
//     labels for those frames as coalesced int64 stores.  Two staging buffers and two lines: the loads of block i-1 are
//     issued into registers before block i is walked and land in LDS after it, one barrier per block.  The staging reuses the
//     LDS of the forward loop.
//  3. compaction, chunks of W frames ascending: thread i flags t == 0 || nodes[t] != nodes[t-1], ballot + popcount rank it
//     in the wavefront, the wavefronts' counts go through the reduction slots, tokens and token_frames land at base + rank.
// Every output element is written here (the -1 fills too: no memset), no float atomics, nothing synchronises the host:
// bit-identical run to run and capturable.  Every byte offset into the workspace is 64-bit.
#include "asg_target_graph_path.h"

namespace asg {

namespace {

// (the LDS of the workgroup: tgv_lds, asg_target_graph_path.h)
template <typename R, int W>
__global__ void __launch_bounds__(W) target_graph_viterbi(Problem P, TargetGraphArgs G, uint16_t *bp, R *scores, int64_t *nodes,
                                                          int64_t *labels, int64_t *tokens, int64_t *frames, int64_t *tlen) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int F = Tgv<W>::F;
    R *red = (R *) lds;
    const R NINF = Num<R>::ninf();
    const int k = threadIdx.x, b = blockIdx.x, T = P.T, Kmax = G.Kmax;
    const TgView g = tg_view(G, b);
    const int len = g.K > 0 ? tg_len(P.in_len, b, T) : 0;
    int64_t *nb = nodes + (int64_t) b * T, *lb = labels + (int64_t) b * T;
    int64_t *kb = tokens + (int64_t) b * T, *fb = frames + (int64_t) b * T;
    // ---- 1. forward ----
    R m = NINF;
    int end = 0;
    if (len >= 1) {                                   // (uniform over the workgroup; asg_target_graph_path.h)
        const bool mine = k < g.K;
        const R c = tgv_forward<R>(P, G, g, b, len, lds, bp + (int64_t) b * T * Kmax);
        m = tg_reduce<R, W, true>(c, red);
        end = -tg_reduce<int, W, true>(mine && c == m ? -k : -(1 << 30), (int *) red);
    }
    if (k == 0) scores[b] = m;
    const int n = m > NINF ? len : 0;                 // frames that carry a path; the rest of every row is -1
    for (int t = n + k; t < T; t += W) nb[t] = lb[t] = -1;
    if (n == 0) {                                     // (uniform)
        for (int t = k; t < T; t += W) kb[t] = fb[t] = -1;
        if (k == 0) tlen[b] = 0;
        return;
    }
    // ---- 2. backtrace, block by block from the end ----
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
                nb[lo + k] = nd;
                lb[lo + k] = g.label[nd];
            }
        }
    }
    // ---- 3. compaction ----
    __syncthreads();                                  // nodes and labels of this utterance are written
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += W) {
        const int t = c0 + k;
        bool f = false;
        if (t < n) f = t == 0 || nb[t] != nb[t - 1];
        const unsigned long long mask = __ballot(f);
        const int rank = __popcll(mask & ((1ull << (k & 63)) - 1));
        int off = 0, tot = __popcll(mask);
        if (W > 64) {
            int *cnt = (int *) red;
            if ((k & 63) == 0) cnt[k >> 6] = tot;
            __syncthreads();
            tot = 0;
#pragma unroll
            for (int s = 0; s < W / 64; ++s) {
                const int c = cnt[s];
                if (s < (k >> 6)) off += c;
                tot += c;
            }
            __syncthreads();
        }
        if (f) {
            kb[base + off + rank] = lb[t];
            fb[base + off + rank] = t;
        }
        base += tot;
    }
    for (int t = base + k; t < T; t += W) kb[t] = fb[t] = -1;
    if (k == 0) tlen[b] = base;
}

template <typename R, int W>
hipError_t tgv_launch(const Problem &P, const TargetGraphArgs &G, void *work, void *scores, int64_t *const out[5],
                      hipStream_t stream) {
    const size_t dyn = tgv_lds(sizeof(R), G.Kmax, G.Emax);
    tg_set_lds((const void *) target_graph_viterbi<R, W>, dyn);
    hipLaunchKernelGGL((target_graph_viterbi<R, W>), dim3(P.B), dim3(W), dyn, stream, P, G, (uint16_t *) work, (R *) scores,
                       out[0], out[1], out[2], out[3], out[4]);
    return hipGetLastError();
}

}  // namespace

size_t target_graph_viterbi_work_bytes(int T, int B, int Kmax) { return (size_t) B * T * Kmax * 2; }

template <typename R>
hipError_t launch_target_graph_viterbi(const Problem &P, const TargetGraphArgs &G, void *work, void *scores, int64_t *nodes,
                                       int64_t *labels, int64_t *tokens, int64_t *token_frames, int64_t *token_lengths,
                                       hipStream_t stream) {
    int64_t *const out[5] = {nodes, labels, tokens, token_frames, token_lengths};
    if (G.Kmax <= 64) return tgv_launch<R, 64>(P, G, work, scores, out, stream);
    if (G.Kmax <= 256) return tgv_launch<R, 256>(P, G, work, scores, out, stream);
    return tgv_launch<R, 1024>(P, G, work, scores, out, stream);
}

template hipError_t launch_target_graph_viterbi<float>(const Problem &, const TargetGraphArgs &, void *, void *, int64_t *,
                                                       int64_t *, int64_t *, int64_t *, int64_t *, hipStream_t);
template hipError_t launch_target_graph_viterbi<double>(const Problem &, const TargetGraphArgs &, void *, void *, int64_t *,
                                                        int64_t *, int64_t *, int64_t *, int64_t *, hipStream_t);

}  // namespace asg
