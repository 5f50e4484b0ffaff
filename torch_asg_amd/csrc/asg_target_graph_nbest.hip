// torch_asg_amd/csrc/asg_target_graph_nbest.hip -- the N BEST paths of a per-utterance target graph, one per final node:
// "which of these pronunciations / segmentations / readings was spoken, which was the runner-up, and by how much".  Row r is
// the best path that ends in the r-th best final node.  v, bp, f_e and len are asg_target_graph_viterbi.hip's, unchanged
// (the same device function runs); in the dtype of the problem, adds and compares only:
//   end[k]      = v[len-1][k] + final_w[k]                                    for k < K_b
//   candidates  = the nodes with end[k] > -inf, ordered by (end descending, k ascending)
//   num_hyps[b] = min(nbest, number of candidates)
//   row r < num_hyps: end_nodes = candidate r; scores = end[candidate r]; nodes[len-1] = candidate r,
//                     nodes[t-1] = bp[t][nodes[t]], labels[t] = l_{nodes[t]}; tokens / token_frames / token_lengths by the
//                     best path's rule; emission_scores: a = I[0][labels[0]], then for t = 1 .. len-1 in order
//                     a = (a + tr[labels[t]][labels[t-1]]) + I[t][labels[t]]
//   rows >= num_hyps: scores and emission_scores -inf, every integer -1, token_lengths 0
// Row 0 is the best path's result bit for bit (the lowest arg-max node is the first candidate).
//
// ONE launch, one workgroup per utterance, one thread per node, 64 / 256 / 1024 threads wide; four phases:
//  1. forward: tgv_forward (asg_target_graph_path.h); end[k] stays in the thread's register.
//  2. rank: end goes to LDS (the forward's v vector is free) and thread k COUNTS the nodes that precede it -- a loop over K_b
//     elements in which all lanes read the same address (a broadcast, no bank conflict), at most 1024 steps, no data
//     movement.  A bitonic network over W (value, index) pairs would take log2(W)^2 / 2 exchange steps with a barrier each
//     (55 at 1024) and still needs the count of candidates; the count gives the rank directly and costs less than one frame
//     block of the walk.  A candidate of rank < nbest writes k to order[rank] (ranks are distinct: a total order), the number
//     of candidates is a workgroup sum in the fixed tree.  No atomics.
//  3. walk: num_hyps <= K_b <= W, so thread r walks row r, and ALL rows share one pass over the back-pointers: the blocks of
//     F frames are staged exactly as the best path stages them (tgv_fetch / tgv_put, double-buffered through registers), and
//     after the barrier threads 0 .. num_hyps-1 walk the staged block concurrently, each from its own node.  Each leaves its
//     nodes as 16-bit values in an LDS tile of row pitch F + 2 halfwords: (F + 2) / 2 is odd, so the walkers' stores (lanes =
//     rows, one frame) fall into distinct banks, and the write-out's loads (lanes = frames, one row) are consecutive
//     halfwords.  After the block's barrier the workgroup copies the tile to the utterance's node columns in the workspace,
//     [rows][T] uint16, contiguous over t.  Two tiles where they fit beside the two staging buffers (one barrier per block);
//     ONE tile and a second barrier per block where they do not (Kmax = 256 with more than 248 rows, Kmax = 1024 with more
//     than 909): `tiles` is chosen by the host, tgn_tiles.
//  4. write: one wavefront per row, wavefronts striding the rows, padding rows included.  Chunks of 64 frames: lane = frame
//     reads its node, gathers its label, its emission and its transition (the previous label by a lane shift, carried over
//     the chunk edge); nodes / labels go out as coalesced int64 when asked for; tokens / token_frames by ballot + popcount
//     with the base carried over the chunks; emission_scores by a serial sum in frame order over the lanes' values -- the
//     loads do not depend on the sum, and the next chunk's are issued before this chunk's adds.  Then the -1 tails,
//     token_lengths and emission_scores.
// Every output element is written here (no memset), no float atomics, nothing synchronises the host: bit-identical run to
// run and capturable.  Every offset into the workspace and the outputs is 64-bit.
#include "asg_target_graph_path.h"

namespace asg {

namespace {

inline size_t tgn_round16(size_t n) { return (n + 15) & ~(size_t) 15; }
inline int tgn_rows(int Kmax, int nbest) { return nbest < Kmax ? nbest : Kmax; }
inline size_t tgn_tile(int Kmax, int rows) { return (size_t) rows * (tgv_frames(Kmax) + 2) * 2; }
inline size_t tgn_walk_lds(int Kmax, int rows, int tiles) { return kTgRed + 2 * tgv_granules(Kmax) * 16 + tiles * tgn_tile(Kmax, rows); }
inline int tgn_tiles(int Kmax, int rows) { return tgn_walk_lds(Kmax, rows, 2) <= kTgLds ? 2 : 1; }
// [reduction slots 256 B] then the larger of the forward's vectors (the rank's [end Kmax R][order Kmax int] lie in its two v
// vectors) and the walk's [stage 2 x granules x 16 B][tile `tiles` x rows x (F + 2) x 2 B]
inline size_t tgn_lds(int elem, int Kmax, int64_t Emax, int rows) {
    const size_t walk = tgn_walk_lds(Kmax, rows, tgn_tiles(Kmax, rows)), fwd = tg_fwd_lds(elem, Kmax, Emax);
    return fwd > walk ? fwd : walk;
}

// One chunk of row `col` for the write phase: lane = frame c0 + lane.  nd / lab: the node and its label (-1 behind n); pn: the
// node of the frame before (pnd / plab: those of the last frame of the chunk before); e, tv: the emission and the transition
// into this frame (0 where there is none).
template <typename R>
struct TgnChunk {
    int nd, lab, pn;
    R e, tv;
};
template <typename R>
__device__ __forceinline__ TgnChunk<R> tgn_load(const Problem &P, const R *inb, const int *label, const uint16_t *col, int c0, int n,
                                                int pnd, int plab) {
    const int lane = threadIdx.x & 63, t = c0 + lane;
    const bool ok = t < n;
    TgnChunk<R> c;
    c.nd = ok ? (int) col[t] : -1;
    c.lab = ok ? label[c.nd] : -1;
    c.pn = __shfl_up(c.nd, 1);
    int pl = __shfl_up(c.lab, 1);
    if (lane == 0) { c.pn = pnd; pl = plab; }
    c.e = ok ? inb[(int64_t) t * P.is0 + (int64_t) c.lab * P.is2] : R(0);
    c.tv = ok && t > 0 ? ((const R *) P.transition)[(int64_t) c.lab * P.ts0 + (int64_t) pl * P.ts1] : R(0);
    return c;
}

template <typename R, int W>
__global__ void __launch_bounds__(W) target_graph_nbest(Problem P, TargetGraphArgs G, int nbest, int rows, int tiles, uint16_t *bp,
                                                        uint16_t *cols, TargetGraphNBestOut O) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int F = Tgv<W>::F, PITCH = F + 2;
    R *red = (R *) lds;
    const R NINF = Num<R>::ninf();
    const int k = threadIdx.x, b = blockIdx.x, T = P.T, Kmax = G.Kmax;
    const TgView g = tg_view(G, b);
    const int len = g.K > 0 ? tg_len(P.in_len, b, T) : 0;
    const uint16_t *bpb = bp + (int64_t) b * T * Kmax;
    uint16_t *cb = cols + (int64_t) b * rows * T;
    // ---- 1. forward, 2. rank ----
    int num = 0, cur = 0;
    R mine = NINF;                                    // the score of row k
    if (len >= 1) {                                   // (uniform over the workgroup)
        const R c = tgv_forward<R>(P, G, g, b, len, lds, bp + (int64_t) b * T * Kmax);
        R *ev = (R *) (lds + kTgRed);                 // the forward's two v vectors: end [Kmax], order [Kmax]
        int *order = (int *) (ev + Kmax);
        if (k < Kmax) ev[k] = c;
        __syncthreads();
        const bool cand = c > NINF;
        int rank = 0;
#pragma unroll 4
        for (int j = 0; j < g.K; ++j) {               // every lane reads ev[j]: a broadcast
            const R u = ev[j];
            rank += (u > c || (u == c && j < k)) ? 1 : 0;
        }
        if (cand && rank < nbest) order[rank] = k;
        const int cnt = tg_reduce<int, W, false>(cand ? 1 : 0, (int *) red);
        num = cnt < nbest ? cnt : nbest;
        __syncthreads();                              // order is complete
        if (k < num) {
            cur = order[k];
            mine = ev[cur];
        }
    }
    {
        R *sb = (R *) O.scores + (int64_t) b * nbest;
        int64_t *eb = O.end_nodes + (int64_t) b * nbest;
        for (int r = k; r < nbest; r += W) {          // (r < num only at r == k: num <= W)
            sb[r] = r < num ? mine : NINF;
            eb[r] = r < num ? cur : -1;
        }
        if (k == 0) O.num_hyps[b] = num;
    }
    // ---- 3. walk, block by block from the end: thread r < num walks row r ----
    if (num > 0) {                                    // (uniform)
        __syncthreads();                              // order and end are read, the rows of this workgroup are written
        const int n = len;
        const size_t cap = ((size_t) F * Kmax + 14) / 8;
        uint4 *stage = (uint4 *) (lds + kTgRed);      // two buffers of `cap` granules
        uint16_t *tile = (uint16_t *) (stage + 2 * cap);      // `tiles` tiles of rows x PITCH
        const size_t tsz = (size_t) rows * PITCH;
        uint4 r[Tgv<W>::NG];
        const int last = (n - 1) / F;
        {
            const uint16_t *rw = bpb + (int64_t) last * F * Kmax;
            tgv_fetch<W>(rw, (n - last * F) * Kmax, r);
            tgv_put<W>(rw, (n - last * F) * Kmax, r, stage);
        }
        __syncthreads();
        int p = 0;
        for (int j = last; j >= 0; --j, p ^= 1) {
            const int lo = j * F, hi = (lo + F < n ? lo + F : n) - 1;
            const uint16_t *rw = bpb + (int64_t) lo * Kmax, *next = rw - (int64_t) F * Kmax;
            uint16_t *tl = tile + (tiles == 2 ? p * tsz : 0);
            if (j > 0) tgv_fetch<W>(next, F * Kmax, r);            // block j-1: in flight while block j is walked
            if (k < num) {
                const uint16_t *st = (const uint16_t *) (stage + (size_t) p * cap) + (((uintptr_t) rw & 15) >> 1);
                uint16_t *ln = tl + (size_t) k * PITCH;
                for (int t = hi; t >= lo; --t) {
                    ln[t - lo] = (uint16_t) cur;
                    if (t > 0) cur = st[(t - lo) * Kmax + cur];
                }
            }
            if (j > 0) tgv_put<W>(next, F * Kmax, r, stage + (size_t) (p ^ 1) * cap);
            __syncthreads();
            for (int i = k; i < num * F; i += W) {    // lanes = frames of one row
                const int row = i / F, f = i % F;
                if (f <= hi - lo) cb[(int64_t) row * T + lo + f] = tl[(size_t) row * PITCH + f];
            }
            if (tiles == 1) __syncthreads();          // the one tile is copied before the next block is walked into it
        }
    }
    // ---- 4. write: wavefront w takes rows w, w + W/64, ... ----
    __syncthreads();                                  // the node columns of this utterance are written
    const int lane = k & 63;
    const R *inb = (const R *) P.inputs + (int64_t) b * P.is1;
    for (int row = k >> 6; row < nbest; row += W / 64) {           // (uniform over the wavefront)
        const int n = row < num ? len : 0;
        const uint16_t *col = cb + (int64_t) row * T;              // (read only where n > 0: row < num <= rows)
        const int64_t o = ((int64_t) b * nbest + row) * T;
        int64_t *kb = O.tokens + o, *fb = O.token_frames + o;
        int base = 0;
        R a = NINF;
        TgnChunk<R> c = tgn_load<R>(P, inb, g.label, col, 0, n, -1, 0);
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int t = c0 + lane;
            const TgnChunk<R> nx = tgn_load<R>(P, inb, g.label, col, c0 + 64, n, __shfl(c.nd, 63), __shfl(c.lab, 63));
            if (O.nodes && t < n) {
                O.nodes[o + t] = c.nd;
                O.labels[o + t] = c.lab;
            }
            const bool f = t < n && (t == 0 || c.nd != c.pn);
            const unsigned long long mask = __ballot(f);
            if (f) {
                const int at = base + __popcll(mask & ((1ull << lane) - 1));
                kb[at] = c.lab;
                fb[at] = t;
            }
            base += __popcll(mask);
            const int m = n - c0 < 64 ? n - c0 : 64;
            for (int i = 0; i < m; ++i) {             // in frame order; every lane carries the same sum
                const R ei = (R) __shfl(c.e, i), ti = (R) __shfl(c.tv, i);
                a = c0 + i == 0 ? ei : (a + ti) + ei;
            }
            c = nx;
        }
        if (O.nodes)
            for (int t = n + lane; t < T; t += 64) O.nodes[o + t] = O.labels[o + t] = -1;
        for (int t = base + lane; t < T; t += 64) kb[t] = fb[t] = -1;
        if (lane == 0) {
            O.token_lengths[(int64_t) b * nbest + row] = base;
            ((R *) O.emission_scores)[(int64_t) b * nbest + row] = a;
        }
    }
}

template <typename R, int W>
hipError_t tgn_launch(const Problem &P, const TargetGraphArgs &G, int nbest, void *work, const TargetGraphNBestOut &O,
                      hipStream_t stream) {
    const int rows = tgn_rows(G.Kmax, nbest);
    const size_t dyn = tgn_lds(sizeof(R), G.Kmax, G.Emax, rows);
    tg_set_lds((const void *) target_graph_nbest<R, W>, dyn);
    uint16_t *cols = (uint16_t *) ((char *) work + tgn_round16((size_t) P.B * P.T * G.Kmax * 2));
    hipLaunchKernelGGL((target_graph_nbest<R, W>), dim3(P.B), dim3(W), dyn, stream, P, G, nbest, rows, tgn_tiles(G.Kmax, rows),
                       (uint16_t *) work, cols, O);
    return hipGetLastError();
}

}  // namespace

size_t target_graph_nbest_work_bytes(int T, int B, int Kmax, int nbest) {
    return tgn_round16((size_t) B * T * Kmax * 2) + tgn_round16((size_t) B * tgn_rows(Kmax, nbest) * T * 2);
}

template <typename R>
hipError_t launch_target_graph_nbest(const Problem &P, const TargetGraphArgs &G, int nbest, void *work,
                                     const TargetGraphNBestOut &out, hipStream_t stream) {
    if (G.Kmax <= 64) return tgn_launch<R, 64>(P, G, nbest, work, out, stream);
    if (G.Kmax <= 256) return tgn_launch<R, 256>(P, G, nbest, work, out, stream);
    return tgn_launch<R, 1024>(P, G, nbest, work, out, stream);
}

template hipError_t launch_target_graph_nbest<float>(const Problem &, const TargetGraphArgs &, int, void *,
                                                     const TargetGraphNBestOut &, hipStream_t);
template hipError_t launch_target_graph_nbest<double>(const Problem &, const TargetGraphArgs &, int, void *,
                                                      const TargetGraphNBestOut &, hipStream_t);

}  // namespace asg
