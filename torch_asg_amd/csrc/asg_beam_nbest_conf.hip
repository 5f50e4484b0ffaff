// torch_asg_amd/csrc/asg_beam_nbest_conf.hip -- TOKEN CONFIDENCES and START FRAMES for EVERY ROW of the token-graph beam decoder's
// n-best list, from the lattice the same search kept, on gfx950.  The specification is
// include/asg_hip.h::asg_beam_graph_nbest_confidence; tests/beam_nbest_conf_ref.py restates it in numpy.
//
// P(i, t) of asg_beam_graph_confidence does not depend on the hypothesis: a row only selects which (frame, label) CELLS are read
// out.  Eight launches on one stream, the frame loop of the search in one of them:
//   1 - 4  launch_beam_loss_lattice (asg_beam_loss.hip), unchanged kernels: beam_graph_kernel asked for |A_t| of every frame AND
//      for its last set (cnt_off and fin_off are independent), the target walk without a target, U_t = A_t sorted, alpha, Z_K.
//      The search's one-best outputs go to the tail of the workspace, as the n-best call's do.
//   5  beam_nbest_kernel (asg_beam_nbest.hip) over what the search left: the eight n-best outputs and the [T][nb] column block.
//   6  beam_nbest_conf_prep: a wavefront per row collapses the row's column of product states into token_frames (ballot and
//      popcount, as the write stage of the n-best kernel collapses it into tokens) and appends a query (frame << 32 | label) per
//      token; the workgroup sorts the queries -- a bitonic network in LDS up to kBeamWordNbestConfSortLds of them, the same
//      network over the workspace beyond --, drops the duplicates and leaves the CELLS ascending in (frame, label) with the first
//      cell of every frame (asg_beam_row_sink.h, asg_beam_cells.inc).  Cells live at frames 0 .. len - 1.
//   7  beam_nbest_conf_bwd: the pull of asg_beam_conf_pull.h, the text beam_conf_bwd compiles, with the ROW SINK of
//      asg_beam_row_sink.h, the sink of the word-LM rows: accumulators in an LDS ring of the power of two >= nb * (2 tol + 2)
//      slots -- a row starts at most one token per frame --, the labels of the open cells mirrored beside them, a 256-bit filter
//      over label mod 256.
//   8  beam_nbest_conf_fill: every (row, k) looks its cell up and converts with beam_conf_bwd's expression.
// Integer adds only: no order of arrival changes a bit, a cell shared by rows has one value, and row 0 -- the same events
// through the same expressions into the same integer sums -- has asg_beam_graph_confidence's bits.  Every output and every
// workspace word that is read is written by these kernels: no memset, no host synchronisation; the call captures and replays.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_lattice.h"     // subgroup, find_sorted, the butterflies, to_fixed, bwd_front
#include "asg_beam_token_lat.h"   // TokenLat: how a product state's edges are walked
#include "asg_beam_conf_pull.h"   // the beta pull, shared with asg_beam_conf.hip
#include "asg_beam_row_sink.h"    // sort_u64, RowSink: shared with asg_beam_word_nbest_conf.hip

namespace asg {

namespace {

static_assert(kBeamConfMaxTol == kBeamWordConfMaxTol, "the head of RowSink is sized by the word call's tolerance");

// ---------------------------------------------------------------------------------------------------------------------
// 6: token_frames of every row, the queries, the cells.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kNP) beam_nbest_conf_prep(const int64_t *in_len, const int *label, int T, int nbest, int nb,
                                                            char *work, size_t per, size_t rows_off, size_t hdr_off,
                                                            size_t foff_off, size_t qk_off, size_t cells_off, long long qcap,
                                                            const long long *tlen, const long long *nhyp, long long *tframes) {
    __shared__ unsigned long long sq[kBeamWordNbestConfSortLds];
    __shared__ int nq_s, wsum[kNP / 64], run_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int len = clamp_len(in_len, b, T);
    char *wb = work + (size_t) b * per;
    const int *cols = (const int *) (wb + rows_off);                      // [T][nb]
    int *hdr = (int *) (wb + hdr_off), *foff = (int *) (wb + foff_off);
    unsigned long long *qk = (unsigned long long *) (wb + qk_off), *cells = (unsigned long long *) (wb + cells_off);
    const int64_t ob = (int64_t) b * nbest;
    long long nhl = nhyp[b];
    const int nh = (int) (nhl < 0 ? 0 : (nhl > nb ? nb : nhl));
    if (tid == 0) nq_s = 0;
    __syncthreads();
    // ---- one wavefront per row
    for (int r = wave; r < nbest; r += kNP / 64) {
        long long *tf = tframes + (ob + r) * T;
        if (r >= nh || len < 1) {
            for (int t = lane; t < T; t += 64) tf[t] = -1;
            continue;
        }
        long long nl = tlen[ob + r];
        const int n = (int) (nl < 0 ? 0 : (nl > len ? len : nl));         // (a path of len frames starts at most len tokens)
        int qb = 0;
        if (lane == 0 && n) qb = atomicAdd(&nq_s, n);                     // where the row's queries go: any order, they are sorted
        qb = __shfl(qb, 0);
        int base = 0;
        long long carry = -1;
        for (int c0 = 0; c0 < len; c0 += 64) {
            const int t = c0 + lane;
            long long cur = -1;
            if (t < len) cur = label[cols[(size_t) t * nb + r]];
            long long prv = __shfl_up(cur, 1);
            if (lane == 0) prv = carry;
            const bool keep = t < len && cur != prv;
            const unsigned long long m = __ballot(keep);
            const int k = base + __popcll(m & ((1ull << lane) - 1ull));
            if (keep && k < n) {
                tf[k] = t;
                qk[qb + k] = ((unsigned long long) t << 32) | (unsigned) cur;
            }
            base += __popcll(m);
            carry = __shfl(cur, 63);
        }
        if (base > n) base = n;                                           // (cannot happen: the n-best kernel counted the same runs)
        for (int t = base + lane; t < T; t += 64) tf[t] = -1;
        for (int k = base + lane; k < n; k += 64) qk[qb + k] = ~0ull;     // (nor this: a row has exactly n tokens)
    }
    __threadfence_block();
    __syncthreads();
    const int nq = nq_s;
    // ---- sort: in LDS while the queries fit, over the workspace beyond
    int P2 = 2;
    while (P2 < nq) P2 *= 2;                                              // (<= qcap: nq <= nb * T)
    const bool in_lds = P2 <= kBeamWordNbestConfSortLds;
    unsigned long long *v = in_lds ? sq : qk;
    if (in_lds) for (int x = tid; x < P2; x += kNP) sq[x] = x < nq ? qk[x] : ~0ull;
    else for (long long x = nq + tid; x < P2 && x < qcap; x += kNP) qk[x] = ~0ull;
    __threadfence_block();
    __syncthreads();
    if (nq > 1) sort_u64(v, P2);
#include "asg_beam_cells.inc"   // the cells and the first cell of every frame 0 .. T + 1
}

// ---------------------------------------------------------------------------------------------------------------------
// 7: beta with the row sink.  Dynamic LDS: [nb R M][nq int M][pad to 16][fo int32, filter: 1024 bytes][ring u64][mirror int32].
// The pull is asg_beam_conf_pull.h's, the text beam_conf_bwd compiles.
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kBL) beam_nbest_conf_bwd(Problem P, typename TokenLat<R>::Args args, char *work, size_t beta_off,
                                                           size_t hdr_off, size_t foff_off, size_t cells_off, size_t acc_off,
                                                           const R *Zs, int tol, int ring_mask) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int M = args.lay.M, T = P.T;
    R *nb = (R *) lds;                                                         // [M] beta[t] of U_t
    int *nq = (int *) (lds + (size_t) M * sizeof(R));                          // [M] U_t
    unsigned char *head = lds + bwd_front(sizeof(R), 4, M);
    int *fo = (int *) head;                                                    // [2 tol + 2] first cell of frames lo .. lo + 2 tol + 1
    unsigned *filt = (unsigned *) (head + kSinkFiltOff);                       // [8]
    unsigned long long *ring = (unsigned long long *) (head + kSinkFixed);     // [ring]
    int *mw = (int *) (ring + (size_t) ring_mask + 1);                         // [ring] the label of the cell in the slot
    const int tid = threadIdx.x, b = blockIdx.x;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    const R Z = Zs[b];
    char *wb = work + (size_t) b * args.lay.per;
    const int *foff = (const int *) (wb + foff_off);
    const unsigned long long *cells = (const unsigned long long *) (wb + cells_off);
    unsigned long long *acc = (unsigned long long *) (wb + acc_off);
    const int nc = *(const int *) (wb + hdr_off);
    if (!(len >= 1 && Z > NINF) || nc < 1) return;                             // (the fill stage then reads no accumulator)
    for (int x = tid; x <= ring_mask; x += kBL) ring[x] = 0ull;
    if (tid < 8) filt[tid] = 0u;
    __syncthreads();
    for (int c = tid; c < nc; c += kBL) {
        const unsigned w = (unsigned) cells[c];
        atomicOr(&filt[(w & 255u) >> 5], 1u << (w & 31u));
    }
    RowSink sink;
    sink.foff = foff; sink.cells = cells; sink.acc = acc; sink.ring = ring; sink.mw = mw; sink.fo = fo; sink.filt = filt;
    sink.tol = tol; sink.T = T; sink.ring_mask = ring_mask; sink.ca = sink.cb = nc; sink.nfr = 0;
    beam_conf_pull<R>(P, args, wb, beta_off, Z, len, -tol - 1, nq, nb, sink);
}

// ---------------------------------------------------------------------------------------------------------------------
// 8: token_confidences [nbest][T] of one utterance: the cell of (token_frames, tokens), converted; 0 behind the tokens.
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kNP) beam_nbest_conf_fill(const int64_t *in_len, int T, int nbest, int nb, const char *work,
                                                            size_t per, size_t hdr_off, size_t cells_off, size_t acc_off,
                                                            const R *Zs, const long long *tokens, const long long *tlen,
                                                            const long long *nhyp, const long long *tframes, R *conf) {
    const int b = blockIdx.x;
    const int len = clamp_len(in_len, b, T);
    const char *wb = work + (size_t) b * per;
    const unsigned long long *cells = (const unsigned long long *) (wb + cells_off);
    const unsigned long long *acc = (const unsigned long long *) (wb + acc_off);
    const int nc = *(const int *) (wb + hdr_off);
    const int64_t ob = (int64_t) b * nbest;
    const long long nhl = nhyp[b];
    const bool live = len >= 1 && Zs[b] > Num<R>::ninf() && nc >= 1;           // (else beam_nbest_conf_bwd wrote no accumulator)
    const int nh = live ? (int) (nhl < 0 ? 0 : (nhl > nb ? nb : nhl)) : 0;
    for (int64_t x = (int64_t) blockIdx.y * kNP + threadIdx.x; x < (int64_t) nbest * T; x += (int64_t) gridDim.y * kNP) {
        const int r = (int) (x / T), k = (int) (x % T);
        R c = R(0);
        if (r < nh && k < len && k < tlen[ob + r]) {
            const long long t = tframes[(ob + r) * T + k];
            const unsigned long long key = ((unsigned long long) t << 32) | (unsigned) tokens[(ob + r) * T + k];
            const int pos = t >= 0 ? find_sorted(cells, nc, key) : -1;
            if (pos >= 0) c = (R) ((double) acc[pos] * (1.0 / kConfScale));
        }
        conf[ob * T + x] = c;
    }
}

}  // namespace

bool beam_nbest_conf_fits(int elem, int T, int K, int nbest, int tol) {
    const size_t nb = (size_t) (nbest < K ? nbest : K);
    if (nb * (size_t) T > ((size_t) 1 << 30)) return false;
    return sink_lds(elem, 4, K, beam_word_nbest_conf_ring(K, nbest, tol)) <= kBLLds;
}

BeamNbestConfLayout beam_nbest_conf_layout(int elem, int T, int Q, int K, int cap, int nbest) {
    BeamNbestConfLayout l{};
    l.nb = nbest < K ? nbest : K;
    l.conf = beam_conf_layout(elem, T, Q, K, cap);
    l.qcap = p2_size((size_t) l.nb * T);
    size_t off = l.conf.per;
    l.nbest.nb = l.nb;
    l.nbest.fin = off;  off += a256(8 + (size_t) K * elem);
    l.nbest.rows = off; off += a256((size_t) T * l.nb * 4);
    l.hdr = off;   off += 256;
    l.foff = off;  off += a256(((size_t) T + 2) * 4);
    l.qk = off;    off += a256(l.qcap * 8);
    l.cells = off; off += a256((size_t) l.nb * T * 8);
    l.acc = off;   off += a256((size_t) l.nb * T * 8);
    l.per = off;
    l.nbest.per = l.per;
    l.conf.per = l.per;
    l.conf.lat.per = l.per;
    return l;
}

size_t beam_nbest_conf_work_bytes(int elem, int T, int B, int Q, int K, int cap, int nbest) {
    return (size_t) B * beam_nbest_conf_layout(elem, T, Q, K, cap, nbest).per + beam_loss_tail_bytes(T, B);
}

template <typename R>
hipError_t launch_beam_nbest_conf(const Problem &P0, const GraphArgs &G, const BeamGraphArgs &BG, const BeamLossArgs &L, int K,
                                  double theta, int nbest, int tol, void *work, void *scores, void *emission_scores,
                                  void *graph_scores, long long *path, long long *tokens, long long *tlen, long long *states,
                                  long long *num_hyps, long long *token_frames, void *token_conf, void *normalisers,
                                  hipStream_t stream) {
    Problem P = P0;
    P.targets = nullptr;                                                         // the lattice of the search alone: U_t = A_t
    P.tg_len = nullptr;
    const int T = P.T, B = P.B;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const BeamNbestConfLayout lay = beam_nbest_conf_layout(sizeof(R), T, G.Q, K, cap, nbest);
    char *w = (char *) work, *tail = w + (size_t) B * lay.per;
    const size_t bb = a256((size_t) B * 8), BT = (size_t) B * T;
    long long *btl = (long long *) (tail + bb), *bpa = (long long *) (tail + 2 * bb);     // the one best: lengths, path / tokens / states
    hipError_t e = launch_beam_loss_lattice<R>(P, G, BG, L, lay.conf.lat, K, theta, true, work, normalisers, tail, bpa, bpa + BT, btl,
                                               bpa + 2 * BT, lay.nbest.fin, stream);
    if (e != hipSuccess) return e;
    e = launch_beam_nbest_over<R>(P, G, BG, lay.nbest, K, nbest, work, scores, emission_scores, graph_scores, path, tokens, tlen,
                                  states, num_hyps, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beam_nbest_conf_prep, dim3(B), dim3(kNP), 0, stream, P.in_len, G.label, T, nbest, lay.nb, w, lay.per,
                       lay.nbest.rows, lay.hdr, lay.foff, lay.qk, lay.cells, (long long) lay.qcap, (const long long *) tlen,
                       (const long long *) num_hyps, token_frames);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t ring = beam_word_nbest_conf_ring(K, nbest, tol);
    const size_t dyn = sink_lds(sizeof(R), 4, lay.conf.lat.M, ring);
    set_lds((const void *) beam_nbest_conf_bwd<R>, dyn);
    hipLaunchKernelGGL((beam_nbest_conf_bwd<R>), dim3(B), dim3(kBL), dyn, stream, P, typename TokenLat<R>::Args{G, BG, lay.conf.lat}, w,
                       lay.conf.beta, lay.hdr, lay.foff, lay.cells, lay.acc, (const R *) normalisers, tol, (int) (ring - 1));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t cellsn = (size_t) nbest * T;
    const unsigned gy = (unsigned) (cellsn < 8 * (size_t) kNP ? 1 : (cellsn / (8 * (size_t) kNP) > 64 ? 64 : cellsn / (8 * (size_t) kNP)));
    hipLaunchKernelGGL((beam_nbest_conf_fill<R>), dim3(B, gy), dim3(kNP), 0, stream, P.in_len, T, nbest, lay.nb, (const char *) w,
                       lay.per, lay.hdr, lay.cells, lay.acc, (const R *) normalisers, (const long long *) tokens,
                       (const long long *) tlen, (const long long *) num_hyps, (const long long *) token_frames, (R *) token_conf);
    return hipGetLastError();
}

#define ASG_BEAM_NBEST_CONF_INST(R)                                                                                            \
    template hipError_t launch_beam_nbest_conf<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const BeamLossArgs &, \
                                                  int, double, int, int, void *, void *, void *, void *, long long *, long long *, \
                                                  long long *, long long *, long long *, long long *, void *, void *, hipStream_t);
ASG_BEAM_NBEST_CONF_INST(float)
ASG_BEAM_NBEST_CONF_INST(double)
#undef ASG_BEAM_NBEST_CONF_INST

}  // namespace asg
