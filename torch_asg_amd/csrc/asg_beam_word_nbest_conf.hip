// torch_asg_amd/csrc/asg_beam_word_nbest_conf.hip -- WORD CONFIDENCES and END FRAMES for EVERY ROW of the word-LM beam decoder's
// n-best list, from the lattice the same search kept, on gfx950.  The specification is
// include/asg_hip.h::asg_beam_words_nbest_confidence; tests/beam_word_nbest_conf_ref.py restates it in numpy.
//
// P(w, t) of asg_beam_words_confidence does not depend on the hypothesis: a row only selects which (word, frame) CELLS are read
// out.  Eight launches on one stream, the frame loop of the search in one of them:
//   1  beam_word_conf_search<.., FIN> (asg_beam_word_conf.hip): the search with the decoder's end, which also leaves the last set;
//      its one-best outputs go to the tail of the workspace, as the n-best call's decoder's do.
//   2  beam_word_nbest_kernel (asg_beam_word_nbest.hip) over what it left: the twelve n-best outputs.
//   3  nbest_conf_prep: a wavefront per row collapses the row's column of product states into word_frames (ballot and popcount,
//      as the write stage of the n-best kernel collapses it into words) and appends a query (frame << 32 | word) per word; the
//      workgroup sorts the queries -- a bitonic network in LDS up to kBeamWordNbestConfSortLds of them, the same network over the
//      workspace beyond --, drops the duplicates and leaves the CELLS ascending in (frame, word) with the first cell of every frame.
//   4 - 6  launch_beam_word_loss_lattice, unchanged: U, alpha, Z_K.
//   7  nbest_conf_bwd: the pull of asg_beam_word_conf_pull.h, the text beam_word_conf_bwd compiles, with the ROW SINK.  The cells whose window holds
//      frame t are those of the frames [t - tol, t + tol]: one range of the sorted list, which only moves down with t.  A cell's
//      accumulator is slot (cell index mod ring) of a ring of u64 in LDS, ring the power of two >= nb * (2 tol + 2): a row ends at
//      most one word per frame, so the ranges of two neighbouring frames fit.  The words of the open cells are mirrored in LDS at
//      the same slots; the first cell of each open frame sits in LDS too, so an event is a binary search per open frame over LDS.
//      A 256-bit mask over word mod 256 of every cell's word turns away most events whose word is in no row after one LDS read.
//      A cell that leaves the range is stored as its integer and its slot zeroed.
//   8  nbest_conf_fill: every (row, k) looks its cell up and converts.
// Integer adds only: no order of arrival changes a bit, and a cell shared by rows has one value.  Every output and every
// workspace word that is read is written by these kernels: no memset, no host synchronisation; the call captures and replays.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"
#include "asg_beam_lattice.h"     // subgroup, find_sorted, the butterflies, to_fixed, bwd_front
#include "asg_beam_word_lat.h"    // WordLat: how a pair's edges are walked
#include "asg_beam_word_conf_pull.h"  // the beta pull and 2^54, shared with asg_beam_word_conf.hip
#include "asg_beam_row_sink.h"        // sort_u64, RowSink: shared with asg_beam_nbest_conf.hip

namespace asg {

namespace {

// behind the utterances: what the one-best search writes (scores [B], token and word lengths [B], path / tokens / states /
// lm_states / words / word_frames [6][B][T])
inline size_t tail_bytes(int T, int B) { return 3 * a256((size_t) B * 8) + a256((size_t) 6 * B * T * 8); }

// ---------------------------------------------------------------------------------------------------------------------
// 3: word_frames of every row, the queries, the cells.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kNP) nbest_conf_prep(const int64_t *in_len, const int *label, int sep, int T, int nbest, int nb,
                                                       char *work, size_t per, size_t rows_off, size_t hdr_off, size_t foff_off,
                                                       size_t qk_off, size_t cells_off, long long qcap, const long long *words,
                                                       const long long *wlen, const long long *nhyp, long long *wframes) {
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
        long long *wf = wframes + (ob + r) * T;
        if (r >= nh || len < 1) {
            for (int t = lane; t < T; t += 64) wf[t] = -1;
            continue;
        }
        const long long *wd = words + (ob + r) * T;
        long long nl = wlen[ob + r];
        const int n = (int) (nl < 0 ? 0 : (nl > len ? len : nl));         // (a path of len frames ends at most len words)
        int qb = 0;
        if (lane == 0 && n) qb = atomicAdd(&nq_s, n);                     // where the row's queries go: any order, they are sorted
        qb = __shfl(qb, 0);
        int wbase = 0;
        long long carry = -1;
        for (int c0 = 0; c0 < len; c0 += 64) {
            const int t = c0 + lane;
            long long cur = -1;
            if (t < len) cur = label[cols[(size_t) t * nb + r]];
            long long prv = __shfl_up(cur, 1);
            if (lane == 0) prv = carry;
            const bool wend = t < len && t >= 1 && cur == sep && prv != sep;
            const unsigned long long mw = __ballot(wend);
            const int k = wbase + __popcll(mw & ((1ull << lane) - 1ull));
            if (wend && k < n) {
                wf[k] = t;
                qk[qb + k] = ((unsigned long long) t << 32) | (unsigned) wd[k];
            }
            wbase += __popcll(mw);
            carry = __shfl(cur, 63);
        }
        if (wbase > n) wbase = n;                                         // (cannot happen: the n-best kernel counted the same edges)
        if (lane == 0 && wbase < n) {                                     // the word of the final step
            wf[wbase] = len;
            qk[qb + wbase] = ((unsigned long long) len << 32) | (unsigned) wd[wbase];
        }
        if (wbase < n) ++wbase;
        for (int t = wbase + lane; t < T; t += 64) wf[t] = -1;
        for (int k = wbase + lane; k < n; k += 64) qk[qb + k] = ~0ull;    // (nor this: a row has exactly n words)
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
// 7: beta with the row sink.  Dynamic LDS: [nq u64 M][nb R M][pad to 16][fo int32, filter: 1024 bytes][ring u64][mirror int32].
// The pull is asg_beam_word_conf_pull.h's, the text beam_word_conf_bwd compiles.
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kBL) nbest_conf_bwd(Problem P, typename WordLat<R>::Args args, char *work, size_t beta_off,
                                                      size_t hdr_off, size_t foff_off, size_t cells_off, size_t acc_off,
                                                      const R *Zs, int tol, int ring_mask) {
    using KeyT = unsigned long long;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int M = args.lay.M, T = P.T;
    KeyT *nq = (KeyT *) lds;                                                   // [M] U_t
    R *nb = (R *) (lds + (size_t) M * sizeof(KeyT));                           // [M] beta[t] of U_t
    unsigned char *head = lds + bwd_front(sizeof(R), sizeof(KeyT), M);
    int *fo = (int *) head;                                                    // [2 tol + 2] first cell of frames lo .. lo + 2 tol + 1
    unsigned *filt = (unsigned *) (head + kSinkFiltOff);                       // [8]
    unsigned long long *ring = (unsigned long long *) (head + kSinkFixed);     // [ring]
    int *mw = (int *) (ring + (size_t) ring_mask + 1);                         // [ring] the word of the cell in the slot
    const int tid = threadIdx.x, b = blockIdx.x;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    const R Z = Zs[b];
    char *wb = work + (size_t) b * args.lay.per;
    const int *foff = (const int *) (wb + foff_off);
    const KeyT *cells = (const KeyT *) (wb + cells_off);
    KeyT *acc = (KeyT *) (wb + acc_off);
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
    beam_word_conf_pull<R>(P, args, wb, beta_off, Z, len, -tol - 1, nq, nb, sink);
}

// ---------------------------------------------------------------------------------------------------------------------
// 8: word_confidences [nbest][T] of one utterance: the cell of (word_frames, words), converted; 0 behind the words.
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kNP) nbest_conf_fill(const int64_t *in_len, int T, int nbest, int nb, const char *work, size_t per,
                                                       size_t hdr_off, size_t cells_off, size_t acc_off, const R *Zs,
                                                       const long long *words, const long long *wlen, const long long *nhyp,
                                                       const long long *wframes, R *conf) {
    const int b = blockIdx.x;
    const int len = clamp_len(in_len, b, T);
    const char *wb = work + (size_t) b * per;
    const unsigned long long *cells = (const unsigned long long *) (wb + cells_off);
    const unsigned long long *acc = (const unsigned long long *) (wb + acc_off);
    const int nc = *(const int *) (wb + hdr_off);
    const int64_t ob = (int64_t) b * nbest;
    const long long nhl = nhyp[b];
    const bool live = len >= 1 && Zs[b] > Num<R>::ninf() && nc >= 1;           // (else nbest_conf_bwd wrote no accumulator)
    const int nh = live ? (int) (nhl < 0 ? 0 : (nhl > nb ? nb : nhl)) : 0;
    for (int64_t x = (int64_t) blockIdx.y * kNP + threadIdx.x; x < (int64_t) nbest * T; x += (int64_t) gridDim.y * kNP) {
        const int r = (int) (x / T), k = (int) (x % T);
        R c = R(0);
        if (r < nh && k < len && k < wlen[ob + r]) {
            const long long t = wframes[(ob + r) * T + k];
            const unsigned long long key = ((unsigned long long) t << 32) | (unsigned) words[(ob + r) * T + k];
            const int pos = t >= 1 ? find_sorted(cells, nc, key) : -1;
            if (pos >= 0) c = (R) ((double) acc[pos] * (1.0 / kConfScale));
        }
        conf[ob * T + x] = c;
    }
}

}  // namespace

bool beam_word_nbest_conf_fits(int elem, int T, int K, int nbest, int tol) {
    const size_t nb = (size_t) (nbest < K ? nbest : K);
    if (nb * (size_t) T > ((size_t) 1 << 30)) return false;
    return sink_lds(elem, 8, K, beam_word_nbest_conf_ring(K, nbest, tol)) <= kBLLds;
}

BeamWordNbestConfLayout beam_word_nbest_conf_layout(int elem, int T, int K, int cap, int nbest) {
    BeamWordNbestConfLayout l{};
    l.nb = nbest < K ? nbest : K;
    l.conf = beam_word_conf_layout(elem, T, K, cap);
    l.qcap = p2_size((size_t) l.nb * T);
    size_t off = l.conf.per;
    l.fin = off;   off += a256(8 + (size_t) K * (elem + 8));
    l.rows = off;  off += a256((size_t) T * l.nb * 4);
    l.hdr = off;   off += 256;
    l.foff = off;  off += a256(((size_t) T + 2) * 4);
    l.qk = off;    off += a256(l.qcap * 8);
    l.cells = off; off += a256((size_t) l.nb * T * 8);
    l.acc = off;   off += a256((size_t) l.nb * T * 8);
    l.per = off;
    l.conf.per = l.per;
    l.conf.lat.per = l.per;
    return l;
}

size_t beam_word_nbest_conf_work_bytes(int elem, int T, int B, int K, int cap, int nbest) {
    return (size_t) B * beam_word_nbest_conf_layout(elem, T, K, cap, nbest).per + tail_bytes(T, B);
}

template <typename R>
hipError_t launch_beam_word_nbest_conf(const Problem &P0, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                       const WordLookArgs *LA, int K, double theta, int nbest, int tol, void *work, void *scores,
                                       void *emission_scores, void *graph_scores, void *lm_scores, long long *path,
                                       long long *tokens, long long *tlen, long long *states, long long *lm_states,
                                       long long *words, long long *wlen, long long *num_hyps, long long *word_frames,
                                       void *word_conf, void *normalisers, hipStream_t stream) {
    Problem P = P0;
    P.targets = nullptr;                                                         // the lattice of the search alone: U_t = A_t
    P.tg_len = nullptr;
    const int T = P.T, B = P.B;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const BeamWordNbestConfLayout lay = beam_word_nbest_conf_layout(sizeof(R), T, K, cap, nbest);
    char *w = (char *) work, *tail = w + (size_t) B * lay.per;
    const size_t bb = a256((size_t) B * 8), BT = (size_t) B * T;
    long long *wide = (long long *) (tail + 3 * bb);        // path, tokens, states, lm_states, words, word_frames of the one best
    hipError_t e = launch_beam_word_conf_search<R>(P, G, BG, LM, LA, K, theta, work, lay.per, lay.conf.lat.cnt, lay.fin, tail, wide,
                                                   wide + BT, (long long *) (tail + bb), wide + 2 * BT, wide + 3 * BT, wide + 4 * BT,
                                                   (long long *) (tail + 2 * bb), wide + 5 * BT, stream);
    if (e != hipSuccess) return e;
    BeamWordNbestSrc src{};
    src.base = w; src.per = lay.per; src.set_off = lay.fin + 8; src.na_off = lay.fin; src.pos_off = 0; src.ovf_off = 0;
    src.cols = w + lay.rows; src.cols_per = lay.per; src.Tw = T; src.nb = lay.nb;
    e = launch_beam_word_nbest_over<R>(P, G, BG, LM, LA, src, K, nbest, scores, emission_scores, graph_scores, lm_scores, path, tokens,
                                       tlen, states, lm_states, words, wlen, num_hyps, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nbest_conf_prep, dim3(B), dim3(kNP), 0, stream, P.in_len, G.label, LM.sep, T, nbest, lay.nb, w, lay.per,
                       lay.rows, lay.hdr, lay.foff, lay.qk, lay.cells, (long long) lay.qcap, (const long long *) words,
                       (const long long *) wlen, (const long long *) num_hyps, word_frames);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_beam_word_loss_lattice<R>(P, G, BG, LM, lay.conf.lat, K, true, work, normalisers, stream);
    if (e != hipSuccess) return e;
    const size_t ring = beam_word_nbest_conf_ring(K, nbest, tol);
    const size_t dyn = sink_lds(sizeof(R), 8, lay.conf.lat.M, ring);
    set_lds((const void *) nbest_conf_bwd<R>, dyn);
    hipLaunchKernelGGL((nbest_conf_bwd<R>), dim3(B), dim3(kBL), dyn, stream, P, typename WordLat<R>::Args{G, BG, LM, lay.conf.lat}, w,
                       lay.conf.beta, lay.hdr, lay.foff, lay.cells, lay.acc, (const R *) normalisers, tol, (int) (ring - 1));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t cellsn = (size_t) nbest * T;
    const unsigned gy = (unsigned) (cellsn < 8 * (size_t) kNP ? 1 : (cellsn / (8 * (size_t) kNP) > 64 ? 64 : cellsn / (8 * (size_t) kNP)));
    hipLaunchKernelGGL((nbest_conf_fill<R>), dim3(B, gy), dim3(kNP), 0, stream, P.in_len, T, nbest, lay.nb, (const char *) w, lay.per,
                       lay.hdr, lay.cells, lay.acc, (const R *) normalisers, (const long long *) words, (const long long *) wlen,
                       (const long long *) num_hyps, (const long long *) word_frames, (R *) word_conf);
    return hipGetLastError();
}

#define ASG_WORD_NBEST_CONF_INST(R)                                                                                              \
    template hipError_t launch_beam_word_nbest_conf<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &,              \
                                                       const WordLmArgs &, const WordLookArgs *, int, double, int, int, void *, \
                                                       void *, void *, void *, void *, long long *, long long *, long long *,   \
                                                       long long *, long long *, long long *, long long *, long long *,         \
                                                       long long *, void *, void *, hipStream_t);
ASG_WORD_NBEST_CONF_INST(float)
ASG_WORD_NBEST_CONF_INST(double)
#undef ASG_WORD_NBEST_CONF_INST

}  // namespace asg
