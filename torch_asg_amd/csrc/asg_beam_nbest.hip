// torch_asg_amd/csrc/asg_beam_nbest.hip -- the N BEST final hypotheses of the beam search of asg_beam_graph.hip, each with its
// score split into the acoustic part (emissions and transitions) and the graph part (automaton weights, token_score, final
// weight), on gfx950.  The specification is include/asg_hip.h::asg_beam_decode_graph_nbest; tests/beam_nbest_ref.py restates it.
//
// The token automaton is deterministic, so the survivors of the last frame carry different transcripts: the n best of them by
// end = v + final_w (q ascending on a tie) are n distinct hypotheses, and the search has already left every back-pointer of
// each on the device.  Two launches on one stream:
//   1  beam_graph_kernel as the decoder runs it (the same device code, so the same sets and back-pointers bit for bit), asked
//      to leave |A_{len-1}| and the values of that set beside its [T][K] lists;
//   2  beam_nbest_kernel, one 1024-thread workgroup per utterance:
//      sort     (~key of end, q << 16 | slot) of the last set in LDS, padded to a power of two with all-ones entries, through a
//               fixed bitonic network, ascending: end descending, then q ascending; states without a finite end sort behind
//               every candidate.  A power of two >= K entries of 12 / 16 bytes: 128 KiB at K = 8192 in float64.
//      walk     one lane per hypothesis follows bs / bq backwards into its column of the frame-major int32 [T][nb] rows of the
//               utterance's workspace (neighbouring lanes store neighbouring words), then forwards again for the two sums: the
//               emission and transition of every frame, and start weight, the weight of every edge taken -- found by binary
//               search for the target in the source's outgoing CSR row, whose targets ascend -- and final weight.  Adds only,
//               in frame order.  Strips of 1024 hypotheses.
//      write    one wavefront per hypothesis turns its column into path / states (when they were asked for) and collapses
//               the labels into tokens with the ballot and popcount routine of the decoders; the same wavefronts fill the
//               padding rows.
// Every output, padding row and scratch word that is read is written by these kernels: no memset, no copy, so a call captures
// and replays.  No atomics on values: results are bit-identical run to run.
//
// The same kernel serves the two streams of the family, which hold their search in a state: told where the set, the header and the
// rows live (asg_kernels.h, BeamNbestSrc), it runs alone over a state of asg_beam_stream.hip (asg_beam_stream_nbest: `final` or
// the n best prefixes, no emission sum) or of asg_beam_window.hip (asg_beam_window_nbest: the rows are a ring, so a hypothesis
// is the uncommitted tail of its chain, and there are no sums).  Sort, walk and write are one text for the three sources.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_window_common.h"   // the window's header and its clamps, the ring's step (and asg_beam_frame.h)

namespace asg {

namespace {

constexpr int kNT = 1024;          // workgroup (kSlotBits, q << 16 | slot with K <= 2^16 slots and q < 2^31, is asg_beam_frame.h's)

// behind the utterances: what the beam search writes besides its sets (scores [B], lengths [B], path / tokens / states [3][B][T])
inline size_t tail_bytes(int T, int B) { return 2 * a256((size_t) B * 8) + a256((size_t) 3 * B * T * 8); }

template <typename U>
__device__ __forceinline__ bool pair_less(U ka, unsigned long long qa, U kb, unsigned long long qb) {
    return ka < kb || (ka == kb && qa < qb);
}

// SRC says where the search lives (asg_kernels.h, BeamNbestSrc).  What differs by source, and nothing else:
//   one-shot   the last set beside the rows, its states in row len-1, the length from the problem; always final; all three sums.
//   stream     the stored set and the header of asg_beam_stream.hip; `final` or the prefix (key and score are v itself,
//              graph_scores ends without the final weight); no emissions, so the walk reads neither P.inputs nor the transitions;
//              frames and status as beam_stream_result_kernel writes them.
//   window     the stored set and the header of asg_beam_window.hip; the rows are a ring, so a row is the TAIL base .. pos-1 of
//              its chain, column t = frame base + t, at most W steps; the collapse starts from the header's carry; no sums (the
//              edge into frame `base` needs the state of frame base-1, whose row may be gone); frames, committed and status as
//              beam_window_result_kernel writes them.
// The state of a stream is only read.
template <typename R, int SRC>
__global__ void __launch_bounds__(kNT) beam_nbest_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, BeamNbestSrc src, int K,
                                                         int cap, int nbest, int P2max, int final, R *scores, R *escores, R *gscores,
                                                         long long *path, long long *tokens, long long *tlen,
                                                         long long *states, long long *nhyp, long long *frames,
                                                         long long *committed, long long *status) {
    using KT = Key<R>;
    using U = typename KT::U;
    constexpr bool kShot = SRC == kBeamNbestShot, kWin = SRC == kBeamNbestWindow;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int ncand;
    unsigned long long *sq = (unsigned long long *) lds;                  // [P2max] q << 16 | slot
    U *sk = (U *) (sq + P2max);                                           // [P2max] ~key of end
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int T = src.Tw, nb = src.nb;                                    // rows of bq / bs, and the width of the wide outputs
    const R NINF = Num<R>::ninf();
    const bool fin = kShot || final != 0;                                 // with the final weights; a stream may ask for prefixes
    const R *sw = (const R *) g.start_w, *fw = (const R *) g.final_w, *ow = (const R *) bg.ow;
    const int2 *oarc = (const int2 *) bg.oarc;
    const char *wb = src.base + (size_t) b * src.per;
    const BeamWorkLayout wl = beam_work_layout(sizeof(R), T, g.Q, K, cap);
    const int *bq = (const int *) (wb + wl.bq), *bs = (const int *) (wb + wl.bs);            // [T][K] what the search left
    int *rows = (int *) (src.cols + (size_t) b * src.cols_per);                              // [T][nb]
    const int64_t ob = (int64_t) b * nbest;                                                  // the slot's first output row

    // ---- where the set is, how many frames a row has, and what the collapse starts from
    int len, na, row_top = 0;                                             // row_top: the ring's row of frame pos-1
    long long carry0 = -1;
    const R *set_v;
    const int *set_q;
    if constexpr (kShot) {
        len = clamp_len(P.in_len, b, T);
        na = len >= 1 ? *(const int *) (wb + src.fin) : 0;
        set_v = (const R *) (wb + src.fin + 8);
        set_q = bq + (size_t) (len >= 1 ? len - 1 : 0) * K;
    } else {
        set_v = (const R *) (wb + src.set);
        set_q = (const int *) (set_v + K);
        if constexpr (kWin) {
            const TokenWinHdr *hdr = (const TokenWinHdr *) (wb + src.hdr);
            long long pos = hdr->pos, base = hdr->base;
            na = hdr->na;
            window_header(pos, base, na, K);
            if (tid == 0) {
                frames[b] = pos;
                committed[b] = base;
                status[b] = (hdr->status & 1) | (pos >= 1 && na == 0 ? 2 : 0);
            }
            base = window_live_base(pos, base, T);                        // (a set that is not empty has pos <= base + W)
            len = na > 0 ? (int) (pos - base) : 0;                        // 0 .. W: the tail may be empty, and its row still counts
            row_top = pos >= 1 ? (int) ((pos - 1) % T) : 0;
            carry0 = hdr->carry;
        } else {
            const int *hdr = (const int *) (wb + src.hdr);
            len = hdr[0];
            len = len < 0 ? 0 : (len > T ? T : len);
            na = len >= 1 ? hdr[1] : 0;
            if (tid == 0) { frames[b] = len; status[b] = hdr[2] != 0; }
        }
    }
    na = na < 0 ? 0 : (na > K ? K : na);
    int P2 = 1;
    while (P2 < na) P2 *= 2;                                              // (<= P2max: na <= K)
    if (tid == 0) ncand = 0;
    __syncthreads();
    // ---- the candidates of the last set
    for (int x0 = 0; x0 < P2; x0 += kNT) {
        const int x = x0 + tid;
        U ik = ~(U) 0;
        unsigned long long qs = ~0ull;
        bool cand = false;
        if (x < na) {
            int q = set_q[x];
            if constexpr (!kShot) q = (unsigned) q < (unsigned) g.Q ? q : 0;
            const R end = fin ? set_v[x] + fw[q] : set_v[x];
            cand = end > NINF;
            ik = cand ? (U) ~KT::enc(end) : ~(U) 0;
            qs = ((unsigned long long) (unsigned) q << kSlotBits) | (unsigned) x;
        }
        if (x < P2) { sk[x] = ik; sq[x] = qs; }
        const unsigned long long m = __ballot(cand);
        if (lane == 0 && m) atomicAdd(&ncand, __popcll(m));
    }
    __syncthreads();
    // ---- bitonic network, ascending in (~key, q)
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = tid; x < P2; x += kNT) {
                const int y = x ^ j;
                if (y > x) {
                    const U ka = sk[x], kb = sk[y];
                    const unsigned long long qa = sq[x], qb = sq[y];
                    const bool up = (x & k) == 0;
                    if (pair_less(kb, qb, ka, qa) == up) { sk[x] = kb; sk[y] = ka; sq[x] = qb; sq[y] = qa; }
                }
            }
            __syncthreads();
        }
    const int nh = ncand < nbest ? ncand : nbest;                         // (<= na <= K, so <= nb)
    if (tid == 0) nhyp[b] = nh;

    // ---- one lane per hypothesis: backwards through the slots, forwards for the sums
    for (int r = tid; r < nh; r += kNT) {
        const unsigned long long qs = sq[r];
        int k = (int) (qs & ((1ull << kSlotBits) - 1ull));
        const int ql = (int) (qs >> kSlotBits);
        const R end = fin ? set_v[k] + fw[ql] : set_v[k];               // from the state's own sum (the key folds -0 into +0)
        int rr = row_top;                                                 // (the ring: the row of frame base + t, stepped)
        for (int t = len - 1; t >= 0; --t) {
            if (k < 0 || k >= K) k = 0;                                   // (cannot happen: every kept state stored its source's slot)
            const size_t at = (size_t) (kWin ? rr : t) * K + k;
            int q = bq[at];
            if constexpr (!kShot) q = (unsigned) q < (unsigned) g.Q ? q : 0;      // (nor this: the column indexes the graph's arrays)
            rows[(size_t) t * nb + r] = q;
            k = bs[at];
            if constexpr (kWin) rr = ring_prev(rr, T);
        }
        scores[ob + r] = end;
        if constexpr (!kWin) {
            // (without emissions the walk reads neither P.inputs nor the transitions)
            const R *in = kShot ? (const R *) P.inputs + (int64_t) b * P.is1 : nullptr;
            const R *tr = (const R *) P.transition;
            int qp = rows[r], ip = kShot ? g.label[qp] : 0;
            R a = kShot ? in[(int64_t) ip * P.is2] : NINF;
            R gs = sw[qp];
            for (int t = 1; t < len; ++t) {
                const int q = rows[(size_t) t * nb + r];
                if constexpr (kShot) {
                    const int i = g.label[q];
                    a = (a + tr[(int64_t) i * P.ts0 + (int64_t) ip * P.ts1]) + in[(int64_t) t * P.is0 + (int64_t) i * P.is2];
                    ip = i;
                }
                if (q != qp) {
                    int lo = bg.orow[qp];
                    const int e1 = bg.orow[qp + 1];
                    int hi = e1;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (oarc[mid].x < q) lo = mid + 1; else hi = mid;
                    }
                    gs = gs + ((lo < e1 && oarc[lo].x == q) ? ow[lo] : NINF);
                }
                qp = q;
            }
            if (fin) gs = gs + fw[qp];
            if constexpr (kShot) escores[ob + r] = a;
            gscores[ob + r] = gs;
        }
    }
    __threadfence();
    __syncthreads();

    // ---- one wavefront per output row
    for (int r = wave; r < nbest; r += kNT / 64) {
        long long *tk = tokens + (ob + r) * T;
        long long *pb = path ? path + (ob + r) * T : nullptr, *st = states ? states + (ob + r) * T : nullptr;
        if (r >= nh) {
            for (int t = lane; t < T; t += 64) {
                tk[t] = -1;
                if (pb) pb[t] = -1;
                if (st) st[t] = -1;
            }
            if (lane == 0) {
                scores[ob + r] = NINF; tlen[ob + r] = 0;
                if constexpr (kShot) escores[ob + r] = NINF;
                if constexpr (!kWin) gscores[ob + r] = NINF;
            }
            continue;
        }
        int base = 0;
        long long carry = carry0;
        for (int c0 = 0; c0 < len; c0 += 64) {
            const int t = c0 + lane;
            long long cur = -1;
            if (t < len) {
                const int q = rows[(size_t) t * nb + r];
                cur = g.label[q];
                if (pb) pb[t] = cur;
                if (st) st[t] = g.state[q];
            }
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
        for (int t = len + lane; t < T; t += 64) {
            if (pb) pb[t] = -1;
            if (st) st[t] = -1;
        }
        if (lane == 0) tlen[ob + r] = base;
    }
}

// One launch of the kernel over B slots.
template <typename R, int SRC>
hipError_t launch_nbest_kernel(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const BeamNbestSrc &src, int B, int K,
                               int nbest, int final, void *scores, void *escores, void *gscores, long long *path,
                               long long *tokens, long long *tlen, long long *states, long long *num_hyps, long long *frames,
                               long long *committed, long long *status, hipStream_t stream) {
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    int P2 = 1;
    while (P2 < K) P2 *= 2;
    const size_t dyn = (size_t) P2 * (8 + sizeof(typename Key<R>::U));
    const void *fn = (const void *) beam_nbest_kernel<R, SRC>;
    if (dyn + 64 > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);
    hipLaunchKernelGGL((beam_nbest_kernel<R, SRC>), dim3(B), dim3(kNT), dyn, stream, P, G, BG, src, K, cap, nbest, P2, final,
                       (R *) scores, (R *) escores, (R *) gscores, path, tokens, tlen, states, num_hyps, frames, committed,
                       status);
    return hipGetLastError();
}

}  // namespace

BeamNbestLayout beam_nbest_layout(int elem, int T, int Q, int K, int cap, int nbest) {
    BeamNbestLayout l{};
    l.nb = nbest < K ? nbest : K;
    size_t off = beam_work_layout(elem, T, Q, K, cap).end;                // the beam search's own part, at the front
    l.fin = off;  off += a256(8 + (size_t) K * elem);
    l.rows = off; off += a256((size_t) T * l.nb * 4);
    l.per = off;
    return l;
}

size_t beam_nbest_work_bytes(int elem, int T, int B, int Q, int K, int cap, int nbest) {
    return (size_t) B * beam_nbest_layout(elem, T, Q, K, cap, nbest).per + tail_bytes(T, B);
}

template <typename R>
hipError_t launch_beam_nbest(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta, int nbest,
                             void *work, void *scores, void *emission_scores, void *graph_scores, long long *path,
                             long long *tokens, long long *tlen, long long *states, long long *num_hyps, hipStream_t stream) {
    const int T = P.T, B = P.B;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const BeamNbestLayout lay = beam_nbest_layout(sizeof(R), T, G.Q, K, cap, nbest);
    char *w = (char *) work, *tail = w + (size_t) B * lay.per;
    R *bsc = (R *) tail;
    long long *btl = (long long *) (tail + a256((size_t) B * 8));
    long long *bpa = (long long *) (tail + 2 * a256((size_t) B * 8));
    hipError_t e = launch_beam_graph<R>(P, G, BG, K, theta, work, bsc, bpa, bpa + (size_t) B * T, btl, bpa + 2 * (size_t) B * T,
                                        stream, lay.per, 0, lay.fin);
    if (e != hipSuccess) return e;
    return launch_beam_nbest_over<R>(P, G, BG, lay, K, nbest, work, scores, emission_scores, graph_scores, path, tokens, tlen, states,
                                     num_hyps, stream);
}

template <typename R>
hipError_t launch_beam_nbest_over(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const BeamNbestLayout &lay, int K,
                                  int nbest, void *work, void *scores, void *emission_scores, void *graph_scores, long long *path,
                                  long long *tokens, long long *tlen, long long *states, long long *num_hyps, hipStream_t stream) {
    char *w = (char *) work;
    BeamNbestSrc src{};
    src.base = w; src.per = lay.per; src.fin = lay.fin;
    src.cols = w + lay.rows; src.cols_per = lay.per; src.Tw = P.T; src.nb = lay.nb;
    return launch_nbest_kernel<R, kBeamNbestShot>(P, G, BG, src, P.B, K, nbest, 1, scores, emission_scores, graph_scores, path, tokens,
                                                  tlen, states, num_hyps, nullptr, nullptr, nullptr, stream);
}
template hipError_t launch_beam_nbest<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, double, int, void *,
                                             void *, void *, void *, long long *, long long *, long long *, long long *,
                                             long long *, hipStream_t);
template hipError_t launch_beam_nbest<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, double, int, void *,
                                              void *, void *, void *, long long *, long long *, long long *, long long *,
                                              long long *, hipStream_t);
#define ASG_BEAM_NBEST_OVER_INST(R)                                                                                            \
    template hipError_t launch_beam_nbest_over<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &,                     \
                                                  const BeamNbestLayout &, int, int, void *, void *, void *, void *, long long *, \
                                                  long long *, long long *, long long *, long long *, hipStream_t);
ASG_BEAM_NBEST_OVER_INST(float)
ASG_BEAM_NBEST_OVER_INST(double)
#undef ASG_BEAM_NBEST_OVER_INST

size_t beam_stream_nbest_work_bytes(int rows, int B, int K, int nbest) {
    return (size_t) B * a256((size_t) rows * (nbest < K ? nbest : K) * 4);
}

namespace {

// The source of a stream (rows = max_frames) or a window (rows = W) state: both have the slot of beam_stream_layout.
inline BeamNbestSrc stream_src(int elem, const GraphArgs &G, const BeamGraphArgs &BG, int K, int rows, const void *state, int nbest,
                               void *work, size_t stride = 0) {
    const BeamStreamLayout lay = beam_stream_layout(elem, rows, G.Q, K, beam_graph_cap(G.Q, K, BG.max_out, BG.num_start));
    BeamNbestSrc src{};
    src.base = (const char *) state; src.hdr = lay.hdr; src.set = lay.set;
    src.per = stride ? stride : lay.per;                                    // (a slot with parts of the caller's behind it)
    src.nb = nbest < K ? nbest : K;
    src.cols = (char *) work; src.cols_per = a256((size_t) rows * src.nb * 4); src.Tw = rows;
    return src;
}

}  // namespace

template <typename R>
hipError_t launch_beam_stream_nbest(const GraphArgs &G, const BeamGraphArgs &BG, int K, int max_frames, int B, const void *state,
                                    int final, int nbest, void *work, void *scores, void *graph_scores, long long *path,
                                    long long *tokens, long long *tlen, long long *states, long long *num_hyps, long long *frames,
                                    long long *status, hipStream_t stream, size_t stride) {
    Problem P{};                                                            // no emissions, no lengths: the state has both
    P.T = max_frames; P.B = B; P.N = 0;
    return launch_nbest_kernel<R, kBeamNbestStream>(P, G, BG, stream_src(sizeof(R), G, BG, K, max_frames, state, nbest, work, stride), B, K,
                                                    nbest, final != 0, scores, nullptr, graph_scores, path, tokens, tlen, states,
                                                    num_hyps, frames, nullptr, status, stream);
}
template <typename R>
hipError_t launch_beam_window_nbest(const GraphArgs &G, const BeamGraphArgs &BG, int K, int W, int B, const void *state, int final,
                                    int nbest, void *work, void *scores, long long *path, long long *tokens, long long *tlen,
                                    long long *states, long long *num_hyps, long long *frames, long long *committed,
                                    long long *status, hipStream_t stream, size_t stride) {
    Problem P{};
    P.T = W; P.B = B; P.N = 0;
    return launch_nbest_kernel<R, kBeamNbestWindow>(P, G, BG, stream_src(sizeof(R), G, BG, K, W, state, nbest, work, stride), B, K, nbest,
                                                    final != 0, scores, nullptr, nullptr, path, tokens, tlen, states, num_hyps,
                                                    frames, committed, status, stream);
}
#define ASG_BEAM_STREAM_NBEST_INST(R)                                                                                            \
    template hipError_t launch_beam_stream_nbest<R>(const GraphArgs &, const BeamGraphArgs &, int, int, int, const void *, int, int, \
                                                    void *, void *, void *, long long *, long long *, long long *, long long *,    \
                                                    long long *, long long *, long long *, hipStream_t, size_t);                   \
    template hipError_t launch_beam_window_nbest<R>(const GraphArgs &, const BeamGraphArgs &, int, int, int, const void *, int, int, \
                                                    void *, void *, long long *, long long *, long long *, long long *,            \
                                                    long long *, long long *, long long *, long long *, hipStream_t, size_t);
ASG_BEAM_STREAM_NBEST_INST(float)
ASG_BEAM_STREAM_NBEST_INST(double)
#undef ASG_BEAM_STREAM_NBEST_INST

}  // namespace asg
