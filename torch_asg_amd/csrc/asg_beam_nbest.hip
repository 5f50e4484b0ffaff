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
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"

namespace asg {

namespace {

constexpr int kNT = 1024;          // workgroup
constexpr int kSlotBits = 16;      // q << 16 | slot: K <= 2^16 slots, q < 2^31

// behind the utterances: what the beam search writes besides its sets (scores [B], lengths [B], path / tokens / states [3][B][T])
inline size_t tail_bytes(int T, int B) { return 2 * a256((size_t) B * 8) + a256((size_t) 3 * B * T * 8); }

template <typename U>
__device__ __forceinline__ bool pair_less(U ka, unsigned long long qa, U kb, unsigned long long qb) {
    return ka < kb || (ka == kb && qa < qb);
}

template <typename R>
__global__ void __launch_bounds__(kNT) beam_nbest_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, BeamNbestLayout lay, int K,
                                                         int cap, int nbest, int P2max, char *work, R *scores, R *escores, R *gscores,
                                                         long long *path, long long *tokens, long long *tlen,
                                                         long long *states, long long *nhyp) {
    using KT = Key<R>;
    using U = typename KT::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int ncand;
    unsigned long long *sq = (unsigned long long *) lds;                  // [P2max] q << 16 | slot
    U *sk = (U *) (sq + P2max);                                           // [P2max] ~key of end
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int N = P.N, T = P.T, nb = lay.nb;
    (void) N;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *tr = (const R *) P.transition;
    const R *sw = (const R *) g.start_w, *fw = (const R *) g.final_w, *ow = (const R *) bg.ow;
    const int2 *oarc = (const int2 *) bg.oarc;
    char *wb = work + (size_t) b * lay.per;
    const BeamWorkLayout wl = beam_work_layout(sizeof(R), T, g.Q, K, cap);
    const int *bq = (const int *) (wb + wl.bq), *bs = (const int *) (wb + wl.bs);            // [T][K] what beam_graph_kernel left
    const R *fin_v = (const R *) (wb + lay.fin + 8);
    int *rows = (int *) (wb + lay.rows);                                                     // [T][nb]
    const int64_t ob = (int64_t) b * nbest;                                                  // the utterance's first output row

    int na = len >= 1 ? *(const int *) (wb + lay.fin) : 0;
    na = na < 0 ? 0 : (na > K ? K : na);
    int P2 = 1;
    while (P2 < na) P2 *= 2;                                              // (<= P2max: na <= K)
    if (tid == 0) ncand = 0;
    __syncthreads();
    // ---- the candidates of the last set
    const int *bql = bq + (size_t) (len >= 1 ? len - 1 : 0) * K;
    for (int x0 = 0; x0 < P2; x0 += kNT) {
        const int x = x0 + tid;
        U ik = ~(U) 0;
        unsigned long long qs = ~0ull;
        bool cand = false;
        if (x < na) {
            const int q = bql[x];
            const R end = fin_v[x] + fw[q];
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
        const R end = fin_v[k] + fw[ql];                                  // from the state's own sum (the key folds -0 into +0)
        for (int t = len - 1; t >= 0; --t) {
            if (k < 0 || k >= K) k = 0;                                   // (cannot happen: every kept state stored its source's slot)
            rows[(size_t) t * nb + r] = bq[(size_t) t * K + k];
            k = bs[(size_t) t * K + k];
        }
        int qp = rows[r], ip = g.label[qp];
        R a = in[(int64_t) ip * P.is2];
        R gs = sw[qp];
        for (int t = 1; t < len; ++t) {
            const int q = rows[(size_t) t * nb + r], i = g.label[q];
            a = (a + tr[(int64_t) i * P.ts0 + (int64_t) ip * P.ts1]) + in[(int64_t) t * P.is0 + (int64_t) i * P.is2];
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
            qp = q; ip = i;
        }
        gs = gs + fw[qp];
        scores[ob + r] = end;
        escores[ob + r] = a;
        gscores[ob + r] = gs;
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
            if (lane == 0) { scores[ob + r] = NINF; escores[ob + r] = NINF; gscores[ob + r] = NINF; tlen[ob + r] = 0; }
            continue;
        }
        int base = 0;
        long long carry = -1;
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
    const int B = P.B;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    char *w = (char *) work;
    int P2 = 1;
    while (P2 < K) P2 *= 2;
    const size_t dyn = (size_t) P2 * (8 + sizeof(typename Key<R>::U));
    const void *fn = (const void *) beam_nbest_kernel<R>;
    if (dyn + 64 > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);
    hipLaunchKernelGGL((beam_nbest_kernel<R>), dim3(B), dim3(kNT), dyn, stream, P, G, BG, lay, K, cap, nbest, P2, w,
                       (R *) scores,
                       (R *) emission_scores, (R *) graph_scores, path, tokens, tlen, states, num_hyps);
    return hipGetLastError();
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

}  // namespace asg
