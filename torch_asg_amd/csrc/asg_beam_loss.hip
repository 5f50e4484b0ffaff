// torch_asg_amd/csrc/asg_beam_loss.hip -- the BEAM-PRUNED normaliser of an ASG criterion composed with a token automaton, on
// gfx950: the log-semiring pass of asg_graph_loss.hip restricted, frame by frame, to the product states the beam search of
// asg_beam_graph.hip keeps (plus the states every alignment of the target runs through), and its gradients.  The specification
// is include/asg_hip.h::asg_beam_graph_full_forward; tests/beam_loss_ref.py restates it in numpy.
//
// Forward, four launches on one stream:
//   1  beam_graph_kernel as the decoder runs it (the same device code, so the same active sets A_t bit for bit), asked to
//      leave |A_t| of every frame beside its [T][K] list of kept product states;
//   2  beam_loss_targets: one workgroup per utterance walks the automaton along the merged target (one thread, n dependent
//      loads), then finds every product state q_k = (y_k, s_k) by binary search over the (state, label) order of the states;
//   3  beam_loss_sets<TokenSets>: one workgroup per (utterance, frame) -- utterances in x, frames strided over y -- sorts A_t with
//      the forced states F_t of the frame in LDS (bitonic over the power of two its own count needs), blanks the duplicates
//      and sorts again: U[t][0 .. nu[t]) ascending;
//   4  beam_loss_fwd: one 1024-thread workgroup per utterance walks the frames with U_{t-1} and its alphas in LDS.  G lanes per
//      target q pull through q's incoming CSR row and find each source in U_{t-1} by binary search in LDS; when the row is
//      longer than |U_{t-1}| (the root of a lexicon trie) they walk U_{t-1} instead and binary-search each kept source in the
//      row.  Max pass, then sum pass; partial results of the G lanes meet in a fixed butterfly.  The alpha of a frame goes to
//      the workspace ([T][M] when a gradient is wanted, else two rows) and comes back into LDS with device-scope loads.  The body
//      of a frame is asg_beam_alpha.inc, which the catch-up of the lattice-keeping stream (asg_beam_stream_conf.hip) includes too.
// Backward, two launches: beam_loss_bwd<R, TL, TokenLat<R>> (the mirror image through the outgoing CSR against U_{t+1} in LDS; it
// owns beta, the label posteriors and the posteriors of every stay and edge) and beam_loss_tr_reduce.
// Launches 3 and the backward, the end of 4 (Z_K) and every small helper are written once for this unit and
// asg_beam_word_loss.hip, in asg_beam_lattice.h; this unit keeps what is its own: the target kernels, the alpha kernel (a PULL
// through incoming rows), and TokenSets / TokenLat, which tell the shared text what a key is and where its edges lie.
// NO FLOAT ATOMICS: posteriors are summed as 64-bit fixed-point integers (integer adds are associative, so the order the
// lanes arrive in cannot change a bit): a frame's label posteriors in LDS with 62 fractional bits (their sum is 1), the
// expected (i, j) counts of an utterance in a [N][N] tile -- in LDS while it fits, else in the utterance's scratch -- with
// 62 - ceil(log2(len)) fractional bits (a cell holds at most len - 1).  The tiles become grad_transition in a last launch that
// adds the utterances in ascending order.  Work and memory per frame follow |U_t| and the edges of the kept states, never Q
// or E (the Q-sized slot arrays are the beam search's own).  Every output, padding row and scratch word that is read is
// written by these kernels: no memset, so both directions can be captured and replayed.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"     // a256, beam_work_layout: the beam search's own part lies at the front of the workspace
#include "asg_beam_lattice.h"    // everything behind the search that the word family's loss shares
#include "asg_beam_token_lat.h"  // TokenLat: how a product state's edges are walked (shared with asg_beam_conf.hip)

namespace asg {

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// 2: the forced product states q_1 .. q_n of every utterance; hdr[0] = n (0: nothing is forced).
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBS) beam_loss_targets(Problem P, GraphArgs g, BeamLossArgs L, BeamLossLayout lay, char *work) {
    __shared__ int sn, bad;
    const int b = blockIdx.x, tid = threadIdx.x, N = P.N, S = P.S;
    char *wb = work + (size_t) b * lay.per;
    int *hdr = (int *) (wb + lay.hdr), *qk = (int *) (wb + lay.qk);
    long long *key = (long long *) (wb + lay.key);
    const int len = clamp_len(P.in_len, b, P.T);
    if (tid == 0) {
        int n = 0;
        if (P.targets && lay.nf > 0) {
            const int64_t l = P.tg_len ? P.tg_len[b] : S;
            const int tl = (int) (l < 0 ? 0 : (l > S ? S : l));
            if (tl >= 1 && tl <= len) {                   // (otherwise the target has no alignment)
                int st = L.start;
                long long prev = -1;
                for (int k = 0; k < tl; ++k) {
                    const long long y = P.targets[(int64_t) b * P.gs0 + (int64_t) k * P.gs1];
                    if (y == prev) continue;
                    const int nx = (y < 0 || y >= N) ? -1 : L.next[(int64_t) st * N + y];
                    if (nx < 0) { n = 0; break; }
                    key[n++] = (long long) nx * N + y;
                    st = nx;
                    prev = y;
                }
            }
        }
        sn = n;
        bad = 0;
    }
    __threadfence();
    __syncthreads();
    const int n = sn, Q = g.Q;
    for (int k = tid; k < n; k += kBS) {
        const long long want = dev_load(key + k);
        int lo = 0, hi = Q;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((long long) g.state[mid] * N + g.label[mid] < want) lo = mid + 1; else hi = mid;
        }
        if (lo >= Q || (long long) g.state[lo] * N + g.label[lo] != want) { atomicOr(&bad, 1); lo = 0; }
        qk[k] = lo;
    }
    __syncthreads();
    if (tid == 0) hdr[0] = bad ? 0 : n;
}

// the automaton must also ACCEPT the target: final_w of the last forced state
template <typename R>
__global__ void __launch_bounds__(64) beam_loss_accept(GraphArgs g, BeamLossLayout lay, char *work, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    char *wb = work + (size_t) b * lay.per;
    int *hdr = (int *) (wb + lay.hdr);
    const int *qk = (const int *) (wb + lay.qk);
    const int n = hdr[0];
    if (n > 0 && !(((const R *) g.final_w)[qk[n - 1]] > Num<R>::ninf())) hdr[0] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// 3: beam_loss_sets<TokenSets> (asg_beam_lattice.h).  A key is a product state: 4 bytes in LDS, in U and in the workspace.
// ---------------------------------------------------------------------------------------------------------------------
struct TokenSets {
    using Key = int;
    static constexpr Key kFlag = (int) 0x80000000;                          // a state is below 2^31: the sign bit flags a duplicate
    BeamLossLayout lay;
    int K;
    __device__ Key kept(const char *wb, int t, int x) const { return ((const int *) wb)[(int64_t) t * K + x]; }   // the search's [T][K]
    __device__ const Key *forced(const char *wb) const { return (const int *) (wb + lay.qk); }
};

// ---------------------------------------------------------------------------------------------------------------------
// 4: alpha over the U_t, and Z_K.  Dynamic LDS: [reduction slots][pq int M][pa R M].
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kBL) beam_loss_fwd(Problem P, GraphArgs g, BeamLossLayout lay, int store, char *work, R *scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    R *red = (R *) lds;
    const int M = lay.M;
    R *pa = (R *) (lds + kBLHead);                       // [M] alpha[t-1] of U_{t-1}
    int *pq = (int *) (pa + M);                          // [M] U_{t-1}
    const int tid = threadIdx.x, b = blockIdx.x, T = P.T;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    if (len < 1) { if (tid == 0) scores[b] = NINF; return; }
    char *wb = work + (size_t) b * lay.per;
    const int *U = (const int *) (wb + lay.U), *nu = (const int *) (wb + lay.nu);
    R *A = (R *) (wb + lay.A);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *trm = (const R *) P.transition;
    const R *sw = (const R *) g.start_w, *fw = (const R *) g.final_w, *ew = (const R *) g.edge_w;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };

    int mp = nu[0];
    for (int x = tid; x < mp; x += kBL) {
        const int q = U[x];
        const R a = sw[q] + in[(int64_t) g.label[q] * P.is2];
        pq[x] = q;
        pa[x] = a;
        if (store) A[x] = a;
    }
    __syncthreads();
    for (int t = 1; t < len; ++t) {
        const int mt = nu[t];
        const int *Ut = U + (int64_t) t * M;
        R *Arow = A + (int64_t) (store ? t : (t & 1)) * M;
        const R *xt = in + (int64_t) t * P.is0;
#include "asg_beam_alpha.inc"       // the frame body (shared with asg_beam_stream_conf.hip)
    }
    const R Z = lattice_z<R>(mp, red, [&](int x) -> R { return pa[x] + fw[pq[x]]; });
    if (tid == 0) scores[b] = Z;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward: beam_loss_bwd<R, TL, TokenLat<R>> (asg_beam_lattice.h), the mirror image of 4 through the outgoing CSR.
// ---------------------------------------------------------------------------------------------------------------------
// TokenLat<R> (asg_beam_token_lat.h): the edges are bg's outgoing CSR; the token confidences (asg_beam_conf.hip) walk them too.

}  // namespace

BeamLossLayout beam_loss_layout(int elem, int T, int Q, int K, int cap, int nf, bool store) {
    BeamLossLayout l{};
    l.nf = nf;
    l.M = K + nf;
    size_t off = beam_work_layout(elem, T, Q, K, cap).end;                 // the beam search's own part, at the front
    l.cnt = off; off += a256((size_t) T * 4);
    l.nu = off;  off += a256((size_t) T * 4);
    l.hdr = off; off += 256;
    l.key = off; off += a256((size_t) nf * 8);
    l.qk = off;  off += a256((size_t) nf * 4);
    l.U = off;   off += a256((size_t) T * l.M * 4);
    l.A = off;   off += a256((size_t) (store ? T : 2) * l.M * elem);
    l.per = off;
    return l;
}

// behind the utterances: what the beam search writes besides its sets (scores [B], path / tokens / states [3][B][T], lengths [B])
size_t beam_loss_tail_bytes(int T, int B) { return 2 * a256((size_t) B * 8) + a256((size_t) 3 * B * T * 8); }

size_t beam_loss_work_bytes(int elem, int T, int B, int Q, int K, int cap, int nf, bool store) {
    return (size_t) B * beam_loss_layout(elem, T, Q, K, cap, nf, store).per + beam_loss_tail_bytes(T, B);
}

size_t beam_loss_scratch_per(int elem, int M, int N) { return a256(2 * (size_t) M * elem) + a256((size_t) N * N * 8); }

bool beam_loss_fits(int elem, int M, int N) {
    return kBLHead + (size_t) M * (elem + 4) <= kBLLds && bwd_lds(elem, 4, M, N, false) <= kBLLds;
}

// The forward's launches behind a layout the caller made: `lay.per` may be wider than beam_loss_layout's (a caller with parts of
// its own behind the layout -- asg_beam_conf.hip), and the five outputs of the search go where the caller says.  fin_off != 0: the
// search also leaves its last set there (launch_beam_graph's fin_off), for an n-best stage behind it (asg_beam_nbest_conf.hip).
template <typename R>
hipError_t launch_beam_loss_lattice(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const BeamLossArgs &L,
                                    const BeamLossLayout &lay, int K, double theta, bool store, void *work, void *scores,
                                    void *beam_scores, long long *path, long long *tokens, long long *tlen, long long *states,
                                    size_t fin_off, hipStream_t stream) {
    const int B = P.B;
    char *w = (char *) work;
    hipError_t e = launch_beam_graph<R>(P, G, BG, K, theta, work, beam_scores, path, tokens, tlen, states, stream, lay.per, lay.cnt, fin_off);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beam_loss_targets, dim3(B), dim3(kBS), 0, stream, P, G, L, lay, w);
    hipLaunchKernelGGL((beam_loss_accept<R>), dim3((B + 63) / 64), dim3(64), 0, stream, G, lay, w, B);
    e = launch_beam_loss_sets(P, TokenSets{lay, K}, w, stream);
    if (e != hipSuccess) return e;
    const size_t dyn = kBLHead + (size_t) lay.M * (sizeof(R) + 4);
    set_lds((const void *) beam_loss_fwd<R>, dyn);
    hipLaunchKernelGGL((beam_loss_fwd<R>), dim3(B), dim3(kBL), dyn, stream, P, G, lay, (int) store, w, (R *) scores);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_loss_forward(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const BeamLossArgs &L, int K,
                                    double theta, bool store, void *work, void *scores, hipStream_t stream) {
    const int T = P.T, B = P.B;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const int nf = P.targets ? (P.S < T ? P.S : T) : 0;
    const BeamLossLayout lay = beam_loss_layout(sizeof(R), T, G.Q, K, cap, nf, store);
    char *tail = (char *) work + (size_t) B * lay.per;
    long long *btl = (long long *) (tail + a256((size_t) B * 8));
    long long *bpa = (long long *) (tail + 2 * a256((size_t) B * 8));
    return launch_beam_loss_lattice<R>(P, G, BG, L, lay, K, theta, store, work, scores, tail, bpa, bpa + (size_t) B * T, btl,
                                       bpa + 2 * (size_t) B * T, 0, stream);
}

template <typename R>
hipError_t launch_beam_loss_backward(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, const void *work,
                                     const void *scores, const void *grad_scores, void *grad_inputs, void *grad_transition,
                                     void *scratch, bool accumulate, hipStream_t stream) {
    const int T = P.T;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const int nf = P.targets ? (P.S < T ? P.S : T) : 0;
    return launch_lattice_backward<R, TokenLat<R>>(P, {G, BG, beam_loss_layout(sizeof(R), T, G.Q, K, cap, nf, true)}, work, scores,
                                                   grad_scores, grad_inputs, grad_transition, scratch, accumulate, stream);
}

template hipError_t launch_beam_loss_forward<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const BeamLossArgs &,
                                                    int, double, bool, void *, void *, hipStream_t);
template hipError_t launch_beam_loss_forward<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const BeamLossArgs &,
                                                     int, double, bool, void *, void *, hipStream_t);
#define ASG_BEAM_LOSS_LATTICE_INST(R)                                                                                        \
    template hipError_t launch_beam_loss_lattice<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &,                 \
                                                    const BeamLossArgs &, const BeamLossLayout &, int, double, bool, void *,    \
                                                    void *, void *, long long *, long long *, long long *, long long *,        \
                                                    size_t, hipStream_t);
ASG_BEAM_LOSS_LATTICE_INST(float)
ASG_BEAM_LOSS_LATTICE_INST(double)
#undef ASG_BEAM_LOSS_LATTICE_INST
template hipError_t launch_beam_loss_backward<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, const void *,
                                                     const void *, const void *, void *, void *, void *, bool, hipStream_t);
template hipError_t launch_beam_loss_backward<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, const void *,
                                                      const void *, const void *, void *, void *, void *, bool, hipStream_t);

}  // namespace asg
