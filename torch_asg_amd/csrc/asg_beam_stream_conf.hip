// torch_asg_amd/csrc/asg_beam_stream_conf.hip -- the LATTICE-KEEPING beam stream on gfx950: the streaming search of
// asg_beam_stream.hip with a state that also keeps what the token confidences of asg_beam_conf.hip are computed from, so that a
// stream can say how sure it is of a token while the utterance is still arriving.  The specification is
// include/asg_hip.h::asg_beam_conf_stream_confidence; tests/beam_stream_conf_ref.py restates it in numpy.  DESIGN.md 5ad, 5af.
//
// One slot of the state (beam_conf_stream_layout; every part 256-byte aligned): the plain stream's slot unchanged at the front --
// the search's workspace for T = max_frames, the header, the stored set --; behind it cnt int32 [max_frames] (|A_t|), the emissions
// [max_frames][N], nu int32 [max_frames], U int32 [max_frames][K] (A_t ascending), A [max_frames][K] (alpha) and two rows of beta.
// The header's word 3 is apos: the frames whose U / nu / A rows are valid.
// The search is NOT here.  Reset, advance, result and n-best are the plain stream's kernels, launched by the plain stream's
// launchers with this layout's stride: the advance is beam_stream_advance_kernel with the KeepLattice policy
// (asg_beam_stream_lat.h), which besides the plain kernel's work writes cnt[gt] of every frame of the chunk -- 0 for the frames an
// empty beam skips -- and copies the chunk's emissions into rows pos .. pos+n-1.  This unit holds the layout and the two kernels of
// a confidence call:
//   beam_stream_conf_catchup         one 1024-thread workgroup per slot, frames [apos, pos) read from the header: U_t = A_t sorted
//                                    (stream_lat_sets), then the frame body of asg_beam_alpha.inc (the text beam_loss_fwd
//                                    compiles) resumed from the stored rows U[apos-1] / A[apos-1], loaded into LDS with
//                                    device-scope loads, or from the start weights at frame 0; then apos = pos.
//                                    LAZY: it runs in front of a confidence call, every frame's alpha is computed once however
//                                    often confidences are asked for, and what it writes depends on nothing but the frames.
//   beam_stream_conf_bwd             one workgroup per slot: the hypothesis by beam_stream_hyp (the function
//                                    beam_stream_result_kernel is), Z by lattice_z over the last set, and the tail of
//                                    beam_conf_bwd by beam_conf_tokens (asg_beam_conf_pull.h) over the stored emissions.
//                                    The one new thing is the end term of a PREFIX (0 instead of the final weight), which the
//                                    pull takes as its lattice type (PrefixLat).
// A confidence call is two launches (catch-up, bwd): no host synchronisation, no memset, no copy.  No float atomics: integer
// accumulators with 54 fractional bits in the ring, the same adds in the same order as asg_beam_graph_confidence.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_frame.h"
#include "asg_beam_lattice.h"
#include "asg_beam_stream_lat.h"
#include "asg_beam_token_lat.h"
#include "asg_beam_conf_sink.h"
#include "asg_beam_conf_pull.h"

namespace asg {

namespace {

// Dynamic LDS: [reduction slots][pa R K][pq int K] (beam_loss_fwd's), the sort's int [P2(K)] over the same bytes.
template <typename R>
__global__ void __launch_bounds__(kBL) beam_stream_conf_catchup(Problem P, GraphArgs g, int K, int max_frames, char *state,
                                                                BeamConfStreamLayout lay) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    R *pa = (R *) (lds + kBLHead);                       // [K] alpha[t-1] of U_{t-1}
    int *pq = (int *) (pa + K);                          // [K] U_{t-1}
    int *v = (int *) (lds + kBLHead);                    // the sort's slots, before pa / pq are used
    const int tid = threadIdx.x, b = blockIdx.x, N = P.N;
    char *wb = state + (size_t) b * lay.per;
    int *hdr = (int *) (wb + lay.st.hdr);
    const int L = stream_pos(hdr, max_frames);
    int a0 = stream_apos(hdr, L);
    if (a0 >= L) return;                                 // caught up (apos <= pos always: nothing to store)
    const int *bq = (const int *) wb;                    // the search's [max_frames][K] kept states
    int *nu = (int *) (wb + lay.lat.nu);
    int *U = (int *) (wb + lay.lat.U);
    R *A = (R *) (wb + lay.lat.A);
    const R *em = (const R *) (wb + lay.em);
    const R *trm = (const R *) P.transition;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };

    stream_lat_sets<int>(a0, L, K, (const int *) (wb + lay.lat.cnt), v, 0x7FFFFFFF, U, nu,
                         [&](int t, int x) -> int { return bq[(int64_t) t * K + x]; });

    // ---- alpha, resumed: beam_loss_fwd's frame 0, or rows a0 - 1 back into LDS; then the frame body it compiles
    const R NINF = Num<R>::ninf();
    const R *sw = (const R *) g.start_w, *ew = (const R *) g.edge_w;
    int mp;
    if (a0 == 0) {
        mp = nu[0];
        for (int x = tid; x < mp; x += kBL) {
            const int q = U[x];
            const R a = sw[q] + em[g.label[q]];
            pq[x] = q;
            pa[x] = a;
            A[x] = a;
        }
        a0 = 1;
    } else {
        mp = nu[a0 - 1];
        const int *Up = U + (int64_t) (a0 - 1) * K;
        const R *Ap = A + (int64_t) (a0 - 1) * K;
        for (int x = tid; x < mp; x += kBL) { pq[x] = dev_load(Up + x); pa[x] = dev_load(Ap + x); }
    }
    __syncthreads();
    for (int t = a0; t < L; ++t) {
        const int mt = nu[t];
        const int *Ut = U + (int64_t) t * K;
        R *Arow = A + (int64_t) t * K;
        const R *xt = em + (int64_t) t * N;                // (P.is2 is 1: the stored rows are dense)
#include "asg_beam_alpha.inc"
    }
    if (tid == 0) hdr[kHdrApos] = L;
}

inline size_t stream_conf_lds(int elem, int K) { return bwd_front(elem, 4, K) + (size_t) kConfRing * 8; }

// Dynamic LDS: [nb R K][nq int K][pad to 16][ring u64 256] (beam_conf_bwd's).
template <typename R>
__global__ void __launch_bounds__(kBL) beam_stream_conf_bwd(Problem P, typename PrefixLat<R>::Args args, int K, int cap, int max_frames,
                                                            char *state, BeamConfStreamLayout lay, int tol, R *scores,
                                                            long long *path, long long *tokens, long long *tlen, long long *states,
                                                            long long *tframes, R *conf, R *Zs, long long *frames,
                                                            long long *status) {
    using U = typename Key<R>::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ Ctl<U> ctl;
    __shared__ R red[kBL / 64];
    R *nb = (R *) lds;                                                         // [K] beta[t] of U_t
    int *nq = (int *) (lds + (size_t) K * sizeof(R));                          // [K] U_t
    unsigned long long *ring = (unsigned long long *) (lds + bwd_front(sizeof(R), 4, K));
    const int tid = threadIdx.x, b = blockIdx.x, T = max_frames;
    char *wb = state + (size_t) b * lay.per;
    const R *fw = args.fin ? (const R *) args.g.final_w : nullptr;

    int len;
    const U bkey = beam_stream_hyp<R>(ctl, args.g, K, cap, T, wb, lay.st, args.fin, scores, path, tokens, tlen, states, frames,
                                      status, len);
    __threadfence();
    __syncthreads();                                        // path, tokens and the token count, for every wavefront

    // ---- Z over the last set
    const int *Ul = (const int *) (wb + lay.lat.U) + (int64_t) (len >= 1 ? len - 1 : 0) * K;
    const R *Al = (const R *) (wb + lay.lat.A) + (int64_t) (len >= 1 ? len - 1 : 0) * K;
    int ml = len >= 1 ? ((const int *) (wb + lay.lat.nu))[len - 1] : 0;
    ml = ml < 0 ? 0 : (ml > K ? K : ml);
    const R Z = lattice_z<R>(ml, red, [&](int x) -> R { return fw ? Al[x] + fw[Ul[x]] : Al[x]; });
    if (tid == 0) Zs[b] = Z;

    int n = 0;
    if (len >= 1) {
        const long long l = bkey == 0 ? 0 : dev_load(tlen + b);
        n = (int) (l < 0 ? 0 : (l > len ? len : l));                           // (a path of len frames starts at most len tokens)
    }
    beam_conf_tokens<R, PrefixLat<R>>(P, args, wb, lay.beta, Z, len, n, T, tol, path + (int64_t) b * T, tokens + (int64_t) b * T,
                                      tframes + (int64_t) b * T, conf + (int64_t) b * T, ring, nq, nb);
}

}  // namespace

BeamConfStreamLayout beam_conf_stream_layout(int elem, int max_frames, int Q, int K, int cap, int N) {
    BeamConfStreamLayout l{};
    l.st = beam_stream_layout(elem, max_frames, Q, K, cap);               // the plain stream's slot, at the front
    const size_t T = (size_t) max_frames;
    size_t off = l.st.per;
    l.lat.M = K; l.lat.nf = 0;
    l.lat.hdr = l.st.hdr;
    l.lat.cnt = off; off += a256(T * 4);
    l.em = off;      off += a256(T * N * elem);
    l.lat.nu = off;  off += a256(T * 4);
    l.lat.U = off;   off += a256(T * K * 4);
    l.lat.A = off;   off += a256(T * K * elem);
    l.lat.key = l.lat.qk = off;                                            // (no targets: nothing is forced)
    l.beta = off;    off += a256(2 * (size_t) K * elem);
    l.per = l.st.per = l.lat.per = off;
    return l;
}

size_t beam_conf_stream_state_bytes(int elem, int max_frames, int B, int Q, int K, int cap, int N) {
    return (size_t) B * beam_conf_stream_layout(elem, max_frames, Q, K, cap, N).per;
}

template <typename R>
hipError_t launch_beam_conf_stream_confidence(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, int max_frames,
                                              void *state, int final, int tol, void *scores, long long *path, long long *tokens,
                                              long long *tlen, long long *states, long long *token_frames, void *token_conf,
                                              void *normalisers, long long *frames, long long *status, hipStream_t stream) {
    const int N = P.N;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const BeamConfStreamLayout lay = beam_conf_stream_layout(sizeof(R), max_frames, G.Q, K, cap, N);
    int P2 = 2;
    while (P2 < K) P2 *= 2;
    Problem PC = P;                                                         // the catch-up reads the stored emissions: label stride 1
    PC.is2 = 1;
    size_t dyn = (size_t) K * (sizeof(R) + 4);
    if (dyn < (size_t) P2 * 4) dyn = (size_t) P2 * 4;
    dyn += kBLHead;
    set_lds((const void *) beam_stream_conf_catchup<R>, dyn);
    hipLaunchKernelGGL((beam_stream_conf_catchup<R>), dim3(P.B), dim3(kBL), dyn, stream, PC, G, K, max_frames, (char *) state, lay);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the pull reads the stored emissions as its inputs: frame t of slot b at em + b * per + t * N
    Problem PS = P;
    PS.inputs = (const char *) state + lay.em;
    PS.is0 = N; PS.is1 = (int64_t) (lay.per / sizeof(R)); PS.is2 = 1;
    PS.T = max_frames; PS.in_len = nullptr; PS.targets = nullptr; PS.tg_len = nullptr;
    typename PrefixLat<R>::Args args{};
    args.g = G; args.bg = BG; args.lay = lay.lat; args.fin = final != 0;
    const size_t dyn2 = stream_conf_lds(sizeof(R), K);
    set_lds((const void *) beam_stream_conf_bwd<R>, dyn2, sizeof(Ctl<typename Key<R>::U>) + sizeof(R) * (kBL / 64));
    hipLaunchKernelGGL((beam_stream_conf_bwd<R>), dim3(P.B), dim3(kBL), dyn2, stream, PS, args, K, cap, max_frames, (char *) state, lay,
                       tol, (R *) scores, path, tokens, tlen, states, token_frames, (R *) token_conf, (R *) normalisers, frames,
                       status);
    return hipGetLastError();
}

#define ASG_BEAM_CONF_STREAM_INST(R)                                                                                              \
    template hipError_t launch_beam_conf_stream_confidence<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, int,   \
                                                              void *, int, int, void *, long long *, long long *, long long *,     \
                                                              long long *, long long *, void *, void *, long long *, long long *,  \
                                                              hipStream_t);
ASG_BEAM_CONF_STREAM_INST(float)
ASG_BEAM_CONF_STREAM_INST(double)
#undef ASG_BEAM_CONF_STREAM_INST

}  // namespace asg
