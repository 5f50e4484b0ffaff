// torch_asg_amd/csrc/asg_beam_stream_conf.hip -- the LATTICE-KEEPING beam stream on gfx950: the streaming search of
// asg_beam_stream.hip with a state that also keeps what the token confidences of asg_beam_conf.hip are computed from, so that a
// stream can say how sure it is of a token while the utterance is still arriving.  The specification is
// include/asg_hip.h::asg_beam_conf_stream_confidence; tests/beam_stream_conf_ref.py restates it in numpy.  DESIGN.md 5ad.
//
// One slot of the state (beam_conf_stream_layout; every part 256-byte aligned): the plain stream's slot unchanged at the front --
// the search's workspace for T = max_frames, the header, the stored set -- so that beam_stream_result_kernel and beam_nbest_kernel
// run on it as they are (their launchers take the slot stride); behind it cnt int32 [max_frames] (|A_t|), the emissions
// [max_frames][N], nu int32 [max_frames], U int32 [max_frames][K] (A_t ascending), A [max_frames][K] (alpha) and two rows of beta.
// The header's word 3 is apos: the frames whose U / nu / A rows are valid.
//   beam_stream_conf_reset_kernel    the plain reset, and apos = 0.
//   beam_stream_conf_advance_kernel  beam_stream_advance_kernel's frame loop (beam_frame: the same sets and values), which also
//                                    writes cnt[gt] of every frame of the chunk -- 0 for the frames an empty beam skips -- and
//                                    copies the chunk's emissions into rows pos .. pos+n-1 (coalesced, the whole workgroup).
//   beam_stream_conf_catchup         one 1024-thread workgroup per slot, frames [apos, pos) read from the header: U_t = A_t sorted
//                                    (bitonic in LDS; the kept states of a frame are distinct, so the ascending list is what
//                                    beam_loss_sets<TokenSets> leaves without targets), then the frame body of asg_beam_alpha.inc
//                                    (the text beam_loss_fwd compiles) resumed from the stored rows U[apos-1] / A[apos-1], loaded
//                                    into LDS with device-scope loads, or from the start weights at frame 0; then apos = pos.
//                                    LAZY: it runs in front of a confidence call, every frame's alpha is computed once however
//                                    often confidences are asked for, and what it writes depends on nothing but the frames.
//   beam_stream_conf_bwd             one workgroup per slot: the winner, backtrace and collapse of beam_stream_result_kernel (with
//                                    or without the final weights), token_frames by beam_conf_bwd's ballot / popcount walk, Z by
//                                    lattice_z over the last set, and beam_conf_pull<R, HypSink<R>> over the stored emissions.
//                                    The one new thing is the end term of a PREFIX (0 instead of the final weight), which the
//                                    pull takes as its lattice type (PrefixLat), so asg_beam_conf.hip's text is unchanged.
// A confidence call is two launches (catch-up, bwd): no host synchronisation, no memset, no copy.  No float atomics: integer
// accumulators with 54 fractional bits in the ring, the same adds in the same order as asg_beam_graph_confidence.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_frame.h"
#include "asg_beam_lattice.h"
#include "asg_beam_token_lat.h"
#include "asg_beam_conf_sink.h"
#include "asg_beam_conf_pull.h"

namespace asg {

namespace {

constexpr int kHdrApos = 3;                     // header: int32 pos, |A|, overflow, apos

__global__ void __launch_bounds__(256) beam_stream_conf_reset_kernel(char *state, BeamConfStreamLayout lay, BeamWorkLayout wl, int Q,
                                                                      int key_bytes, const unsigned char *mask) {
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;
    char *wb = state + (size_t) b * lay.per;
    beam_reset_tables(wb, wl, Q, key_bytes);
    if (blockIdx.y == 0 && threadIdx.x < 4) ((int *) (wb + lay.st.hdr))[threadIdx.x] = 0;   // pos, |A|, overflow, apos
}

template <typename R, bool TRL>
__global__ void __launch_bounds__(kBT) beam_stream_conf_advance_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, int K, R theta, int cap,
                                                                       int max_frames, char *state, BeamConfStreamLayout lay) {
    using KT = Key<R>;
    using U = typename KT::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Ctl<U> &ctl = *(Ctl<U> *) lds;
    R *cur_v = (R *) (lds + kFixedLds);                    // [K]
    int *cur_q = (int *) (cur_v + K);                      // [K]
    R *trs = (R *) (cur_q + K + (K & 1));                  // [N][N] if TRL
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = P.N;
    char *wb = state + (size_t) b * lay.per;
    int *hdr = (int *) (wb + lay.st.hdr);
    R *set_v = (R *) (wb + lay.st.set);                     // values [K], then product states [K]
    int *cnt = (int *) (wb + lay.lat.cnt);                  // [max_frames]
    R *em = (R *) (wb + lay.em);                            // [max_frames][N]
    int pos = hdr[0];
    pos = pos < 0 ? 0 : (pos > max_frames ? max_frames : pos);
    const int want = clamp_len(P.in_len, b, P.T);
    const int n = want < max_frames - pos ? want : max_frames - pos;
    if (n < want && tid == 0) hdr[2] = 1;                   // frames beyond max_frames are not consumed
    if (n < 1) return;
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    // the chunk's emissions into rows pos .. pos+n-1 (nothing reads them before the next launch)
    for (int64_t x = tid; x < (int64_t) n * N; x += kBT) {
        const int64_t t = x / N, i = x % N;
        em[(int64_t) pos * N + x] = in[t * P.is0 + i * P.is2];
    }
    const R *tr = (const R *) P.transition;
    BeamFrame<R> f;
    f.ctl = &ctl; f.cur_v = cur_v; f.cur_q = cur_q; f.trs = trs; f.tr = tr; f.ts0 = P.ts0; f.ts1 = P.ts1;
    f.N = N; f.Q = g.Q; f.K = K; f.G = beam_lanes_per_state(K); f.theta = theta;
    f.label = g.label; f.orow = bg.orow; f.start_q = bg.start_q; f.num_start = bg.num_start;
    f.oarc = (const int2 *) bg.oarc; f.ow = (const R *) bg.ow; f.sw = (const R *) g.start_w;
    int *bq, *bs;
    f.bind_work(wb, max_frames, cap, bq, bs);

    int na0 = pos >= 1 ? hdr[1] : 0;
    na0 = na0 < 0 ? 0 : (na0 > K ? K : na0);
    beam_load_set<R, TRL>(f, trs, set_v, na0);

    int t = 0;
    for (; t < n; ++t) {
        const int gt = pos + t;                             // the frame's index in the utterance
        const int na = ctl.na;
        if (gt >= 1 && na == 0) break;                      // an empty beam stays empty
        beam_frame<R, TRL>(f, gt == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bs, gt);
        if (tid == 0) cnt[gt] = ctl.na < K ? ctl.na : K;
    }
    for (int u = t + tid; u < n; u += kBT) cnt[pos + u] = 0;      // the frames the empty beam skipped

    const int na = beam_store_set<R>(f, set_v);
    if (tid == 0) { hdr[1] = na; hdr[0] = pos + n; }
}

// ascending sort of v[0 .. P2), P2 a power of two, by the whole workgroup of kBL threads
__device__ __forceinline__ void bitonic_sort_wg(int *v, int P2) {
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = threadIdx.x; x < P2; x += kBL) {
                const int y = x ^ j;
                if (y > x) {
                    const int a = v[x], c = v[y];
                    const bool up = (x & k) == 0;
                    if ((a > c) == up) { v[x] = c; v[y] = a; }
                }
            }
            __syncthreads();
        }
}

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
    int L = hdr[0];
    L = L < 0 ? 0 : (L > max_frames ? max_frames : L);
    int a0 = hdr[kHdrApos];
    a0 = a0 < 0 ? 0 : (a0 > L ? L : a0);
    if (a0 >= L) return;                                 // caught up (apos <= pos always: nothing to store)
    const int *bq = (const int *) wb;                    // the search's [max_frames][K] kept states
    const int *cnt = (const int *) (wb + lay.lat.cnt);
    int *nu = (int *) (wb + lay.lat.nu);
    int *U = (int *) (wb + lay.lat.U);
    R *A = (R *) (wb + lay.lat.A);
    const R *em = (const R *) (wb + lay.em);
    const R *trm = (const R *) P.transition;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };

    // ---- the sets: U_t = A_t ascending, nu[t] = |A_t|
    for (int t = a0; t < L; ++t) {
        int na = cnt[t];
        na = na < 0 ? 0 : (na > K ? K : na);
        int p2 = 2;
        while (p2 < na) p2 *= 2;
        for (int x = tid; x < p2; x += kBL) v[x] = x < na ? bq[(int64_t) t * K + x] : 0x7FFFFFFF;
        __syncthreads();
        bitonic_sort_wg(v, p2);
        int *Ut = U + (int64_t) t * K;
        for (int x = tid; x < na; x += kBL) Ut[x] = v[x];
        if (tid == 0) nu[t] = na;
        __syncthreads();                                 // v is the next frame's
    }
    __threadfence();
    __syncthreads();

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

// TokenLat with the end term of a prefix: a path may end in any kept state of the last set with weight 0.
template <typename R>
struct PrefixLat : TokenLat<R> {
    struct Args : TokenLat<R>::Args { int fin; };
    int fin;
    __device__ void bind(const Args &a) { TokenLat<R>::bind(a); fin = a.fin; }
    __device__ void end(int q, R &e) const { e = fin ? this->fw[q] : R(0); }
};

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
    const R NINF = Num<R>::ninf();
    const GraphArgs &g = args.g;
    char *wb = state + (size_t) b * lay.per;
    const int *hdr = (const int *) (wb + lay.st.hdr);
    const R *set_v = (const R *) (wb + lay.st.set);
    const int *set_q = (const int *) (set_v + K);
    const BeamWorkLayout wl = beam_work_layout(sizeof(R), T, g.Q, K, cap);
    const int *bq = (const int *) (wb + wl.bq), *bs = (const int *) (wb + wl.bs);             // [max_frames][K]
    long long *pb = path + (int64_t) b * T, *tk = tokens + (int64_t) b * T, *st = states + (int64_t) b * T;
    long long *tf = tframes + (int64_t) b * T;
    R *cf = conf + (int64_t) b * T;
    int len = hdr[0];
    len = len < 0 ? 0 : (len > T ? T : len);
    int na = len >= 1 ? hdr[1] : 0;
    na = na < 0 ? 0 : (na > K ? K : na);
    if (tid == 0) { frames[b] = len; status[b] = hdr[2] != 0; }
    const int fin = args.fin;
    const R *fw = fin ? (const R *) g.final_w : nullptr;

    // ---- the hypothesis: beam_stream_result_kernel's
    U bkey;
    int bqq, bk;
    beam_best_end<R>(ctl, set_q, set_v, na, fw, bkey, bqq, bk);
    if (bkey == 0) {                                        // no frame yet, an empty set, or no finite end
        beam_no_path(T, pb, tk, st, tlen + b);
        if (tid == 0) scores[b] = NINF;
    } else {
        if (tid == 0) scores[b] = fw ? set_v[bk] + fw[bqq] : set_v[bk];
        beam_backtrace(bq, bs, K, len, T, bk, g.label, g.state, pb, tk, st, tlen + b);
    }
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
    // ---- where the tokens start: the frames at which collapse_tokens kept a label (beam_conf_bwd's walk)
    for (int k = n + tid; k < T; k += kBL) tf[k] = -1;
    if (tid < 64 && n > 0) {
        int base = 0;
        long long carry = -1;
        for (int c0 = 0; c0 < len; c0 += 64) {
            const int t = c0 + tid;
            const long long cur = t < len ? pb[t] : -1;
            long long prv = __shfl_up(cur, 1);
            if (tid == 0) prv = carry;
            const bool keep = t < len && cur != prv;
            const unsigned long long m = __ballot(keep);
            const int pre = base + __popcll(m & ((1ull << tid) - 1ull));
            if (keep && pre < n) tf[pre] = t;
            base += __popcll(m);
            carry = __shfl(cur, 63);
        }
    }
    const int nw = Z > NINF ? n : 0;
    for (int k = nw + tid; k < T; k += kBL) cf[k] = R(0);
    if (nw == 0) return;
    for (int x = tid; x < kConfRing; x += kBL) ring[x] = 0ull;
    __threadfence();                                                           // the frames, for the windows of every wavefront
    HypSink<R> sink;
    sink.wd = tk; sink.wf = tf; sink.cf = cf; sink.ring = ring; sink.tol = tol;
    sink.ka = sink.kb = nw;
    beam_conf_pull<R, HypSink<R>, PrefixLat<R>>(P, args, wb, lay.beta, Z, len, -tol - 1, nq, nb, sink);
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

hipError_t launch_beam_conf_stream_reset(int elem, const GraphArgs &G, const BeamGraphArgs &BG, int K, int max_frames, int B, int N,
                                         void *state, const unsigned char *mask, hipStream_t stream) {
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const BeamConfStreamLayout lay = beam_conf_stream_layout(elem, max_frames, G.Q, K, cap, N);
    hipLaunchKernelGGL(beam_stream_conf_reset_kernel, dim3(B, reset_blocks(G.Q)), dim3(256), 0, stream, (char *) state, lay,
                       beam_work_layout(elem, max_frames, G.Q, K, cap), G.Q, elem, mask);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_conf_stream_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta,
                                           int max_frames, void *state, hipStream_t stream) {
    const int N = P.N;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const BeamConfStreamLayout lay = beam_conf_stream_layout(sizeof(R), max_frames, G.Q, K, cap, N);
    // the LDS of the one-shot decoder: control block, the set, and the transitions when they fit beside it
    const size_t beam = kFixedLds + (size_t) K * (sizeof(R) + 4) + 8;
    const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
    const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
#define ASG_BEAM_STREAM(TRL)                                                                                               \
    do {                                                                                                                   \
        const void *fn = (const void *) beam_stream_conf_advance_kernel<R, TRL>;                                          \
        if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);     \
        hipLaunchKernelGGL((beam_stream_conf_advance_kernel<R, TRL>), dim3(P.B), dim3(kBT), dyn, stream, P, G, BG, K,     \
                           (R) theta, cap, max_frames, (char *) state, lay);                                              \
    } while (0)
    if (trl) ASG_BEAM_STREAM(true); else ASG_BEAM_STREAM(false);
#undef ASG_BEAM_STREAM
    return hipGetLastError();
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
    template hipError_t launch_beam_conf_stream_advance<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, double,   \
                                                           int, void *, hipStream_t);                                              \
    template hipError_t launch_beam_conf_stream_confidence<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, int,   \
                                                              void *, int, int, void *, long long *, long long *, long long *,     \
                                                              long long *, long long *, void *, void *, long long *, long long *,  \
                                                              hipStream_t);
ASG_BEAM_CONF_STREAM_INST(float)
ASG_BEAM_CONF_STREAM_INST(double)
#undef ASG_BEAM_CONF_STREAM_INST

}  // namespace asg
