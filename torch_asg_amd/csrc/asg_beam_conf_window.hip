// torch_asg_amd/csrc/asg_beam_conf_window.hip -- the LATTICE-KEEPING window stream on gfx950: the windowed search of
// asg_beam_window.hip with a state that also keeps, in a RING, what the token confidences of asg_beam_conf.hip are computed from,
// so that a stream without an end can say how sure it is of a token at the moment it commits it.  The specification is
// include/asg_hip.h::asg_beam_conf_window_advance; tests/beam_window_conf_ref.py restates it in numpy.  DESIGN.md 5ag.
//
// One slot of the state (beam_conf_window_layout; every part 256-byte aligned): the plain window's slot unchanged at the front --
// the search's workspace for T = W, the header block, the stored set --; behind it the lattice ring of
//     RW = W + tol + 1 + C rows,  frame t in row t mod RW (computed in 64 bits),
// cnt int32 [RW] (|A_t|), the emissions [RW][N], nu int32 [RW], U int32 [RW][K] (A_t, ascending once caught up), A [RW][K]
// (alpha); the attempt log of nlog = C / P + 1 entries (WinAttempt); beta [nlog][2][K].  The header block also holds apos -- the
// frames whose U / nu / A rows are valid -- and the number of logged attempts (asg_beam_window_lat.h).  The ring is large enough:
// an attempt at p1 with old base b0 reads the frames b0 - tol - 1 .. p1 - 1 with p1 - b0 <= W, and the call has written at most C
// frames behind p1 when the pull runs.
// The search is NOT here.  Reset, result and n-best are the plain window's kernels with this layout's stride; the advance is
// beam_window_advance_kernel with the WinKeepLattice policy.  This unit holds the layout and three kernels:
//   beam_conf_window_catchup   one 1024-thread workgroup per slot, frames [apos, pos): the rows' kept states sorted in place
//                              (stream_lat_sets), then the frame body of asg_beam_alpha.inc resumed from row apos - 1; apos = pos.
//   beam_conf_window_pull      one workgroup per (slot, logged attempt): Z over row p1 - 1 with end weight 0, then
//                              beam_conf_pull<R, HypSink<R>, PrefixLat<R>, RingRows> from frame p1 - 1 down to max(b0 - tol, 0),
//                              with the frame-0 term when it gets there.  Its sink is the attempt's token range.  The pull counts
//                              frames from an origin below its last one, so its frames are ints however long the stream runs; the
//                              range's start frames are shifted by the origin for the pull and shifted back behind it.
//   beam_conf_window_tail      one workgroup per slot, behind the plain result kernel: the start frames of the tail's tokens, Z
//                              over row pos - 1 (with the final weights, or 0) and one pull from pos - 1 down to base - tol.
// An advance is three launches (search, catch-up, pull), a confidence call two (result, tail): no host synchronisation, no
// memset, no copy.  No float atomics; beta rows are per logged attempt, so the attempts of a call do not meet.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_frame.h"
#include "asg_beam_lattice.h"
#include "asg_beam_stream_lat.h"
#include "asg_beam_window_common.h"
#include "asg_beam_window_lat.h"
#include "asg_beam_token_lat.h"
#include "asg_beam_conf_sink.h"
#include "asg_beam_conf_pull.h"

namespace asg {

namespace {

// The rows of the pull's frames 0 .. len-1: frame t is frame org + t of the utterance, in row (org + t) mod RW (len <= RW).
struct RingRows {
    static constexpr bool kFlat = false;
    int orow, RW;
    bool at0;                    // org == 0 and the pull goes down to the utterance's first frame
    __device__ __forceinline__ int row(int t) const {
        const int r = orow + t;
        return r >= RW ? r - RW : r;
    }
    __device__ __forceinline__ bool first() const { return at0; }
};

// Dynamic LDS: [reduction slots][pa R K][pq int K] (beam_loss_fwd's), the sort's int [P2(K)] over the same bytes.
template <typename R>
__global__ void __launch_bounds__(kBL) beam_conf_window_catchup(Problem P, GraphArgs g, int K, int C, char *state,
                                                                BeamConfWindowLayout lay) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    R *pa = (R *) (lds + kBLHead);                       // [K] alpha[t-1] of U_{t-1}
    int *pq = (int *) (pa + K);                          // [K] U_{t-1}
    int *v = (int *) (lds + kBLHead);                    // the sort's slots, before pa / pq are used
    const int tid = threadIdx.x, b = blockIdx.x, N = P.N, RW = lay.RW;
    char *wb = state + (size_t) b * lay.per;
    const TokenWinHdr *hdr = (const TokenWinHdr *) (wb + lay.st.hdr);
    ConfWinHdr *ch = (ConfWinHdr *) (wb + lay.st.hdr + kConfWinHdrOff);
    long long L = hdr->pos;
    L = L < 0 ? 0 : L;
    long long a0 = ch->apos;
    a0 = a0 > L ? L : a0;
    a0 = a0 < L - C ? L - C : a0;                        // (an advance brings at most C frames)
    a0 = a0 < 0 ? 0 : a0;
    if (a0 >= L) return;                                 // caught up
    int *nu = (int *) (wb + lay.lat.nu);
    int *U = (int *) (wb + lay.lat.U);
    R *A = (R *) (wb + lay.lat.A);
    const R *em = (const R *) (wb + lay.em);
    const R *trm = (const R *) P.transition;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };

    // ---- the rows of [a0, L) sorted in place: at most two runs of rows (L - a0 <= C < RW)
    {
        const int r0 = (int) (a0 % RW), cntf = (int) (L - a0);
        const int e1 = r0 + cntf < RW ? r0 + cntf : RW, e2 = r0 + cntf - e1;
        auto key_of = [&](int t, int x) -> int { return U[(int64_t) t * K + x]; };
        stream_lat_sets<int>(r0, e1, K, (const int *) (wb + lay.lat.cnt), v, 0x7FFFFFFF, U, nu, key_of);
        if (e2 > 0) stream_lat_sets<int>(0, e2, K, (const int *) (wb + lay.lat.cnt), v, 0x7FFFFFFF, U, nu, key_of);
    }

    // ---- alpha, resumed: beam_loss_fwd's frame 0, or row a0 - 1 back into LDS; then the frame body it compiles
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
        const int rp = (int) ((a0 - 1) % RW);
        mp = nu[rp];
        const int *Up = U + (int64_t) rp * K;
        const R *Ap = A + (int64_t) rp * K;
        for (int x = tid; x < mp; x += kBL) { pq[x] = dev_load(Up + x); pa[x] = dev_load(Ap + x); }
    }
    __syncthreads();
    int r = (int) (a0 % RW);
    for (long long t = a0; t < L; ++t, r = r + 1 == RW ? 0 : r + 1) {
        const int mt = nu[r];
        const int *Ut = U + (int64_t) r * K;
        R *Arow = A + (int64_t) r * K;
        const R *xt = em + (int64_t) r * N;                // (P.is2 is 1: the stored rows are dense)
#include "asg_beam_alpha.inc"
    }
    if (tid == 0) ch->apos = L;
}

inline size_t conf_window_lds(int elem, int K) { return bwd_front(elem, 4, K) + (size_t) kConfRing * 8; }

// The pull over the ring for the tokens tk / tf / cf [0, n) of one lattice end: the paths over frames 0 .. p1 - 1 that end in a
// state of row p1 - 1 (end term by args.fin), the tokens' start frames tf absolute and >= b0.  Z: the normaliser of that end.
// The whole workgroup calls it.  nb / nq / ring: the dynamic LDS (bwd_front, then kConfRing words).
template <typename R>
__device__ __forceinline__ void conf_window_pull(const Problem &P, const typename PrefixLat<R>::Args &args, char *wb, size_t beta_off,
                                                 int RW, R Z, long long p1, long long b0, int tol, const long long *tk, long long *tf,
                                                 R *cf, int n, unsigned long long *ring, int *nq, R *nb) {
    const int tid = threadIdx.x;
    if (!(Z > Num<R>::ninf()) || n <= 0) {
        for (int k = tid; k < n; k += kBL) cf[k] = R(0);
        return;
    }
    const long long lo = b0 - tol > 0 ? b0 - tol : 0;       // the last frame whose events a window can hold
    const long long org = lo > 0 ? lo - 1 : 0;              // the pull's frame 0
    const int len = (int) (p1 - org);                       // <= W + tol + 1 < RW
    for (int k = tid; k < n; k += kBL) tf[k] -= org;
    for (int x = tid; x < kConfRing; x += kBL) ring[x] = 0ull;
    __threadfence();                                        // the frames, for the windows of every wavefront
    __syncthreads();
    HypSink<R> sink;
    sink.wd = tk; sink.wf = tf; sink.cf = cf; sink.ring = ring; sink.tol = tol;
    sink.ka = sink.kb = n;
    RingRows rows;
    rows.orow = (int) (org % RW); rows.RW = RW; rows.at0 = lo == 0;
    beam_conf_pull<R, HypSink<R>, PrefixLat<R>, RingRows>(P, args, wb, beta_off, Z, len, -tol - 1, nq, nb, sink, rows);
    __syncthreads();                                        // every thread has read the frames for the last time
    for (int k = tid; k < n; k += kBL) tf[k] += org;
}

// Dynamic LDS: [nb R K][nq int K][pad to 16][ring u64 256] (beam_conf_bwd's).  Block (slot, attempt).
template <typename R>
__global__ void __launch_bounds__(kBL) beam_conf_window_pull(Problem P, typename PrefixLat<R>::Args args, int K, int W, int tol,
                                                             char *state, BeamConfWindowLayout lay, long long cols,
                                                             const long long *new_tokens, const long long *new_tlen,
                                                             long long *new_tf, R *new_cf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ R red[kBL / 64];
    R *nb = (R *) lds;                                                         // [K] beta[t] of U_t
    int *nq = (int *) (lds + (size_t) K * sizeof(R));                          // [K] U_t
    unsigned long long *ring = (unsigned long long *) (lds + bwd_front(sizeof(R), 4, K));
    const int tid = threadIdx.x, b = blockIdx.x, y = blockIdx.y, RW = lay.RW;
    char *wb = state + (size_t) b * lay.per;
    const ConfWinHdr *ch = (const ConfWinHdr *) (wb + lay.st.hdr + kConfWinHdrOff);
    R *cf = new_cf + (int64_t) b * cols;
    if (y == 0) {                                           // behind the tokens: 0
        long long nt = new_tlen[b];
        nt = nt < 0 ? 0 : (nt > cols ? cols : nt);
        for (long long x = nt + tid; x < cols; x += kBL) cf[x] = R(0);
    }
    int nl = ch->nlog;
    nl = nl < 0 ? 0 : (nl > lay.nlog ? lay.nlog : nl);
    if (y >= nl) return;
    const WinAttempt at = ((const WinAttempt *) (wb + lay.log))[y];
    long long p1 = at.p1, b0 = at.b0;
    int k0 = at.k0, k1 = at.k1;
    // (a log the search wrote holds 1 <= p1, p1 - W <= b0 < p1 and 0 <= k0 < k1 <= cols)
    k1 = (long long) k1 > cols ? (int) cols : k1;
    k0 = k0 < 0 ? 0 : k0;
    if (p1 < 1 || k0 >= k1) return;
    b0 = b0 < p1 - W ? p1 - W : b0;
    b0 = b0 < 0 ? 0 : (b0 > p1 - 1 ? p1 - 1 : b0);

    const int rl = (int) ((p1 - 1) % RW);
    const R *Al = (const R *) (wb + lay.lat.A) + (int64_t) rl * K;
    int ml = ((const int *) (wb + lay.lat.nu))[rl];
    ml = ml < 0 ? 0 : (ml > K ? K : ml);
    const R Z = lattice_z<R>(ml, red, [&](int x) -> R { return Al[x]; });
    conf_window_pull<R>(P, args, wb, lay.beta + (size_t) y * a256(2 * (size_t) K * sizeof(R)), RW, Z, p1, b0, tol,
                        new_tokens + (int64_t) b * cols + k0, new_tf + (int64_t) b * cols + k0, cf + k0, k1 - k0, ring, nq, nb);
}

// Behind beam_window_result_kernel, which wrote path / tokens / tlen of the uncommitted tail: its tokens' start frames, Z, and
// the pull.  Same dynamic LDS.
template <typename R>
__global__ void __launch_bounds__(kBL) beam_conf_window_tail(Problem P, typename PrefixLat<R>::Args args, int K, int W, int tol,
                                                             char *state, BeamConfWindowLayout lay, const long long *path,
                                                             const long long *tokens, const long long *tlen, long long *tframes,
                                                             R *conf, R *Zs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ R red[kBL / 64];
    R *nb = (R *) lds;
    int *nq = (int *) (lds + (size_t) K * sizeof(R));
    unsigned long long *ring = (unsigned long long *) (lds + bwd_front(sizeof(R), 4, K));
    const int tid = threadIdx.x, b = blockIdx.x, RW = lay.RW;
    char *wb = state + (size_t) b * lay.per;
    const TokenWinHdr *hdr = (const TokenWinHdr *) (wb + lay.st.hdr);
    const R *fw = args.fin ? (const R *) args.g.final_w : nullptr;
    long long *tf = tframes + (int64_t) b * W;
    R *cf = conf + (int64_t) b * W;
    long long pos = hdr->pos, base = hdr->base;
    int na = hdr->na;
    window_header(pos, base, na, K);

    // ---- Z over the last set
    R Z = Num<R>::ninf();
    if (pos >= 1) {
        const int rl = (int) ((pos - 1) % RW);
        const int *Ul = (const int *) (wb + lay.lat.U) + (int64_t) rl * K;
        const R *Al = (const R *) (wb + lay.lat.A) + (int64_t) rl * K;
        int ml = ((const int *) (wb + lay.lat.nu))[rl];
        ml = ml < 0 ? 0 : (ml > K ? K : ml);
        Z = lattice_z<R>(ml, red, [&](int x) -> R { return fw ? Al[x] + fw[Ul[x]] : Al[x]; });
    }
    if (tid == 0) Zs[b] = Z;

    // ---- the tail's tokens and where they start
    long long l = tlen[b];
    int n = 0, live = 0;
    if (na > 0 && l > 0) {                                  // (an empty beam has no tail; pos - base may then pass W)
        base = window_live_base(pos, base, W);
        live = (int) (pos - base);
        n = (int) (l > live ? live : l);                    // (a tail of `live` frames starts at most that many tokens)
    }
    for (int k = n + tid; k < W; k += kBL) { tf[k] = -1; cf[k] = R(0); }
    if (n == 0) return;
    if (tid < 64) collapse_frames_from(path + (int64_t) b * W, live, hdr->carry, base, tf, tid);
    __threadfence();
    __syncthreads();
    conf_window_pull<R>(P, args, wb, lay.beta, RW, Z, pos, base, tol, tokens + (int64_t) b * W, tf, cf, n, ring, nq, nb);
}

}  // namespace

BeamConfWindowLayout beam_conf_window_layout(int elem, int W, int CP, int tol, int C, int Q, int K, int cap, int N) {
    BeamConfWindowLayout l{};
    l.st = beam_window_layout(elem, W, Q, K, cap);                        // the plain window's slot, at the front
    l.RW = W + tol + 1 + C;
    l.nlog = C / CP + 1;
    const size_t RW = (size_t) l.RW;
    size_t off = l.st.per;
    l.lat.M = K; l.lat.nf = 0;
    l.lat.hdr = l.st.hdr;
    l.lat.cnt = off; off += a256(RW * 4);
    l.em = off;      off += a256(RW * N * elem);
    l.lat.nu = off;  off += a256(RW * 4);
    l.lat.U = off;   off += a256(RW * K * 4);
    l.lat.A = off;   off += a256(RW * K * elem);
    l.lat.key = l.lat.qk = off;                                            // (no targets: nothing is forced)
    l.log = off;     off += a256((size_t) l.nlog * sizeof(WinAttempt));
    l.beta = off;    off += (size_t) l.nlog * a256(2 * (size_t) K * elem);
    l.per = l.st.per = l.lat.per = off;
    return l;
}

size_t beam_conf_window_state_bytes(int elem, int W, int CP, int tol, int C, int B, int Q, int K, int cap, int N) {
    return (size_t) B * beam_conf_window_layout(elem, W, CP, tol, C, Q, K, cap, N).per;
}

namespace {

// the pull reads the stored emissions as its inputs: row r of slot b at em + b * per + r * N
template <typename R>
Problem ring_problem(const Problem &P, const void *state, const BeamConfWindowLayout &lay) {
    Problem PS = P;
    PS.inputs = (const char *) state + lay.em;
    PS.is0 = P.N; PS.is1 = (int64_t) (lay.per / sizeof(R)); PS.is2 = 1;
    PS.T = lay.RW; PS.in_len = nullptr; PS.targets = nullptr; PS.tg_len = nullptr;
    return PS;
}

}  // namespace

template <typename R>
hipError_t launch_beam_conf_window_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta, int W,
                                           int CP, int tol, int C, void *state, long long *new_path, long long *new_states,
                                           long long *new_tokens, long long *new_frames, long long *new_tlen,
                                           long long *new_token_frames, void *new_token_conf, hipStream_t stream) {
    const int N = P.N;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const BeamConfWindowLayout lay = beam_conf_window_layout(sizeof(R), W, CP, tol, C, G.Q, K, cap, N);
    // (a) the search, with the keep hooks
    hipError_t e = launch_beam_window_advance<R>(P, G, BG, K, theta, W, CP, state, new_path, new_states, new_tokens, new_frames,
                                                 new_tlen, stream, &lay, new_token_frames);
    if (e != hipSuccess) return e;
    // (b) the catch-up over [apos, pos) in the ring
    int P2 = 2;
    while (P2 < K) P2 *= 2;
    Problem PC = P;                                                         // it reads the stored emissions: label stride 1
    PC.is2 = 1;
    size_t dyn = (size_t) K * (sizeof(R) + 4);
    if (dyn < (size_t) P2 * 4) dyn = (size_t) P2 * 4;
    dyn += kBLHead;
    set_lds((const void *) beam_conf_window_catchup<R>, dyn);
    hipLaunchKernelGGL((beam_conf_window_catchup<R>), dim3(P.B), dim3(kBL), dyn, stream, PC, G, K, C, (char *) state, lay);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (c) the pull, per logged attempt
    typename PrefixLat<R>::Args args{};
    args.g = G; args.bg = BG; args.lay = lay.lat; args.fin = 0;
    const size_t dyn2 = conf_window_lds(sizeof(R), K);
    set_lds((const void *) beam_conf_window_pull<R>, dyn2, sizeof(R) * (kBL / 64));
    hipLaunchKernelGGL((beam_conf_window_pull<R>), dim3(P.B, lay.nlog), dim3(kBL), dyn2, stream, ring_problem<R>(P, state, lay), args,
                       K, W, tol, (char *) state, lay, (long long) W + P.T, (const long long *) new_tokens,
                       (const long long *) new_tlen, new_token_frames, (R *) new_token_conf);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_conf_window_confidence(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, int W, int CP,
                                              int tol, int C, void *state, int final, void *scores, long long *path,
                                              long long *tokens, long long *tlen, long long *states, long long *token_frames,
                                              void *token_conf, void *normalisers, long long *frames, long long *committed,
                                              long long *status, hipStream_t stream) {
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const BeamConfWindowLayout lay = beam_conf_window_layout(sizeof(R), W, CP, tol, C, G.Q, K, cap, P.N);
    hipError_t e = launch_beam_window_result<R>(G, BG, K, W, P.B, state, final, scores, path, tokens, tlen, states, frames, committed,
                                                status, stream, lay.per);
    if (e != hipSuccess) return e;
    typename PrefixLat<R>::Args args{};
    args.g = G; args.bg = BG; args.lay = lay.lat; args.fin = final != 0;
    const size_t dyn = conf_window_lds(sizeof(R), K);
    set_lds((const void *) beam_conf_window_tail<R>, dyn, sizeof(R) * (kBL / 64));
    hipLaunchKernelGGL((beam_conf_window_tail<R>), dim3(P.B), dim3(kBL), dyn, stream, ring_problem<R>(P, state, lay), args, K, W, tol,
                       (char *) state, lay, (const long long *) path, (const long long *) tokens, (const long long *) tlen,
                       token_frames, (R *) token_conf, (R *) normalisers);
    return hipGetLastError();
}

#define ASG_BEAM_CONF_WINDOW_INST(R)                                                                                              \
    template hipError_t launch_beam_conf_window_advance<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, double,   \
                                                           int, int, int, int, void *, long long *, long long *, long long *,      \
                                                           long long *, long long *, long long *, void *, hipStream_t);            \
    template hipError_t launch_beam_conf_window_confidence<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, int,   \
                                                              int, int, int, void *, int, void *, long long *, long long *,        \
                                                              long long *, long long *, long long *, void *, void *, long long *,  \
                                                              long long *, long long *, hipStream_t);
ASG_BEAM_CONF_WINDOW_INST(float)
ASG_BEAM_CONF_WINDOW_INST(double)
#undef ASG_BEAM_CONF_WINDOW_INST

}  // namespace asg
