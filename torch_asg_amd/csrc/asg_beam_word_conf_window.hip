// torch_asg_amd/csrc/asg_beam_word_conf_window.hip -- the LATTICE-KEEPING word window stream on gfx950: the windowed search over
// pairs of asg_beam_word_window.hip with a state that also keeps, in a RING, what the word confidences of asg_beam_word_conf.hip
// are computed from, so that a word-LM stream without an end can say how sure it is of a word, and where the word ends, at the
// moment it commits it.  The specification is include/asg_hip.h::asg_beam_word_conf_window_advance;
// tests/beam_word_window_conf_ref.py restates it in numpy.  DESIGN.md 5ah.
//
// One slot of the state (beam_word_conf_window_layout; every part 256-byte aligned): the plain word window's slot unchanged at the
// front -- the search's workspace for T = W, the header block, the stored set --; behind it the lattice ring of
//     RW = W + tol + 1 + C rows,  frame t in row t mod RW (computed in 64 bits),
// cnt int32 [RW] (|A_t|), the emissions [RW][N], nu int32 [RW], U u64 [RW][K] (the pair keys h << qbits | q of A_t, ascending once
// caught up), A [RW][K] (alpha); the attempt log of nlog = C / CP + 1 entries (WinAttempt, with WORD ranges); beta [nlog][2][K].
// The header block also holds apos -- the frames whose U / nu / A rows are valid -- and the number of logged attempts
// (asg_beam_window_lat.h).  The ring is large enough: an attempt at p1 with old base b0 reads the frames b0 - tol - 1 .. p1 - 1 with
// p1 - b0 <= W, and the call has written at most C frames behind p1 when the pull runs.
// The search is NOT here.  Reset, result and n-best are the plain word window's kernels with this layout's stride; the advance is
// beam_word_window_advance_kernel, with or without the look-ahead flag, with the WinKeepLattice policy.  This unit holds the
// layout and three kernels, none of which reads a look-ahead (the lattice weighs the pairs plainly, as asg_beam_word_conf.hip does
// behind a look-ahead search):
//   beam_word_conf_window_catchup   one 1024-thread workgroup per slot, frames [apos, pos): the rows' pair keys sorted in place
//                                   (stream_lat_sets over the at most two runs of ring rows), then the frame body of
//                                   asg_beam_word_alpha.inc resumed from row apos - 1, frame 0 as beam_word_stream_conf_catchup
//                                   has it; apos = pos.
//   beam_word_conf_window_pull      one workgroup per (slot, logged attempt): Z over row p1 - 1 with end weight 0, then
//                                   beam_word_conf_pull<R, HypSink<R>, PrefixWordLat<R>, RingRows> from frame p1 - 1 down to
//                                   max(b0 - tol, 1).  Its sink is the attempt's word range.  The pull counts frames from an origin
//                                   just below its last one, so its frames are ints however long the stream runs; the range's
//                                   frames are shifted by the origin for the pull and shifted back behind it.
//   beam_word_conf_window_tail      one workgroup per slot, behind the plain result kernel: the separator frames of the tail's words
//                                   by the carried walk, the frame pos for a word the final step closes, Z over row pos - 1 (through
//                                   word_end with the final weights, or alpha alone) and one pull from pos - 1 down to base - tol.
// An advance is three launches (search, catch-up, pull), a confidence call two (result, tail): no host synchronisation, no
// memset, no copy.  No float atomics: integer maxima and fixed-point sums; beta rows are per logged attempt, so the attempts of a
// call do not meet.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"
#include "asg_beam_lattice.h"
#include "asg_beam_stream_lat.h"
#include "asg_beam_window_common.h"
#include "asg_beam_window_lat.h"
#include "asg_beam_word_lat.h"
#include "asg_beam_conf_sink.h"
#include "asg_beam_word_conf_pull.h"

namespace asg {

namespace {

inline size_t catchup_lds(int elem, int K) {
    size_t P2 = 2;
    while (P2 < (size_t) K) P2 *= 2;
    size_t dyn = (size_t) K * (16 + elem);                  // beam_word_loss_fwd's ut / sm / mk
    if (dyn < P2 * 8) dyn = P2 * 8;                         // the sort's slots
    return kBLHead + dyn;
}

// Dynamic LDS: [reduction slots][ut u64 K][sm u64 K][mk key K] (beam_word_loss_fwd's), the sort's u64 [P2(K)] over the same bytes.
template <typename R>
__global__ void __launch_bounds__(kBL) beam_word_conf_window_catchup(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, int K,
                                                                     int C, char *state, BeamWordConfWindowLayout lay) {
    using KT = Key<R>;
    using KU = typename KT::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int M = lay.lat.M;                                              // (= K)
    unsigned long long *ut = (unsigned long long *) (lds + kBLHead);      // [M] U_t
    unsigned long long *sm = ut + M;                                      // [M] sum of exp(c - max), 48 fractional bits
    KU *mk = (KU *) (sm + M);                                             // [M] max candidate as a key, 0: none
    unsigned long long *v = (unsigned long long *) (lds + kBLHead);       // the sort's slots, before ut / sm / mk are used
    const int tid = threadIdx.x, b = blockIdx.x, N = P.N, RW = lay.RW;
    char *wb = state + (size_t) b * lay.per;
    const WordWinHdr *hdr = (const WordWinHdr *) (wb + lay.st.hdr);
    ConfWinHdr *ch = (ConfWinHdr *) (wb + lay.st.hdr + kConfWinHdrOff);
    long long L = hdr->pos;
    L = L < 0 ? 0 : L;
    long long a0 = ch->apos;
    a0 = a0 > L ? L : a0;
    a0 = a0 < L - C ? L - C : a0;                        // (an advance brings at most C frames)
    a0 = a0 < 0 ? 0 : a0;
    if (a0 >= L) return;                                 // caught up
    int *nu = (int *) (wb + lay.lat.nu);
    unsigned long long *U = (unsigned long long *) (wb + lay.lat.U);
    R *A = (R *) (wb + lay.lat.A);
    const R *em = (const R *) (wb + lay.em);
    const R *trm = (const R *) P.transition;
    const R NINF = Num<R>::ninf();
    BeamWordFrame<R> f;
    bind_walk<R>(f, g, bg, lm);
    const unsigned long long qmask = (1ull << f.qbits) - 1ull;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };

    // ---- the rows of [a0, L) sorted in place: at most two runs of rows (L - a0 <= C < RW)
    {
        const int r0 = (int) (a0 % RW), cntf = (int) (L - a0);
        const int e1 = r0 + cntf < RW ? r0 + cntf : RW, e2 = r0 + cntf - e1;
        const int *cnt = (const int *) (wb + lay.lat.cnt);
        auto key_of = [&](int t, int x) -> unsigned long long { return U[(int64_t) t * K + x]; };
        stream_lat_sets<unsigned long long>(r0, e1, K, cnt, v, ~0ull, U, nu, key_of);
        if (e2 > 0) stream_lat_sets<unsigned long long>(0, e2, K, cnt, v, ~0ull, U, nu, key_of);
    }

    // ---- alpha, resumed: beam_word_loss_fwd's frame 0 (row 0), or mp of row a0 - 1; then the frame body it compiles
    int mp;
    if (a0 == 0) {
        mp = nu[0];
        for (int x = tid; x < mp; x += kBL) {
            const unsigned long long p = U[x];
            const int q = (int) (p & qmask), h = (int) (p >> f.qbits);
            dev_store(A + x, h == f.lstart ? f.sw[q] + em[f.label[q]] : NINF);
        }
        __threadfence();
        __syncthreads();
        a0 = 1;
    } else {
        mp = nu[(int) ((a0 - 1) % RW)];
        mp = mp < 0 ? 0 : (mp > K ? K : mp);               // (a state that was reset holds 0 .. K)
    }
    int r = (int) (a0 % RW), rp = (int) ((a0 - 1) % RW);
    for (long long t = a0; t < L; ++t, rp = r, r = r + 1 == RW ? 0 : r + 1) {
        const int mt = nu[r];
        const unsigned long long *Up = U + (int64_t) rp * M, *Ut = U + (int64_t) r * M;
        const R *Ap = A + (int64_t) rp * M;
        R *Arow = A + (int64_t) r * M;
        const R *xt = em + (int64_t) r * N;                // (P.is2 is 1: the stored rows are dense)
#include "asg_beam_word_alpha.inc"
    }
    if (tid == 0) ch->apos = L;
}

inline size_t conf_window_lds(int elem, int K) { return bwd_front(elem, 8, K) + (size_t) kConfRing * 8; }

// The pull over the ring for the words wd / wf / cf [0, n) of one lattice end: the paths over frames 0 .. p1 - 1 that end in a
// pair of row p1 - 1 (end term and the event of frame p1 by args.fin), the words' frames wf absolute and >= b0.  Z: the normaliser
// of that end.  The whole workgroup calls it.  nq / nb / ring: the dynamic LDS (bwd_front, then kConfRing words).
template <typename R>
__device__ __forceinline__ void conf_window_pull(const Problem &P, const typename PrefixWordLat<R>::Args &args, char *wb,
                                                 size_t beta_off, int RW, R Z, long long p1, long long b0, int tol, const long long *wd,
                                                 long long *wf, R *cf, int n, unsigned long long *ring, unsigned long long *nq,
                                                 R *nb) {
    const int tid = threadIdx.x;
    if (!(Z > Num<R>::ninf()) || n <= 0) {
        for (int k = tid; k < n; k += kBL) cf[k] = R(0);
        return;
    }
    const long long lo = b0 - tol > 1 ? b0 - tol : 1;       // the last frame whose events a window can hold (no word ends at 0)
    const long long org = lo - 1;                           // the pull's frame 0
    const int len = (int) (p1 - org);                       // <= W + tol + 1 < RW
    for (int k = tid; k < n; k += kBL) wf[k] -= org;
    for (int x = tid; x < kConfRing; x += kBL) ring[x] = 0ull;
    __threadfence();                                        // the frames, for the windows of every wavefront
    __syncthreads();
    HypSink<R> sink;
    sink.wd = wd; sink.wf = wf; sink.cf = cf; sink.ring = ring; sink.tol = tol;
    sink.ka = sink.kb = n;
    RingRows rows;
    rows.orow = (int) (org % RW); rows.RW = RW; rows.at0 = org == 0;
    beam_word_conf_pull<R, HypSink<R>, PrefixWordLat<R>, RingRows>(P, args, wb, beta_off, Z, len, -tol - 1, nq, nb, sink, rows);
    __syncthreads();                                        // every thread has read the frames for the last time
    for (int k = tid; k < n; k += kBL) wf[k] += org;
}

// Dynamic LDS: [nq u64 K][nb R K][pad to 16][ring u64 256] (beam_word_conf_bwd's).  Block (slot, attempt).
template <typename R>
__global__ void __launch_bounds__(kBL) beam_word_conf_window_pull(Problem P, typename PrefixWordLat<R>::Args args, int K, int W,
                                                                  int tol, char *state, BeamWordConfWindowLayout lay, long long cols,
                                                                  const long long *new_words, const long long *new_wlen,
                                                                  long long *new_wf, R *new_cf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ R red[kBL / 64];
    unsigned long long *nq = (unsigned long long *) lds;                      // [K] U_t
    R *nb = (R *) (lds + (size_t) K * 8);                                      // [K] beta[t] of U_t
    unsigned long long *ring = (unsigned long long *) (lds + bwd_front(sizeof(R), 8, K));
    const int tid = threadIdx.x, b = blockIdx.x, y = blockIdx.y, RW = lay.RW;
    char *wb = state + (size_t) b * lay.per;
    const ConfWinHdr *ch = (const ConfWinHdr *) (wb + lay.st.hdr + kConfWinHdrOff);
    R *cf = new_cf + (int64_t) b * cols;
    if (y == 0) {                                           // behind the words: 0
        long long nw = new_wlen[b];
        nw = nw < 0 ? 0 : (nw > cols ? cols : nw);
        for (long long x = nw + tid; x < cols; x += kBL) cf[x] = R(0);
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
    const R Z = lattice_z<R>(ml, red, [&](int x) -> R { return dev_load(Al + x); });
    conf_window_pull<R>(P, args, wb, lay.beta + (size_t) y * a256(2 * (size_t) K * sizeof(R)), RW, Z, p1, b0, tol,
                        new_words + (int64_t) b * cols + k0, new_wf + (int64_t) b * cols + k0, cf + k0, k1 - k0, ring, nq, nb);
}

// Behind beam_word_window_result_kernel, which wrote path / words / wlen of the uncommitted tail: its words' end frames, Z, and
// the pull.  Same dynamic LDS.
template <typename R>
__global__ void __launch_bounds__(kBL) beam_word_conf_window_tail(Problem P, typename PrefixWordLat<R>::Args args, int K, int W,
                                                                  int tol, char *state, BeamWordConfWindowLayout lay,
                                                                  const long long *path, const long long *words,
                                                                  const long long *wlen, long long *wframes, R *conf, R *Zs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ R red[kBL / 64];
    unsigned long long *nq = (unsigned long long *) lds;
    R *nb = (R *) (lds + (size_t) K * 8);
    unsigned long long *ring = (unsigned long long *) (lds + bwd_front(sizeof(R), 8, K));
    const int tid = threadIdx.x, b = blockIdx.x, RW = lay.RW;
    const R NINF = Num<R>::ninf();
    char *wb = state + (size_t) b * lay.per;
    const WordWinHdr *hdr = (const WordWinHdr *) (wb + lay.st.hdr);
    const bool fin = args.fin != 0;
    const R *fw = (const R *) args.g.final_w;
    long long *wf = wframes + (int64_t) b * W;
    R *cf = conf + (int64_t) b * W;
    long long pos = hdr->pos, base = hdr->base;
    int na = hdr->na;
    window_header(pos, base, na, K);

    // ---- Z over the last set: beam_word_loss_fwd's end through word_end, or alpha alone
    R Z = NINF;
    if (pos >= 1) {
        const int rl = (int) ((pos - 1) % RW);
        const unsigned long long *Ul = (const unsigned long long *) (wb + lay.lat.U) + (int64_t) rl * K;
        const R *Al = (const R *) (wb + lay.lat.A) + (int64_t) rl * K;
        int ml = ((const int *) (wb + lay.lat.nu))[rl];
        ml = ml < 0 ? 0 : (ml > K ? K : ml);
        BeamWordFrame<R> fz;
        bind_walk<R>(fz, args.g, args.bg, args.lm);
        const unsigned long long qmask = (1ull << fz.qbits) - 1ull;
        Z = lattice_z<R>(ml, red, [&](int x) -> R {
            const unsigned long long p = Ul[x];
            R e;
            int w;
            const R a = dev_load(Al + x);
            if (!fin) return a;
            if (!(a > NINF) || !word_end<R>(fz, fw, (int) (p >> fz.qbits), (int) (p & qmask), a, e, w)) return NINF;
            return e;
        });
    }
    if (tid == 0) Zs[b] = Z;

    // ---- the tail's words and where they end: the separators by the carried walk, then pos for the word of the final step
    long long l = wlen[b];
    int n = 0, live = 0;
    if (na > 0 && l > 0) {                                  // (an empty beam has no tail; pos - base may then pass W)
        base = window_live_base(pos, base, W);
        live = (int) (pos - base);
        n = (int) (l > W ? W : l);                          // (the result kernel wrote at most W words)
    }
    for (int k = n + tid; k < W; k += kBL) { wf[k] = -1; cf[k] = R(0); }
    if (n == 0) return;
    if (tid < 64) {
        // (a tail of `live` <= W frames has at most W separators; the count beyond n cannot happen: the result kernel counted them)
        const int ns = collapse_word_frames_from(path + (int64_t) b * W, live, hdr->carry, args.lm.sep, base, wf, tid);
        if (tid == 0 && ns < n) wf[ns] = pos;               // (at most one: the word the final step closes)
    }
    __threadfence();
    __syncthreads();
    conf_window_pull<R>(P, args, wb, lay.beta, RW, Z, pos, base, tol, words + (int64_t) b * W, wf, cf, n, ring, nq, nb);
}

}  // namespace

BeamWordConfWindowLayout beam_word_conf_window_layout(int elem, int W, int CP, int tol, int C, int K, int cap, int N) {
    BeamWordConfWindowLayout l{};
    l.st = beam_word_window_layout(elem, W, K, cap);                      // the plain word window's slot, at the front
    const BeamWordWorkLayout w = beam_word_work_layout(elem, W, K, cap, word_table_bits(cap));
    l.RW = W + tol + 1 + C;
    l.nlog = C / CP + 1;
    const size_t RW = (size_t) l.RW;
    size_t off = l.st.per;
    l.lat.M = K; l.lat.nf = 0;
    l.lat.bq = w.bq; l.lat.bh = w.bh;                                      // (the search's rings; the lattice passes read U)
    l.lat.hdr = l.st.hdr;
    l.lat.cnt = off; off += a256(RW * 4);
    l.em = off;      off += a256(RW * N * elem);
    l.lat.nu = off;  off += a256(RW * 4);
    l.lat.U = off;   off += a256(RW * K * 8);
    l.lat.A = off;   off += a256(RW * K * elem);
    l.lat.key = off;                                                      // (no targets: nothing is forced)
    l.log = off;     off += a256((size_t) l.nlog * sizeof(WinAttempt));
    l.beta = off;    off += (size_t) l.nlog * a256(2 * (size_t) K * elem);
    l.per = l.st.per = l.lat.per = off;
    return l;
}

size_t beam_word_conf_window_state_bytes(int elem, int W, int CP, int tol, int C, int B, int K, int cap, int N) {
    return (size_t) B * beam_word_conf_window_layout(elem, W, CP, tol, C, K, cap, N).per;
}

namespace {

// the pull reads the stored emissions as its inputs: row r of slot b at em + b * per + r * N
template <typename R>
Problem ring_problem(const Problem &P, const void *state, const BeamWordConfWindowLayout &lay) {
    Problem PS = P;
    PS.inputs = (const char *) state + lay.em;
    PS.is0 = P.N; PS.is1 = (int64_t) (lay.per / sizeof(R)); PS.is2 = 1;
    PS.T = lay.RW; PS.in_len = nullptr; PS.targets = nullptr; PS.tg_len = nullptr;
    return PS;
}

}  // namespace

template <typename R>
hipError_t launch_beam_word_conf_window_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                                const WordLookArgs *LA, int S, int K, double theta, int W, int CP, int tol, int C,
                                                void *state, long long *new_path, long long *new_states, long long *new_lm_states,
                                                long long *new_tokens, long long *new_words, long long *new_frames,
                                                long long *new_tlen, long long *new_wlen, long long *new_word_frames,
                                                void *new_word_conf, hipStream_t stream) {
    const int N = P.N;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const BeamWordConfWindowLayout lay = beam_word_conf_window_layout(sizeof(R), W, CP, tol, C, K, cap, N);
    // (a) the search, with the keep hooks
    hipError_t e = launch_beam_word_window_advance<R>(P, G, BG, LM, LA, S, K, theta, W, CP, state, new_path, new_states, new_lm_states,
                                                      new_tokens, new_words, new_frames, new_tlen, new_wlen, stream, &lay,
                                                      new_word_frames);
    if (e != hipSuccess) return e;
    // (b) the catch-up over [apos, pos) in the ring
    Problem PC = P;                                                         // it reads the stored emissions: label stride 1
    PC.is2 = 1;
    const size_t dyn = catchup_lds(sizeof(R), K);
    set_lds((const void *) beam_word_conf_window_catchup<R>, dyn);
    hipLaunchKernelGGL((beam_word_conf_window_catchup<R>), dim3(P.B), dim3(kBL), dyn, stream, PC, G, BG, LM, K, C, (char *) state, lay);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (c) the pull, per logged attempt
    typename PrefixWordLat<R>::Args args{};
    args.g = G; args.bg = BG; args.lm = LM; args.lay = lay.lat; args.fin = 0;
    const size_t dyn2 = conf_window_lds(sizeof(R), K);
    set_lds((const void *) beam_word_conf_window_pull<R>, dyn2, sizeof(R) * (kBL / 64));
    hipLaunchKernelGGL((beam_word_conf_window_pull<R>), dim3(P.B, lay.nlog), dim3(kBL), dyn2, stream, ring_problem<R>(P, state, lay),
                       args, K, W, tol, (char *) state, lay, (long long) W + P.T, (const long long *) new_words,
                       (const long long *) new_wlen, new_word_frames, (R *) new_word_conf);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_word_conf_window_confidence(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG,
                                                   const WordLmArgs &LM, const WordLookArgs *LA, int S, int K, int W, int CP, int tol,
                                                   int C, void *state, int final, void *scores, long long *path, long long *tokens,
                                                   long long *tlen, long long *states, long long *lm_states, long long *words,
                                                   long long *wlen, long long *word_frames, void *word_conf, void *normalisers,
                                                   long long *frames, long long *committed, long long *status, hipStream_t stream) {
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const BeamWordConfWindowLayout lay = beam_word_conf_window_layout(sizeof(R), W, CP, tol, C, K, cap, P.N);
    hipError_t e = launch_beam_word_window_result<R>(G, BG, LM, LA, S, K, W, P.B, state, final, scores, path, tokens, tlen, states,
                                                     lm_states, words, wlen, frames, committed, status, stream, lay.per);
    if (e != hipSuccess) return e;
    typename PrefixWordLat<R>::Args args{};
    args.g = G; args.bg = BG; args.lm = LM; args.lay = lay.lat; args.fin = final != 0;
    const size_t dyn = conf_window_lds(sizeof(R), K);
    set_lds((const void *) beam_word_conf_window_tail<R>, dyn, sizeof(R) * (kBL / 64));
    hipLaunchKernelGGL((beam_word_conf_window_tail<R>), dim3(P.B), dim3(kBL), dyn, stream, ring_problem<R>(P, state, lay), args, K, W,
                       tol, (char *) state, lay, (const long long *) path, (const long long *) words, (const long long *) wlen,
                       word_frames, (R *) word_conf, (R *) normalisers);
    return hipGetLastError();
}

#define ASG_BEAM_WORD_CONF_WINDOW_INST(R)                                                                                          \
    template hipError_t launch_beam_word_conf_window_advance<R>(                                                                   \
        const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, const WordLookArgs *, int, int, double, int, \
        int, int, int, void *, long long *, long long *, long long *, long long *, long long *, long long *, long long *,          \
        long long *, long long *, void *, hipStream_t);                                                                            \
    template hipError_t launch_beam_word_conf_window_confidence<R>(                                                                \
        const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, const WordLookArgs *, int, int, int, int,   \
        int, int, void *, int, void *, long long *, long long *, long long *, long long *, long long *, long long *, long long *,  \
        long long *, void *, void *, long long *, long long *, long long *, hipStream_t);
ASG_BEAM_WORD_CONF_WINDOW_INST(float)
ASG_BEAM_WORD_CONF_WINDOW_INST(double)
#undef ASG_BEAM_WORD_CONF_WINDOW_INST

}  // namespace asg
