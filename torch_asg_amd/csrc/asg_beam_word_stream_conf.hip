// torch_asg_amd/csrc/asg_beam_word_stream_conf.hip -- the LATTICE-KEEPING word-LM beam stream on gfx950: the streaming search over
// pairs of asg_beam_word_stream.hip with a state that also keeps what the word confidences of asg_beam_word_conf.hip are computed
// from, so that a stream can say how sure it is of a word while the utterance is still arriving.  The specification is
// include/asg_hip.h::asg_beam_word_conf_stream_confidence; tests/beam_word_stream_conf_ref.py restates it in numpy.  DESIGN.md 5ae.
//
// One slot of the state (beam_word_conf_stream_layout; every part 256-byte aligned): the plain word stream's slot unchanged at the
// front -- the search's workspace for T = max_frames, the header, the stored set -- so that beam_word_stream_result_kernel and the
// word n-best kernels run on it as they are (their launchers take the slot stride); behind it cnt int32 [max_frames] (|A_t|), the
// emissions [max_frames][N], nu int32 [max_frames], U u64 [max_frames][K] (the pair keys h << qbits | q of A_t, ascending), A
// [max_frames][K] (alpha) and two rows of beta.  The header's word 3 is apos: the frames whose U / nu / A rows are valid.
//   beam_word_stream_conf_reset_kernel    the plain reset, and apos = 0.
//   beam_word_stream_conf_advance_kernel  beam_word_stream_advance_kernel's frame loop (beam_word_frame: the same sets and values,
//                                         with or without the look-ahead flag), which also writes cnt[gt] of every frame of the
//                                         chunk -- 0 for the frames an empty beam skips -- and copies the chunk's emissions into
//                                         rows pos .. pos+n-1 (coalesced, the whole workgroup).
//   beam_word_stream_conf_catchup         one 1024-thread workgroup per slot, frames [apos, pos) read from the header: U_t = the
//                                         keys of A_t sorted (bitonic in LDS; the kept pairs of a frame are distinct, so the
//                                         ascending list is what beam_loss_sets<WordSets> leaves without targets), then the frame
//                                         body of asg_beam_word_alpha.inc (the text beam_word_loss_fwd compiles), which reads row
//                                         t-1 of U and A from the state as the one-shot kernel reads them from its workspace:
//                                         resuming needs mp = nu[apos-1] and nothing else; then apos = pos.  LAZY: it runs in front
//                                         of a confidence call, every frame's alpha is computed once however often confidences are
//                                         asked for, and what it writes depends on nothing but the frames.
//   beam_word_stream_conf_bwd             one workgroup per slot: the winner and backtrace of beam_word_stream_result_kernel (with
//                                         or without the end terms), word_frames by beam_word_conf_search's serial walk, Z by
//                                         lattice_z over the last set, and beam_word_conf_pull<R, HypSink<R>> over the stored
//                                         emissions.  The one new thing is the end of a PREFIX (weight 0, no event at frame len),
//                                         which the pull takes as its lattice type (PrefixWordLat), so asg_beam_word_conf.hip's
//                                         text is unchanged.
// The lattice pass weighs the pairs plainly, as asg_beam_word_conf.hip does behind a look-ahead search: only the advance and the
// winner of the bwd read the look-ahead.  A confidence call is two launches (catch-up, bwd): no host synchronisation, no memset,
// no copy.  No float atomics: integer maxima and fixed-point sums, the same adds in the same order as asg_beam_words_confidence.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"
#include "asg_beam_lattice.h"
#include "asg_beam_word_lat.h"
#include "asg_beam_word_conf_pull.h"
#include "asg_beam_conf_sink.h"

namespace asg {

namespace {

constexpr int kHdrApos = 3;                     // header: int32 pos, |A|, overflow, apos

__global__ void __launch_bounds__(256) beam_word_stream_conf_reset_kernel(char *state, BeamWordConfStreamLayout lay,
                                                                           BeamWordWorkLayout wl, unsigned C, int key_bytes,
                                                                           const unsigned char *mask) {
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;
    char *wb = state + (size_t) b * lay.per;
    beam_word_reset_tables(wb, wl, C, key_bytes);
    if (blockIdx.y == 0 && threadIdx.x < 4) ((int *) (wb + lay.st.hdr))[threadIdx.x] = 0;   // pos, |A|, overflow, apos
}

template <typename R, bool TRL, bool LA>
__global__ void __launch_bounds__(kBT) beam_word_stream_conf_advance_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm,
                                                                            int K, R theta, int cap, int tbits, int max_frames,
                                                                            char *state, BeamWordConfStreamLayout lay,
                                                                            WordLookParam<LA> la) {
    using KT = Key<R>;
    using U = typename KT::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Ctl<U> &ctl = *(Ctl<U> *) lds;
    WordCtl &wctl = *(WordCtl *) (lds + kWordCtlOff);
    R *cur_v = (R *) (lds + kFixedLds);                    // [K]
    int *cur_q = (int *) (cur_v + K);                      // [K]
    int *cur_h = cur_q + K;                                // [K]
    R *trs = (R *) (cur_h + K);                            // [N][N] if TRL (2 * K ints: aligned)
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = P.N;
    char *wb = state + (size_t) b * lay.per;
    int *hdr = (int *) (wb + lay.st.hdr);
    R *set_v = (R *) (wb + lay.st.set);                     // values [K], then product states [K], then LM states [K]
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
    BeamWordFrame<R, LA> f;
    f.ctl = &ctl; f.wctl = &wctl; f.cur_v = cur_v; f.cur_q = cur_q; f.cur_h = cur_h; f.trs = trs; f.tr = tr;
    f.ts0 = P.ts0; f.ts1 = P.ts1; f.N = N; f.theta = theta;
    bind_graph<R>(f, g, bg, lm, K, cap, tbits);
    bind_look<R>(f, la);
    int *bq, *bh, *bs;
    f.bind_work(wb, max_frames, bq, bh, bs);

    int na0 = pos >= 1 ? hdr[1] : 0;
    na0 = na0 < 0 ? 0 : (na0 > K ? K : na0);
    beam_word_load_set<R, TRL, LA>(f, trs, set_v, na0);

    int t = 0;
    for (; t < n; ++t) {
        const int gt = pos + t;                             // the frame's index in the utterance
        const int na = ctl.na;
        if (gt >= 1 && na == 0) break;                      // an empty beam stays empty (pos still advances)
        beam_word_frame<R, TRL, LA>(f, gt == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bh, bs, gt);
        if (tid == 0) cnt[gt] = ctl.na < K ? ctl.na : K;
    }
    for (int u = t + tid; u < n; u += kBT) cnt[pos + u] = 0;      // the frames the empty beam skipped

    const int na = beam_word_store_set<R, LA>(f, set_v);
    if (tid == 0) { hdr[1] = na; hdr[0] = pos + n; }
}

// ascending sort of v[0 .. P2), P2 a power of two, by the whole workgroup of kBL threads
__device__ __forceinline__ void bitonic_sort_wg(unsigned long long *v, int P2) {
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = threadIdx.x; x < P2; x += kBL) {
                const int y = x ^ j;
                if (y > x) {
                    const unsigned long long a = v[x], c = v[y];
                    const bool up = (x & k) == 0;
                    if ((a > c) == up) { v[x] = c; v[y] = a; }
                }
            }
            __syncthreads();
        }
}

inline size_t catchup_lds(int elem, int K) {
    size_t P2 = 2;
    while (P2 < (size_t) K) P2 *= 2;
    size_t dyn = (size_t) K * (16 + elem);                  // beam_word_loss_fwd's ut / sm / mk
    if (dyn < P2 * 8) dyn = P2 * 8;                         // the sort's slots
    return kBLHead + dyn;
}

// Dynamic LDS: [reduction slots][ut u64 K][sm u64 K][mk key K] (beam_word_loss_fwd's), the sort's u64 [P2(K)] over the same bytes.
template <typename R>
__global__ void __launch_bounds__(kBL) beam_word_stream_conf_catchup(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, int K,
                                                                     int max_frames, char *state, BeamWordConfStreamLayout lay) {
    using KT = Key<R>;
    using KU = typename KT::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int M = lay.lat.M;                                              // (= K)
    unsigned long long *ut = (unsigned long long *) (lds + kBLHead);      // [M] U_t
    unsigned long long *sm = ut + M;                                      // [M] sum of exp(c - max), 48 fractional bits
    KU *mk = (KU *) (sm + M);                                             // [M] max candidate as a key, 0: none
    unsigned long long *v = (unsigned long long *) (lds + kBLHead);       // the sort's slots, before ut / sm / mk are used
    const int tid = threadIdx.x, b = blockIdx.x, N = P.N;
    char *wb = state + (size_t) b * lay.per;
    int *hdr = (int *) (wb + lay.st.hdr);
    int L = hdr[0];
    L = L < 0 ? 0 : (L > max_frames ? max_frames : L);
    int a0 = hdr[kHdrApos];
    a0 = a0 < 0 ? 0 : (a0 > L ? L : a0);
    if (a0 >= L) return;                                 // caught up (apos <= pos always: nothing to store)
    const int *bq = (const int *) (wb + lay.lat.bq), *bh = (const int *) (wb + lay.lat.bh);   // the search's [max_frames][K] pairs
    const int *cnt = (const int *) (wb + lay.lat.cnt);
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

    // ---- the sets: U_t = the keys of A_t ascending, nu[t] = |A_t|
    for (int t = a0; t < L; ++t) {
        int na = cnt[t];
        na = na < 0 ? 0 : (na > K ? K : na);
        int p2 = 2;
        while (p2 < na) p2 *= 2;
        for (int x = tid; x < p2; x += kBL) {
            const int64_t at = (int64_t) t * K + x;
            v[x] = x < na ? f.pair(bh[at], bq[at]) : ~0ull;
        }
        __syncthreads();
        bitonic_sort_wg(v, p2);
        unsigned long long *Ut = U + (int64_t) t * M;
        for (int x = tid; x < na; x += kBL) Ut[x] = v[x];
        if (tid == 0) nu[t] = na;
        __syncthreads();                                 // v is the next frame's
    }
    __threadfence();
    __syncthreads();

    // ---- alpha, resumed: beam_word_loss_fwd's frame 0, or mp of row a0 - 1; then the frame body it compiles
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
        mp = nu[a0 - 1];
        mp = mp < 0 ? 0 : (mp > K ? K : mp);               // (a state that was reset holds 0 .. K)
    }
    for (int t = a0; t < L; ++t) {
        const int mt = nu[t];
        const unsigned long long *Up = U + (int64_t) (t - 1) * M, *Ut = U + (int64_t) t * M;
        const R *Ap = A + (int64_t) (t - 1) * M;
        R *Arow = A + (int64_t) t * M;
        const R *xt = em + (int64_t) t * N;                // (P.is2 is 1: the stored rows are dense)
#include "asg_beam_word_alpha.inc"
    }
    if (tid == 0) hdr[kHdrApos] = L;
}

// WordLat with the end of a prefix: a path may end in any kept pair of the last set with weight 0, and no word completes at
// frame len (there is no final step).
template <typename R>
struct PrefixWordLat : WordLat<R> {
    using Key = typename WordLat<R>::Key;
    struct Args : WordLat<R>::Args { int fin; };
    int fin;
    __device__ void bind(const Args &a) { WordLat<R>::bind(a); fin = a.fin; }
    __device__ void end(Key p, R &e) const {
        if (fin) WordLat<R>::end(p, e); else e = R(0);
    }
    __device__ bool end_event() const { return fin != 0; }
};

inline size_t stream_conf_lds(int elem, int K) { return bwd_front(elem, 8, K) + (size_t) kConfRing * 8; }

// Dynamic LDS: [nq u64 K][nb R K][pad to 16][ring u64 256] (beam_word_conf_bwd's).
template <typename R, bool LA>
__global__ void __launch_bounds__(kBL) beam_word_stream_conf_bwd(Problem P, typename PrefixWordLat<R>::Args args, int K, int cap,
                                                                 int tbits, int max_frames, char *state, BeamWordConfStreamLayout lay,
                                                                 int tol, R *scores, long long *path, long long *tokens,
                                                                 long long *tlen, long long *states, long long *lm_states,
                                                                 long long *words, long long *wlen, long long *wframes, R *conf,
                                                                 R *Zs, long long *frames, long long *status, WordLookParam<LA> la) {
    using U = typename Key<R>::U;
    using KeyT = unsigned long long;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ WordCtl wctl;
    __shared__ R red[kBL / 64];
    KeyT *nq = (KeyT *) lds;                                                   // [K] U_t
    R *nb = (R *) (lds + (size_t) K * sizeof(KeyT));                           // [K] beta[t] of U_t
    unsigned long long *ring = (unsigned long long *) (lds + bwd_front(sizeof(R), sizeof(KeyT), K));
    const int tid = threadIdx.x, b = blockIdx.x, T = max_frames;
    const R NINF = Num<R>::ninf();
    char *wb = state + (size_t) b * lay.per;
    const int *hdr = (const int *) (wb + lay.st.hdr);
    const R *set_v = (const R *) (wb + lay.st.set);
    const int *set_q = (const int *) (set_v + K);
    const int *set_h = set_q + K;
    long long *pb = path + (int64_t) b * T, *tk = tokens + (int64_t) b * T, *st = states + (int64_t) b * T;
    long long *ls = lm_states + (int64_t) b * T, *wd = words + (int64_t) b * T, *wf = wframes + (int64_t) b * T;
    R *cf = conf + (int64_t) b * T;
    BeamWordFrame<R, LA> f;
    f.ctl = nullptr; f.wctl = &wctl; f.cur_v = nullptr; f.cur_q = nullptr; f.cur_h = nullptr; f.trs = nullptr; f.tr = nullptr;
    f.ts0 = 0; f.ts1 = 0; f.N = 0; f.theta = (R) 0;
    bind_graph<R>(f, args.g, BeamGraphArgs{}, args.lm, K, cap, tbits);
    bind_look<R>(f, la);
    int *bq, *bh, *bs;
    f.bind_work(wb, T, bq, bh, bs);
    int len = hdr[0];
    len = len < 0 ? 0 : (len > T ? T : len);
    int na = len >= 1 ? hdr[1] : 0;
    na = na < 0 ? 0 : (na > K ? K : na);
    if (tid == 0) { frames[b] = len; status[b] = hdr[2] != 0; }
    const bool fin = args.fin != 0;
    const R *fw = (const R *) args.g.final_w;

    // ---- the hypothesis: beam_word_stream_result_kernel's
    U bkey;
    int bk;
    word_best_end<R, LA>(f, fw, fin, set_h, set_q, set_v, na, bkey, bk);
    if (bkey == 0) {                                        // no frame yet, an empty set, or no finite end
        word_no_path(T, pb, tk, st, ls, wd, tlen + b, wlen + b);
        if (tid == 0) scores[b] = NINF;
        for (int u = tid; u < T; u += kBL) wf[u] = -1;
    } else {
        word_backtrace<R, LA>(f, fw, fin, set_h, set_q, set_v, bk, bq, bh, bs, len, T, scores + b, pb, tk, st, ls, wd, tlen + b,
                              wlen + b);
        // ---- where the words end: the frames of the separator edges word_backtrace read its words from, then len for the word
        // of the final step (a prefix has none: its word count is the separator count)
        for (int u = tid; u < T; u += kBL) wf[u] = -1;
        __threadfence();
        __syncthreads();
        if (tid == 0) {
            int nw = 0;
            for (int u = 1; u < len; ++u)
                if (pb[u] == f.sep && pb[u - 1] != f.sep) wf[nw++] = u;
            if (nw < (int) wlen[b]) wf[nw] = len;
        }
    }
    __threadfence();
    __syncthreads();                                        // words, their count and their frames, for every wavefront

    // ---- Z over the last set: beam_word_loss_fwd's end through word_end, or alpha alone
    const KeyT *Ul = (const KeyT *) (wb + lay.lat.U) + (int64_t) (len >= 1 ? len - 1 : 0) * K;
    const R *Al = (const R *) (wb + lay.lat.A) + (int64_t) (len >= 1 ? len - 1 : 0) * K;
    int ml = len >= 1 ? ((const int *) (wb + lay.lat.nu))[len - 1] : 0;
    ml = ml < 0 ? 0 : (ml > K ? K : ml);
    BeamWordFrame<R> fz;
    bind_walk<R>(fz, args.g, args.bg, args.lm);
    const KeyT qmask = (1ull << fz.qbits) - 1ull;
    auto end_of = [&](int x) -> R {
        const KeyT p = Ul[x];
        R e;
        int w;
        const R a = dev_load(Al + x);
        if (!fin) return a;
        if (!(a > NINF) || !word_end<R>(fz, fw, (int) (p >> fz.qbits), (int) (p & qmask), a, e, w)) return NINF;
        return e;
    };
    const R Z = lattice_z<R>(ml, red, end_of);
    if (tid == 0) Zs[b] = Z;

    int nw = 0;
    if (len >= 1 && Z > NINF) {
        const long long n = dev_load(wlen + b);
        nw = (int) (n < 0 ? 0 : (n > len ? len : n));                          // (a path of len frames ends at most len words)
    }
    for (int k = nw + tid; k < T; k += kBL) cf[k] = R(0);
    if (nw == 0) return;
    for (int x = tid; x < kConfRing; x += kBL) ring[x] = 0ull;
    HypSink<R> sink;
    sink.wd = wd; sink.wf = wf; sink.cf = cf; sink.ring = ring; sink.tol = tol;
    sink.ka = sink.kb = nw;
    beam_word_conf_pull<R, HypSink<R>, PrefixWordLat<R>>(P, args, wb, lay.beta, Z, len, -tol - 1, nq, nb, sink);
}

}  // namespace

BeamWordConfStreamLayout beam_word_conf_stream_layout(int elem, int max_frames, int K, int cap, int N) {
    BeamWordConfStreamLayout l{};
    l.st = beam_word_stream_layout(elem, max_frames, K, cap);            // the plain word stream's slot, at the front
    const BeamWordWorkLayout w = beam_word_work_layout(elem, max_frames, K, cap, word_table_bits(cap));
    const size_t T = (size_t) max_frames;
    size_t off = l.st.per;
    l.lat.M = K; l.lat.nf = 0;
    l.lat.bq = w.bq; l.lat.bh = w.bh;
    l.lat.hdr = l.st.hdr;
    l.lat.cnt = off; off += a256(T * 4);
    l.em = off;      off += a256(T * N * elem);
    l.lat.nu = off;  off += a256(T * 4);
    l.lat.U = off;   off += a256(T * K * 8);
    l.lat.A = off;   off += a256(T * K * elem);
    l.lat.key = off;                                                      // (no targets: nothing is forced)
    l.beta = off;    off += a256(2 * (size_t) K * elem);
    l.per = l.st.per = l.lat.per = off;
    return l;
}

size_t beam_word_conf_stream_state_bytes(int elem, int max_frames, int B, int K, int cap, int N) {
    return (size_t) B * beam_word_conf_stream_layout(elem, max_frames, K, cap, N).per;
}

hipError_t launch_beam_word_conf_stream_reset(int elem, const BeamGraphArgs &BG, int K, int max_frames, int B, int N, void *state,
                                              const unsigned char *mask, hipStream_t stream) {
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const BeamWordConfStreamLayout lay = beam_word_conf_stream_layout(elem, max_frames, K, cap, N);
    const int tbits = word_table_bits(cap);
    const size_t C = (size_t) 1 << tbits;
    hipLaunchKernelGGL(beam_word_stream_conf_reset_kernel, dim3(B, reset_blocks(C)), dim3(256), 0, stream, (char *) state, lay,
                       beam_word_work_layout(elem, max_frames, K, cap, tbits), (unsigned) C, elem, mask);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_word_conf_stream_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                                const WordLookArgs *LA, int K, double theta, int max_frames, void *state,
                                                hipStream_t stream) {
    const int N = P.N;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const int tbits = word_table_bits(cap);
    const BeamWordConfStreamLayout lay = beam_word_conf_stream_layout(sizeof(R), max_frames, K, cap, N);
    // the LDS of the one-shot decoder: control block, the set, and the transitions when they fit beside it
    const size_t beam = kFixedLds + (size_t) K * (sizeof(R) + 8);
    const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
    const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
#define ASG_BEAM_WORD_STREAM(TRL, LAF, LOOK)                                                                                      \
    do {                                                                                                                          \
        const void *fn = (const void *) beam_word_stream_conf_advance_kernel<R, TRL, LAF>;                                       \
        if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);            \
        hipLaunchKernelGGL((beam_word_stream_conf_advance_kernel<R, TRL, LAF>), dim3(P.B), dim3(kBT), dyn, stream, P, G, BG, LM, \
                           K, (R) theta, cap, tbits, max_frames, (char *) state, lay, LOOK);                                      \
    } while (0)
    if (LA) { if (trl) ASG_BEAM_WORD_STREAM(true, true, *LA); else ASG_BEAM_WORD_STREAM(false, true, *LA); }
    else if (trl) ASG_BEAM_WORD_STREAM(true, false, WordNoLook{}); else ASG_BEAM_WORD_STREAM(false, false, WordNoLook{});
#undef ASG_BEAM_WORD_STREAM
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_word_conf_stream_confidence(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG,
                                                   const WordLmArgs &LM, const WordLookArgs *LA, int K, int max_frames, void *state,
                                                   int final, int tol, void *scores, long long *path, long long *tokens,
                                                   long long *tlen, long long *states, long long *lm_states, long long *words,
                                                   long long *wlen, long long *word_frames, void *word_conf, void *normalisers,
                                                   long long *frames, long long *status, hipStream_t stream) {
    const int N = P.N;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const int tbits = word_table_bits(cap);
    const BeamWordConfStreamLayout lay = beam_word_conf_stream_layout(sizeof(R), max_frames, K, cap, N);
    Problem PC = P;                                                         // the catch-up reads the stored emissions: label stride 1
    PC.is2 = 1;
    const size_t dyn = catchup_lds(sizeof(R), K);
    set_lds((const void *) beam_word_stream_conf_catchup<R>, dyn);
    hipLaunchKernelGGL((beam_word_stream_conf_catchup<R>), dim3(P.B), dim3(kBL), dyn, stream, PC, G, BG, LM, K, max_frames,
                       (char *) state, lay);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the pull reads the stored emissions as its inputs: frame t of slot b at em + b * per + t * N
    Problem PS = P;
    PS.inputs = (const char *) state + lay.em;
    PS.is0 = N; PS.is1 = (int64_t) (lay.per / sizeof(R)); PS.is2 = 1;
    PS.T = max_frames; PS.in_len = nullptr; PS.targets = nullptr; PS.tg_len = nullptr;
    typename PrefixWordLat<R>::Args args{};
    args.g = G; args.bg = BG; args.lm = LM; args.lay = lay.lat; args.fin = final != 0;
    const size_t dyn2 = stream_conf_lds(sizeof(R), K);
#define ASG_BEAM_WORD_STREAM_CONF(LAF, LOOK)                                                                                      \
    do {                                                                                                                          \
        set_lds((const void *) beam_word_stream_conf_bwd<R, LAF>, dyn2, sizeof(WordCtl) + sizeof(R) * (kBL / 64));               \
        hipLaunchKernelGGL((beam_word_stream_conf_bwd<R, LAF>), dim3(P.B), dim3(kBL), dyn2, stream, PS, args, K, cap, tbits,     \
                           max_frames, (char *) state, lay, tol, (R *) scores, path, tokens, tlen, states, lm_states, words,     \
                           wlen, word_frames, (R *) word_conf, (R *) normalisers, frames, status, LOOK);                          \
    } while (0)
    if (LA) ASG_BEAM_WORD_STREAM_CONF(true, *LA); else ASG_BEAM_WORD_STREAM_CONF(false, WordNoLook{});
#undef ASG_BEAM_WORD_STREAM_CONF
    return hipGetLastError();
}

#define ASG_BEAM_WORD_CONF_STREAM_INST(R)                                                                                         \
    template hipError_t launch_beam_word_conf_stream_advance<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &,       \
                                                                const WordLmArgs &, const WordLookArgs *, int, double, int,      \
                                                                void *, hipStream_t);                                             \
    template hipError_t launch_beam_word_conf_stream_confidence<R>(                                                               \
        const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, const WordLookArgs *, int, int, void *, int, \
        int, void *, long long *, long long *, long long *, long long *, long long *, long long *, long long *, long long *,     \
        void *, void *, long long *, long long *, hipStream_t);
ASG_BEAM_WORD_CONF_STREAM_INST(float)
ASG_BEAM_WORD_CONF_STREAM_INST(double)
#undef ASG_BEAM_WORD_CONF_STREAM_INST

}  // namespace asg
