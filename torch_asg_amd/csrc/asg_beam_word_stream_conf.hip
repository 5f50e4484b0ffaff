// torch_asg_amd/csrc/asg_beam_word_stream_conf.hip -- the LATTICE-KEEPING word-LM beam stream on gfx950: the streaming search over
// pairs of asg_beam_word_stream.hip with a state that also keeps what the word confidences of asg_beam_word_conf.hip are computed
// from, so that a stream can say how sure it is of a word while the utterance is still arriving.  The specification is
// include/asg_hip.h::asg_beam_word_conf_stream_confidence; tests/beam_word_stream_conf_ref.py restates it in numpy.  DESIGN.md 5ae,
// 5af.
//
// One slot of the state (beam_word_conf_stream_layout; every part 256-byte aligned): the plain word stream's slot unchanged at the
// front -- the search's workspace for T = max_frames, the header, the stored set --; behind it cnt int32 [max_frames] (|A_t|), the
// emissions [max_frames][N], nu int32 [max_frames], U u64 [max_frames][K] (the pair keys h << qbits | q of A_t, ascending), A
// [max_frames][K] (alpha) and two rows of beta.  The header's word 3 is apos: the frames whose U / nu / A rows are valid.
// The search is NOT here.  Reset, advance, result and n-best are the plain word stream's kernels, launched by the plain word
// stream's launchers with this layout's stride: the advance is beam_word_stream_advance_kernel, with or without the look-ahead
// flag, with the KeepLattice policy (asg_beam_stream_lat.h), which besides the plain kernel's work writes cnt[gt] of every frame
// of the chunk -- 0 for the frames an empty beam skips -- and copies the chunk's emissions into rows pos .. pos+n-1.  This unit
// holds the layout and the two kernels of a confidence call:
//   beam_word_stream_conf_catchup         one 1024-thread workgroup per slot, frames [apos, pos) read from the header: U_t = the
//                                         keys of A_t sorted (stream_lat_sets), then the frame body of asg_beam_word_alpha.inc
//                                         (the text beam_word_loss_fwd compiles), which reads row t-1 of U and A from the state as
//                                         the one-shot kernel reads them from its workspace: resuming needs mp = nu[apos-1] and
//                                         nothing else; then apos = pos.  LAZY: it runs in front of a confidence call, every
//                                         frame's alpha is computed once however often confidences are asked for, and what it
//                                         writes depends on nothing but the frames.
//   beam_word_stream_conf_bwd             one workgroup per slot: the hypothesis by beam_word_stream_hyp (the function
//                                         beam_word_stream_result_kernel is), word_frames by word_end_frames (the walk of
//                                         beam_word_conf_search), Z by lattice_z over the last set, and the tail of
//                                         beam_word_conf_bwd by beam_word_conf_words (asg_beam_word_conf_pull.h) over the stored
//                                         emissions.  The one new thing is the end of a PREFIX (weight 0, no event at frame len),
//                                         which the pull takes as its lattice type (PrefixWordLat).
// The lattice pass weighs the pairs plainly, as asg_beam_word_conf.hip does behind a look-ahead search: only the advance and the
// winner of the bwd read the look-ahead.  A confidence call is two launches (catch-up, bwd): no host synchronisation, no memset,
// no copy.  No float atomics: integer maxima and fixed-point sums, the same adds in the same order as asg_beam_words_confidence.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"
#include "asg_beam_lattice.h"
#include "asg_beam_stream_lat.h"
#include "asg_beam_word_lat.h"
#include "asg_beam_word_conf_pull.h"
#include "asg_beam_conf_sink.h"

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
    const int L = stream_pos(hdr, max_frames);
    int a0 = stream_apos(hdr, L);
    if (a0 >= L) return;                                 // caught up (apos <= pos always: nothing to store)
    const int *bq = (const int *) (wb + lay.lat.bq), *bh = (const int *) (wb + lay.lat.bh);   // the search's [max_frames][K] pairs
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

    stream_lat_sets<unsigned long long>(a0, L, K, (const int *) (wb + lay.lat.cnt), v, ~0ull, U, nu, [&](int t, int x) {
        const int64_t at = (int64_t) t * K + x;
        return f.pair(bh[at], bq[at]);
    });

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
    long long *wf = wframes + (int64_t) b * T;
    const bool fin = args.fin != 0;
    const R *fw = (const R *) args.g.final_w;

    BeamWordFrame<R, LA> f;
    int len;
    const U bkey = beam_word_stream_hyp<R, LA>(f, wctl, args.g, args.lm, la, K, cap, tbits, T, wb, lay.st, fin, scores, path, tokens,
                                               tlen, states, lm_states, words, wlen, frames, status, len);
    if (bkey == 0) {
        for (int u = tid; u < T; u += kBL) wf[u] = -1;
    } else {
        word_end_frames(path + (int64_t) b * T, f.sep, len, T, wlen + b, wf);
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
    beam_word_conf_words<R, PrefixWordLat<R>>(P, args, wb, lay.beta, Z, len, nw, T, tol, words + (int64_t) b * T, wf,
                                              conf + (int64_t) b * T, ring, nq, nb);
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
    template hipError_t launch_beam_word_conf_stream_confidence<R>(                                                               \
        const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, const WordLookArgs *, int, int, void *, int, \
        int, void *, long long *, long long *, long long *, long long *, long long *, long long *, long long *, long long *,     \
        void *, void *, long long *, long long *, hipStream_t);
ASG_BEAM_WORD_CONF_STREAM_INST(float)
ASG_BEAM_WORD_CONF_STREAM_INST(double)
#undef ASG_BEAM_WORD_CONF_STREAM_INST

}  // namespace asg
