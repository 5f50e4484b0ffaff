// torch_asg_amd/csrc/asg_beam_word_loss.hip -- the BEAM-PRUNED normaliser of an ASG criterion composed with a LEXICON and a WORD
// n-gram LM, on gfx950: asg_beam_loss.hip's log-semiring pass over the PAIRS (LM history h, lexicon product state q) that the
// search of asg_beam_word.hip keeps, plus the pairs every alignment of the target runs through, and its gradients.  The
// specification is include/asg_hip.h::asg_beam_words_full_forward; tests/beam_word_loss_ref.py restates it in numpy.
//
// Forward, four launches on one stream:
//   1  beam_word_loss_search: the frame of asg_beam_word_frame.h in a loop of its own (the same device text as beam_word_kernel,
//      so the same kept sets bit for bit) that leaves |A_t| of every frame beside the [T][K] lists bq / bh; no end, no backtrace;
//   2  beam_word_loss_targets: one thread per utterance walks the lexicon's outgoing rows along the merged target, the LM walk
//      on every separator edge included -> the forced pairs as 64-bit keys h << qbits | q; hdr[0] = n (0: nothing is forced);
//   3  beam_loss_sets<WordSets>: one workgroup per (utterance, frame) -- utterances in x, frames strided over y -- sorts the keys of A_t
//      with those of F_t in LDS (bitonic over the power of two its own count needs), blanks the duplicates and sorts again:
//      U[t][0 .. nu[t]) ascending in pair order;
//   4  beam_word_loss_fwd: one 1024-thread workgroup per utterance walks the frames.  There is no incoming-edge list over pairs
//      (the histories that reach (h', q') through a word cannot be listed without inverting the LM), so alpha PUSHES: U_t lies in
//      LDS, G lanes per pair of U_{t-1} stride over the outgoing row of its q (lane 0 adds the stay, a separator edge walks the
//      LM), find the target in U_t by binary search and -- pass 1 -- raise its maximum with an integer atomicMax on the
//      order-preserving key, -- pass 2 -- add exp(c - max) to its sum as a 64-bit fixed-point integer with 48 fractional bits (a
//      target has at most |U_{t-1}| + 1 < 2^14 candidates of at most 1 each: no overflow).  Integer max and add are associative:
//      the order the lanes arrive in cannot change a bit.  alpha = (max + log(sum)) + emission goes to the workspace ([T][M] when
//      a gradient is wanted, else two rows).  The body of its frame loop is asg_beam_word_alpha.inc, which the catch-up of the
//      lattice-keeping word stream (asg_beam_word_stream_conf.hip) compiles too.
// Backward, two launches: beam_loss_bwd<R, TL, WordLat<R>> (beta PULLS: a pair's own outgoing row is a gather against U_{t+1} in
// LDS, no atomics on values; it owns the label posteriors and the (i, j) counts, summed as 64-bit fixed-point integers, the
// counts in LDS while the [N][N] tile fits, else in the utterance's scratch) and beam_loss_tr_reduce (the utterances in
// ascending order).  NO FLOAT ATOMICS anywhere.  Launch 3, the backward, the end of 4 (Z_K) and the small helpers are the text
// of asg_beam_lattice.h, shared with asg_beam_loss.hip; WordSets / WordLat tell it what a pair key is and how a pair's edges
// are walked (the LM step on a separator edge).  Every output, padding row and
// scratch word that is read is written by these kernels: no memset, so both directions can be captured and replayed.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"  // the frame of the search, the LM walk and the end of a pair
#include "asg_beam_word_lat.h"    // bind_walk and WordLat: how a pair's edges are walked (shared with asg_beam_word_conf.hip)
#include "asg_beam_lattice.h"     // everything behind the search that the token family's loss shares

namespace asg {

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// 1: the search.  beam_word_kernel's frame loop; cnt[t] = |A_t| for t < len.  With LA it is beam_word_la_kernel's frame loop
// (include/asg_hip.h::asg_beam_words_full_forward_la): the frame compiled with the look-ahead flag on, as the two word streams
// compile theirs, so the sets are the look-ahead decoder's.  The values the frame ranks by stay in LDS: launches 2 - 4 and the
// backward read the pairs alone and weigh them plainly.
// ---------------------------------------------------------------------------------------------------------------------
template <typename R, bool TRL, bool LA = false>
__global__ void __launch_bounds__(kBT) beam_word_loss_search(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, int K, R theta,
                                                             int cap, int tbits, char *work, size_t per_utt, size_t cnt_off,
                                                             WordLookParam<LA> la) {
    using U = typename Key<R>::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Ctl<U> &ctl = *(Ctl<U> *) lds;
    WordCtl &wctl = *(WordCtl *) (lds + kWordCtlOff);
    R *cur_v = (R *) (lds + kFixedLds);                    // [K]
    int *cur_q = (int *) (cur_v + K);                      // [K]
    int *cur_h = cur_q + K;                                // [K]
    R *trs = (R *) (cur_h + K);                            // [N][N] if TRL
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = P.N, T = P.T;
    const int len = clamp_len(P.in_len, b, T);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *tr = (const R *) P.transition;
    BeamWordFrame<R, LA> f;
    f.ctl = &ctl; f.wctl = &wctl; f.cur_v = cur_v; f.cur_q = cur_q; f.cur_h = cur_h; f.trs = trs; f.tr = tr;
    f.ts0 = P.ts0; f.ts1 = P.ts1; f.N = N; f.theta = theta;
    bind_graph<R, LA>(f, g, bg, lm, K, cap, tbits);
    bind_look<R>(f, la);
    int *bq, *bh, *bs;
    char *wb = work + (size_t) b * per_utt;
    f.bind_work(wb, T, bq, bh, bs);
    int *cnt = (int *) (wb + cnt_off);
    if (len < 1) return;
    if constexpr (TRL)
        for (int x = tid; x < N * N; x += kBT) trs[x] = tr[(int64_t) (x / N) * P.ts0 + (int64_t) (x % N) * P.ts1];
    if (len >= 2) {
        const size_t C = (size_t) 1 << tbits;
        for (size_t s = tid; s < C; s += kBT) { dev_store(f.tkey + s, 0ull); dev_store(f.val + s, (U) 0); dev_store(f.arg + s, ~0ull); }
    }
    if (tid == 0) { ctl.na = 0; ctl.n = 0; }
    __syncthreads();
    int t = 0;
    for (; t < len; ++t) {
        const int na = ctl.na;
        if (t >= 1 && na == 0) break;                       // an empty beam stays empty
        beam_word_frame<R, TRL, LA>(f, t == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bh, bs, t);
        if (tid == 0) cnt[t] = ctl.na < K ? ctl.na : K;
    }
    for (int u = t + tid; u < len; u += kBT) cnt[u] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// 2: the walk of the merged target through the lexicon and the LM.  -> n pairs into key[0 .. n) (when key is not null) and the
// lexicon + LM score of the target, end terms included; n = 0 and -inf when a label lies outside [0, N), an arc is missing, an
// LM step is rejected, the path ends mid-word or its end is -inf.  One thread.
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__device__ int walk_target(const BeamWordFrame<R> &f, const R *fw, const Problem &P, int b, int tl, int max_n,
                           unsigned long long *key, R &score) {
    const R NINF = Num<R>::ninf();
    score = NINF;
    int n = 0, q = -1, h = f.lstart;
    long long prev = -1;
    R s = (R) 0;
    for (int k = 0; k < tl; ++k) {
        const long long y = P.targets[(int64_t) b * P.gs0 + (int64_t) k * P.gs1];
        if (y == prev) continue;
        if (y < 0 || y >= P.N) return 0;
        int q2 = -1;
        if (q < 0) {
            for (int j = 0; j < f.num_start; ++j)
                if (f.label[f.start_q[j]] == (int) y) { q2 = f.start_q[j]; break; }
            if (q2 < 0) return 0;
            s = f.sw[q2];
        } else {
            int e = f.orow[q];
            const int e1 = f.orow[q + 1];
            for (; e < e1; ++e)
                if (f.oarc[e].y == (int) y) break;
            if (e >= e1) return 0;
            q2 = f.oarc[e].x;
            R w = f.ow[e];
            if ((int) y == f.sep) {
                int h2;
                R a;
                if (!f.step(h, f.wos[f.state[q]], h2, a)) return 0;
                h = h2;
                w = w + a;
            }
            s = s + w;
        }
        if (n >= max_n) return 0;                          // (cannot happen: max_n >= tl)
        if (key) key[n] = f.pair(h, q2);
        ++n;
        q = q2;
        prev = y;
    }
    if (n == 0) return 0;
    R e;
    int w;
    if (!word_end<R>(f, fw, h, q, (R) 0, e, w) || !(e > NINF)) return 0;
    score = s + e;
    return n;
}

template <typename R>
__global__ void __launch_bounds__(64) beam_word_loss_targets(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm,
                                                             BeamWordLossLayout lay, char *work) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= P.B) return;
    char *wb = work + (size_t) b * lay.per;
    int *hdr = (int *) (wb + lay.hdr);
    int n = 0;
    if (P.targets && lay.nf > 0) {
        BeamWordFrame<R> f;
        bind_walk<R>(f, g, bg, lm);
        const int len = clamp_len(P.in_len, b, P.T);
        const int64_t l = P.tg_len ? P.tg_len[b] : P.S;
        const int tl = (int) (l < 0 ? 0 : (l > P.S ? P.S : l));
        R score;
        if (tl >= 1 && tl <= len)                          // (otherwise the target has no alignment)
            n = walk_target<R>(f, (const R *) g.final_w, P, b, tl, lay.nf, (unsigned long long *) (wb + lay.key), score);
    }
    hdr[0] = n;
}

template <typename R>
__global__ void __launch_bounds__(64) beam_word_target_scores(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, R *out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= P.B) return;
    BeamWordFrame<R> f;
    bind_walk<R>(f, g, bg, lm);
    const int64_t l = P.tg_len ? P.tg_len[b] : P.S;
    const int tl = (int) (l < 0 ? 0 : (l > P.S ? P.S : l));
    R score;
    (void) walk_target<R>(f, (const R *) g.final_w, P, b, tl, tl, nullptr, score);
    out[b] = score;
}

// ---------------------------------------------------------------------------------------------------------------------
// 3: beam_loss_sets<WordSets> (asg_beam_lattice.h).  A key is a pair h << qbits | q, below 2^50.
// ---------------------------------------------------------------------------------------------------------------------
struct WordSets {
    using Key = unsigned long long;
    static constexpr Key kFlag = 1ull << 63;
    BeamWordLossLayout lay;
    int K, qbits;
    __device__ Key kept(const char *wb, int t, int x) const {                 // the search's [T][K] lists bh and bq
        const int64_t at = (int64_t) t * K + x;
        return ((Key) (unsigned) ((const int *) (wb + lay.bh))[at] << qbits) | (unsigned) ((const int *) (wb + lay.bq))[at];
    }
    __device__ const Key *forced(const char *wb) const { return (const Key *) (wb + lay.key); }
};

// ---------------------------------------------------------------------------------------------------------------------
// 4: alpha over the U_t, and Z_K.  Dynamic LDS: [reduction slots][ut u64 M][sm u64 M][mk key M].
// ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kBL) beam_word_loss_fwd(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm,
                                                          BeamWordLossLayout lay, int store, char *work, R *scores) {
    using KT = Key<R>;
    using KU = typename KT::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    R *red = (R *) lds;
    const int M = lay.M;
    unsigned long long *ut = (unsigned long long *) (lds + kBLHead);      // [M] U_t
    unsigned long long *sm = ut + M;                                      // [M] sum of exp(c - max), 48 fractional bits
    KU *mk = (KU *) (sm + M);                                             // [M] max candidate as a key, 0: none
    const int tid = threadIdx.x, b = blockIdx.x, T = P.T;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    if (len < 1) { if (tid == 0) scores[b] = NINF; return; }
    char *wb = work + (size_t) b * lay.per;
    const unsigned long long *U = (const unsigned long long *) (wb + lay.U);
    const int *nu = (const int *) (wb + lay.nu);
    R *A = (R *) (wb + lay.A);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *trm = (const R *) P.transition;
    const R *fw = (const R *) g.final_w;
    BeamWordFrame<R> f;
    bind_walk<R>(f, g, bg, lm);
    const unsigned long long qmask = (1ull << f.qbits) - 1ull;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };

    int mp = nu[0];
    for (int x = tid; x < mp; x += kBL) {
        const unsigned long long p = U[x];
        const int q = (int) (p & qmask), h = (int) (p >> f.qbits);
        dev_store(A + x, h == f.lstart ? f.sw[q] + in[(int64_t) f.label[q] * P.is2] : NINF);
    }
    __threadfence();
    __syncthreads();
    for (int t = 1; t < len; ++t) {
        const int mt = nu[t];
        const unsigned long long *Up = U + (int64_t) (t - 1) * M, *Ut = U + (int64_t) t * M;
        const R *Ap = A + (int64_t) (store ? t - 1 : ((t - 1) & 1)) * M;
        R *Arow = A + (int64_t) (store ? t : (t & 1)) * M;
        const R *xt = in + (int64_t) t * P.is0;
#include "asg_beam_word_alpha.inc"   // the frame body, shared with asg_beam_word_stream_conf.hip
    }
    // Z_K over the last lattice set: every kind of end through word_end
    const unsigned long long *Ul = U + (int64_t) (len - 1) * M;
    const R *Al = A + (int64_t) (store ? len - 1 : ((len - 1) & 1)) * M;
    auto end_of = [&](int x) -> R {
        const unsigned long long p = Ul[x];
        R e;
        int w;
        const R a = dev_load(Al + x);
        if (!(a > NINF) || !word_end<R>(f, fw, (int) (p >> f.qbits), (int) (p & qmask), a, e, w)) return NINF;
        return e;
    };
    const R Z = lattice_z<R>(mp, red, end_of);
    if (tid == 0) scores[b] = Z;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward: beam_loss_bwd<R, TL, WordLat<R>> (asg_beam_lattice.h) with the WordLat of asg_beam_word_lat.h.
// ---------------------------------------------------------------------------------------------------------------------

inline size_t wfwd_lds(int elem, int M) { return kBLHead + (size_t) M * (16 + elem); }
}  // namespace

BeamWordLossLayout beam_word_loss_layout(int elem, int T, int K, int cap, int nf, bool store) {
    BeamWordLossLayout l{};
    l.nf = nf;
    l.M = K + nf;
    const BeamWordWorkLayout w = beam_word_work_layout(elem, T, K, cap, word_table_bits(cap));   // the search's own part, in front
    l.bq = w.bq;
    l.bh = w.bh;
    size_t off = w.end;
    l.cnt = off; off += a256((size_t) T * 4);
    l.nu = off;  off += a256((size_t) T * 4);
    l.hdr = off; off += 256;
    l.key = off; off += a256((size_t) nf * 8);
    l.U = off;   off += a256((size_t) T * l.M * 8);
    l.A = off;   off += a256((size_t) (store ? T : 2) * l.M * elem);
    l.per = off;
    return l;
}

size_t beam_word_loss_work_bytes(int elem, int T, int B, int K, int cap, int nf, bool store) {
    return (size_t) B * beam_word_loss_layout(elem, T, K, cap, nf, store).per;
}

// THE bound on M = K + nf: a frame's lattice set with the maximum and the sum of every member (forward), and with its beta
// and the label posteriors (backward), stays in 160 KiB of LDS.
bool beam_word_loss_fits(int elem, int M, int N) {
    return wfwd_lds(elem, M) <= kBLLds && bwd_lds(elem, 8, M, N, false) <= kBLLds;
}

template <typename R>
hipError_t launch_beam_word_loss_forward(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                         const WordLookArgs *LA, int K, double theta, bool store, void *work, void *scores,
                                         hipStream_t stream) {
    const int T = P.T, B = P.B, N = P.N;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const int tbits = word_table_bits(cap);
    const int nf = P.targets ? (P.S < T ? P.S : T) : 0;
    const BeamWordLossLayout lay = beam_word_loss_layout(sizeof(R), T, K, cap, nf, store);
    char *w = (char *) work;
    {
        const size_t beam = kFixedLds + (size_t) K * (sizeof(R) + 8);
        const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
        const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
#define ASG_BEAM_WORD_LOSS_SEARCH(TRL, LAF, LOOK)                                                                             \
    do {                                                                                                                     \
        set_lds((const void *) beam_word_loss_search<R, TRL, LAF>, dyn);                                                    \
        hipLaunchKernelGGL((beam_word_loss_search<R, TRL, LAF>), dim3(B), dim3(kBT), dyn, stream, P, G, BG, LM, K,         \
                           (R) theta, cap, tbits, w, lay.per, lay.cnt, LOOK);                                                \
    } while (0)
        if (LA) { if (trl) ASG_BEAM_WORD_LOSS_SEARCH(true, true, *LA); else ASG_BEAM_WORD_LOSS_SEARCH(false, true, *LA); }
        else if (trl) ASG_BEAM_WORD_LOSS_SEARCH(true, false, WordNoLook{});
        else ASG_BEAM_WORD_LOSS_SEARCH(false, false, WordNoLook{});
#undef ASG_BEAM_WORD_LOSS_SEARCH
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_beam_word_loss_lattice<R>(P, G, BG, LM, lay, K, store, work, scores, stream);
}

// Launches 2 - 4 behind a search that left bq / bh / cnt in the layout `lay` (lay.per: the distance of the utterances, which a
// caller with parts of its own behind the layout may have widened -- asg_beam_word_conf.hip).
template <typename R>
hipError_t launch_beam_word_loss_lattice(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                         const BeamWordLossLayout &lay, int K, bool store, void *work, void *scores,
                                         hipStream_t stream) {
    const int B = P.B;
    char *w = (char *) work;
    hipLaunchKernelGGL((beam_word_loss_targets<R>), dim3((B + 63) / 64), dim3(64), 0, stream, P, G, BG, LM, lay, w);
    int qbits = 1;
    while (((int64_t) 1 << qbits) < G.Q) ++qbits;                                // (bits_of on the host)
    const hipError_t e = launch_beam_loss_sets(P, WordSets{lay, K, qbits}, w, stream);
    if (e != hipSuccess) return e;
    const size_t dyn = wfwd_lds(sizeof(R), lay.M);
    set_lds((const void *) beam_word_loss_fwd<R>, dyn);
    hipLaunchKernelGGL((beam_word_loss_fwd<R>), dim3(B), dim3(kBL), dyn, stream, P, G, BG, LM, lay, (int) store, w, (R *) scores);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_beam_word_loss_backward(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, int K,
                                          const void *work, const void *scores, const void *grad_scores, void *grad_inputs,
                                          void *grad_transition, void *scratch, bool accumulate, hipStream_t stream) {
    const int T = P.T;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const int nf = P.targets ? (P.S < T ? P.S : T) : 0;
    return launch_lattice_backward<R, WordLat<R>>(P, {G, BG, LM, beam_word_loss_layout(sizeof(R), T, K, cap, nf, true)}, work, scores,
                                                  grad_scores, grad_inputs, grad_transition, scratch, accumulate, stream);
}

template <typename R>
hipError_t launch_beam_word_target_scores(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                          void *out, hipStream_t stream) {
    hipLaunchKernelGGL((beam_word_target_scores<R>), dim3((P.B + 63) / 64), dim3(64), 0, stream, P, G, BG, LM, (R *) out);
    return hipGetLastError();
}

#define ASG_WORD_LOSS_INST(R)                                                                                                    \
    template hipError_t launch_beam_word_loss_forward<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &,             \
                                                         const WordLmArgs &, const WordLookArgs *, int, double, bool, void *,   \
                                                         void *, hipStream_t);                                                  \
    template hipError_t launch_beam_word_loss_lattice<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &,             \
                                                         const WordLmArgs &, const BeamWordLossLayout &, int, bool, void *,     \
                                                         void *, hipStream_t);                                                  \
    template hipError_t launch_beam_word_loss_backward<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &,            \
                                                          const WordLmArgs &, int, const void *, const void *, const void *,    \
                                                          void *, void *, void *, bool, hipStream_t);                           \
    template hipError_t launch_beam_word_target_scores<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &,            \
                                                          const WordLmArgs &, void *, hipStream_t);
ASG_WORD_LOSS_INST(float)
ASG_WORD_LOSS_INST(double)
#undef ASG_WORD_LOSS_INST

}  // namespace asg
