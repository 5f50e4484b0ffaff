// torch_asg_amd/csrc/asg_beam_word.hip -- beam decoding over the ASG lattice composed with a LEXICON and a WORD n-gram LM, the
// LM composed on the fly, on gfx950 (include/asg_hip.h::asg_beam_decode_words).  The search of asg_beam_graph.hip with the search
// state widened from a product state q of the lexicon automaton to a PAIR (h, q), h a history state of the word LM: a separator
// edge out of a word-end node walks the LM (binary search of the row, backoff loop) and moves h; every other edge keeps it.
// Pairs exist only while the search holds them, so nothing is sized by H, V, A or Q: the slot arrays val[Q] / arg[Q] of
// asg_beam_graph.hip become an open-addressed hash table in the utterance's workspace.
//
// ONE launch, one 1024-thread workgroup per utterance walks the frames; the kept set (h, q, value) lives in LDS.  Per frame:
//   expand A   G lanes per kept pair stride over the outgoing row of its q (lane 0 adds the stay).  The target pair, as the key
//              (h << qbits | q) + 1, is looked up in the table (capacity C, a power of two >= 2 * cap; multiplicative hash, linear
//              probing, at most C probes) and inserted into the first empty slot with a 64-bit atomicCAS; the lane whose CAS
//              inserted it appends the SLOT to the touched list.  The candidate's value goes into val[slot] with an integer
//              atomicMax on its order-preserving key (0 = empty).
//   expand B   the same candidates again (the LM walk included): those whose key equals val[slot] put (source pair << 14 | source
//              slot) into arg[slot] with a 64-bit atomicMin -- the smallest source pair among the tied.
//   select     as in asg_beam_frame.h: c = value + emission as a key beside the list, with the pair beside it; lo = fl(max -
//              threshold); a radix select finds the K-th key when more than K pass, and a second one over the pair's hbits + qbits
//              bits finds the largest pair taken among the keys tied with it.  The last walk appends the chosen to the new set,
//              stores (q, h, source slot) of the frame and empties key, val and arg of every touched slot.
// Which slot a pair lands in depends on the hash and on timing; no result does: max and min are order independent, a pair owns
// exactly one slot for the length of a frame (nothing is deleted inside one), and the order of the kept set is never looked at.
// The table is written by atomics (at L2) and read back with device-scope loads; everything else crosses __syncthreads.
// Frame 0 takes the start states with h = start (their q are distinct: no table).  Then the best end -- at the root + ew[h], in
// a word-end node one more LM walk -- the backtrace, the token collapse and the words, in the same launch.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"  // the frame and the end: the streaming decoder (asg_beam_word_stream.hip) compiles the same text

namespace asg {

namespace {

// FIN: the instantiation behind the n-best stage (asg_beam_word_nbest.hip), which also leaves the last set in memory at fin_off;
// the decoder's own (FIN false) is the code object it was before that stage existed.
template <typename R, bool TRL, bool FIN>
__global__ void __launch_bounds__(kBT) beam_word_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, int K, R theta,
                                                        int cap, int tbits, char *work, size_t per_utt, R *scores,
                                                        long long *path, long long *tokens, long long *tlen, long long *states,
                                                        long long *lm_states, long long *words, long long *wlen,
                                                        size_t fin_off) {
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
    const int N = P.N, T = P.T;
    const R NINF = Num<R>::ninf();
    const int len = clamp_len(P.in_len, b, T);
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *tr = (const R *) P.transition;
    const R *fw = (const R *) g.final_w;
    long long *pb = path + (int64_t) b * T, *tk = tokens + (int64_t) b * T, *st = states + (int64_t) b * T;
    long long *ls = lm_states + (int64_t) b * T, *wd = words + (int64_t) b * T;
    BeamWordFrame<R> f;
    f.ctl = &ctl; f.wctl = &wctl; f.cur_v = cur_v; f.cur_q = cur_q; f.cur_h = cur_h; f.trs = trs; f.tr = tr;
    f.ts0 = P.ts0; f.ts1 = P.ts1;
    f.N = N; f.K = K; f.G = beam_lanes_per_state(K); f.cap = cap; f.sep = lm.sep; f.theta = theta;
    f.qbits = bits_of(g.Q); f.pbits = f.qbits + bits_of(lm.H);
    f.label = g.label; f.state = g.state; f.orow = bg.orow; f.start_q = bg.start_q; f.num_start = bg.num_start;
    f.oarc = (const int2 *) bg.oarc; f.ow = (const R *) bg.ow; f.sw = (const R *) g.start_w;
    f.lrow = lm.row; f.lword = lm.word; f.lnext = lm.next; f.lback = lm.backoff; f.wos = lm.word_of_state;
    f.lw = (const R *) lm.lw; f.bw = (const R *) lm.bw; f.ew = (const R *) lm.ew; f.lstart = lm.start;
    f.tbits = tbits;
    int *bq, *bh, *bs;
    f.bind_work(work + (size_t) b * per_utt, T, bq, bh, bs);

    if (len < 1) {
        word_no_path(T, pb, tk, st, ls, wd, tlen + b, wlen + b);
        if (tid == 0) scores[b] = NINF;
        return;
    }
    if constexpr (TRL)
        for (int x = tid; x < N * N; x += kBT) trs[x] = tr[(int64_t) (x / N) * P.ts0 + (int64_t) (x % N) * P.ts1];
    if (len >= 2) {
        const size_t C = (size_t) 1 << tbits;
        for (size_t s = tid; s < C; s += kBT) { dev_store(f.tkey + s, 0ull); dev_store(f.val + s, (U) 0); dev_store(f.arg + s, ~0ull); }
    }
    if (tid == 0) { ctl.na = 0; ctl.n = 0; }
    __syncthreads();

    for (int t = 0; t < len; ++t) {
        const int na = ctl.na;
        if (t >= 1 && na == 0) break;                       // an empty beam stays empty
        beam_word_frame<R, TRL>(f, t == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bh, bs, t);
    }

    // ---- the best end over the last kept set, the smallest pair on a tie; the backtrace, the words, the tokens
    const int na = ctl.na < K ? ctl.na : K;
    if constexpr (FIN) {                                    // the n-best stage reads the last set from memory
        char *fin = work + (size_t) b * per_utt + fin_off;
        R *fv = (R *) (fin + 8);
        int *fq = (int *) (fv + K), *fh = fq + K;
        for (int k = tid; k < na; k += kBT) { fv[k] = cur_v[k]; fq[k] = cur_q[k]; fh[k] = cur_h[k]; }
        if (tid == 0) *(int *) fin = na;
    }
    U bkey;
    int bk;
    word_best_end<R>(f, fw, true, cur_h, cur_q, cur_v, na, bkey, bk);
    if (bkey == 0) {                                        // an empty beam, or no kept pair with a finite end
        word_no_path(T, pb, tk, st, ls, wd, tlen + b, wlen + b);
        if (tid == 0) scores[b] = NINF;
        return;
    }
    word_backtrace<R>(f, fw, true, cur_h, cur_q, cur_v, bk, bq, bh, bs, len, T, scores + b, pb, tk, st, ls, wd, tlen + b,
                      wlen + b);
}

}  // namespace

// The touched list holds the target pairs of one frame: at most K * (largest out-degree + 1), at least the start states.  (No
// clamp to Q: pairs are not bounded by it.)
int beam_word_cap(int K, int max_out, int num_start) {
    int64_t c = (int64_t) K * ((int64_t) max_out + 1);
    if (c < num_start) c = num_start;
    return (int) (c < 1 ? 1 : c);
}

size_t beam_word_work_bytes(int elem, int T, int B, int K, int cap) {
    return (size_t) B * beam_word_work_layout(elem, T, K, cap, word_table_bits(cap)).end;
}

template <typename R>
hipError_t launch_beam_words(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, int K,
                             double theta, void *work, void *scores, long long *path, long long *tokens, long long *tlen,
                             long long *states, long long *lm_states, long long *words, long long *wlen, hipStream_t stream,
                             size_t stride, size_t fin_off) {
    const int N = P.N;
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    const int tbits = word_table_bits(cap);
    const size_t per = stride ? stride : beam_word_work_layout(sizeof(R), P.T, K, cap, tbits).end;
    const size_t beam = kFixedLds + (size_t) K * (sizeof(R) + 8);
    const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
    const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
#define ASG_BEAM_WORD(TRL, FIN)                                                                                            \
    do {                                                                                                                   \
        const void *fn = (const void *) beam_word_kernel<R, TRL, FIN>;                                                    \
        if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);     \
        hipLaunchKernelGGL((beam_word_kernel<R, TRL, FIN>), dim3(P.B), dim3(kBT), dyn, stream, P, G, BG, LM, K, (R) theta, \
                           cap, tbits, (char *) work, per, (R *) scores, path, tokens, tlen, states, lm_states, words,     \
                           wlen, fin_off);                                                                                 \
    } while (0)
    if (fin_off) { if (trl) ASG_BEAM_WORD(true, true); else ASG_BEAM_WORD(false, true); }
    else if (trl) ASG_BEAM_WORD(true, false); else ASG_BEAM_WORD(false, false);
#undef ASG_BEAM_WORD
    return hipGetLastError();
}
template hipError_t launch_beam_words<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, int,
                                             double, void *, void *, long long *, long long *, long long *, long long *,
                                             long long *, long long *, long long *, hipStream_t, size_t, size_t);
template hipError_t launch_beam_words<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &, int,
                                              double, void *, void *, long long *, long long *, long long *, long long *,
                                              long long *, long long *, long long *, hipStream_t, size_t, size_t);

}  // namespace asg

