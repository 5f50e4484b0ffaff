// torch_asg_amd/csrc/asg_beam_word_stream.hip -- STREAMING beam decoding with a lexicon and a word n-gram LM composed on the fly,
// on gfx950: the search of asg_beam_word.hip over pairs (LM history h, lexicon product state q) carried across chunks of frames.
// The specification is include/asg_hip.h::asg_beam_word_stream_advance; tests/beam_word_stream_ref.py restates it.  Decoding an
// utterance in chunks gives the bits of decoding it in one call, for any chunking: the frames and the end run the device code of
// the one-shot decoder (asg_beam_word_frame.h, compiled into both translation units), and the search never looks ahead -- the LM
// walk of a separator edge reads the source pair's h and nothing else, whether that pair was kept a frame or a call ago.
//
// A stream state serves B utterance slots.  One slot (beam_word_stream_layout; every part 256-byte aligned):
//   the one-shot decoder's workspace of one utterance with T = max_frames (asg_beam_common.h, beam_word_work_layout): bq / bh / bs
//     int32 [max_frames][K] (product state, LM state and source slot of every kept pair of every frame consumed so far), the table
//     tkey u64 [C], arg u64 [C], val key [C], ckey key [cap], cpair u64 [cap], touched int32 [cap];
//   a 256-byte header: int32 pos (frames consumed), |A| (size of the stored set), overflow, and a word a plain state never reads
//     (asg_beam_stream_lat.h);
//   the stored set: values [K] (dtype), then product states int32 [K], then LM states int32 [K].
// A LATTICE-KEEPING state (asg_beam_word_stream_conf.hip) has this slot at its front and more behind it.  Its search is this
// unit's: the launchers take the slot's stride, and the advance kernel is a template over a keep policy (asg_beam_stream_lat.h,
// DESIGN.md 5af) -- KeepNone, empty, for the plain state; KeepLattice, which also writes |A_t| of every frame and the chunk's
// emissions.
// Nothing is sized by H, V, A or Q.  Three kernels, each one launch, no host synchronisation, no copy, no memset:
//   beam_word_stream_reset_kernel    per chosen slot: the header zeroed, and the whole table emptied (tkey = 0, val = 0,
//                                    arg = none).  The only place all C slots are written: a frame empties what it touched, so
//                                    the table is empty between calls.
//   beam_word_stream_advance_kernel  one 1024-thread workgroup per slot: the transitions and the stored set into LDS,
//                                    beam_word_frame for the chunk's frames with the back-pointers into rows pos .. pos+n-1, the
//                                    set and pos back.
//   beam_word_stream_result_kernel   one workgroup per slot: beam_word_stream_hyp (asg_beam_stream_lat.h) -- the best end over the
//                                    stored set (the end of the one-shot decoder, or the best prefix), the backtrace over pos
//                                    frames, the words, the token collapse, the padding.  It only reads the state.
// What one call writes and the next reads crosses a kernel boundary, so plain stores and loads do; the table keeps the
// device-scope loads and atomics of the frame body.  Integer atomics only: bit-identical run to run.
//
// With LM look-ahead (include/asg_hip.h::asg_beam_word_stream_advance_la) the advance and result kernels are compiled a second
// time with the frame's look-ahead flag on, as asg_beam_word_la.hip compiles the one-shot kernel: the stored values then carry
// L(h, state(q)), the end takes it back as the one-shot's does and the best prefix by word_prefix.  `look` reads static arrays
// and the pair's own (h, q), so the argument above holds as it stands; the state has the same bytes.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_frame.h"
#include "asg_beam_stream_lat.h"

namespace asg {

namespace {

__global__ void __launch_bounds__(256) beam_word_stream_reset_kernel(char *state, BeamStreamLayout lay, BeamWordWorkLayout wl,
                                                                      unsigned C, int key_bytes, const unsigned char *mask) {
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;
    char *wb = state + (size_t) b * lay.per;
    beam_word_reset_tables(wb, wl, C, key_bytes);
    if (blockIdx.y == 0 && threadIdx.x < kHdrWords) ((int *) (wb + lay.hdr))[threadIdx.x] = 0;      // pos, |A|, overflow, apos
}

template <typename R, bool TRL, bool LA, typename Keep>
__global__ void __launch_bounds__(kBT) beam_word_stream_advance_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, WordLmArgs lm, int K,
                                                                       R theta, int cap, int tbits, int max_frames, char *state,
                                                                       BeamStreamLayout lay, WordLookParam<LA> la, Keep keep) {
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
    int *hdr = (int *) (wb + lay.hdr);
    R *set_v = (R *) (wb + lay.set);                        // values [K], then product states [K], then LM states [K]
    const int pos = stream_pos(hdr, max_frames);
    const int want = clamp_len(P.in_len, b, P.T);
    const int n = want < max_frames - pos ? want : max_frames - pos;
    if (n < want && tid == 0) hdr[2] = 1;                   // frames beyond max_frames are not consumed
    if (n < 1) return;
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    keep.chunk(wb, in, P, pos, n);
    const R *tr = (const R *) P.transition;
    BeamWordFrame<R, LA> f;
    f.ctl = &ctl; f.wctl = &wctl; f.cur_v = cur_v; f.cur_q = cur_q; f.cur_h = cur_h; f.trs = trs; f.tr = tr;
    f.ts0 = P.ts0; f.ts1 = P.ts1; f.N = N; f.theta = theta;
    bind_graph<R>(f, g, bg, lm, K, cap, tbits);
    bind_look<R>(f, la);
    int *bq, *bh, *bs;
    f.bind_work(wb, max_frames, bq, bh, bs);

    beam_word_load_set<R, TRL, LA>(f, trs, set_v, stream_na(hdr, pos, K));

    int t = 0;
    for (; t < n; ++t) {
        const int gt = pos + t;                             // the frame's index in the utterance
        const int na = ctl.na;
        if (gt >= 1 && na == 0) break;                      // an empty beam stays empty (pos still advances)
        beam_word_frame<R, TRL, LA>(f, gt == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bh, bs, gt);
        keep.frame(wb, gt, ctl.na < K ? ctl.na : K);
    }
    keep.skipped(wb, pos, t, n);

    const int na = beam_word_store_set<R, LA>(f, set_v);
    if (tid == 0) { hdr[1] = na; hdr[0] = pos + n; }
}

template <typename R, bool LA = false>
__global__ void __launch_bounds__(kBT) beam_word_stream_result_kernel(GraphArgs g, WordLmArgs lm, int K, int cap, int tbits,
                                                                      int max_frames, const char *state, BeamStreamLayout lay,
                                                                      int final, R *scores, long long *path, long long *tokens,
                                                                      long long *tlen, long long *states, long long *lm_states,
                                                                      long long *words, long long *wlen, long long *frames,
                                                                      long long *status, WordLookParam<LA> la) {
    __shared__ WordCtl wctl;
    char *wb = const_cast<char *>(state) + (size_t) blockIdx.x * lay.per;   // (only read: bind_work takes the workspace as it is)
    BeamWordFrame<R, LA> f;
    int len;
    beam_word_stream_hyp<R, LA>(f, wctl, g, lm, la, K, cap, tbits, max_frames, wb, lay, final != 0, scores, path, tokens, tlen,
                                states, lm_states, words, wlen, frames, status, len);
}

}  // namespace

BeamStreamLayout beam_word_stream_layout(int elem, int max_frames, int K, int cap) {
    BeamStreamLayout l{};
    size_t off = beam_word_work_layout(elem, max_frames, K, cap, word_table_bits(cap)).end;   // the one-shot decoder's part
    l.hdr = off;  off += 256;
    l.set = off;  off += a256((size_t) K * (elem + 8));
    l.per = off;
    return l;
}

size_t beam_word_stream_state_bytes(int elem, int max_frames, int B, int K, int cap) {
    return (size_t) B * beam_word_stream_layout(elem, max_frames, K, cap).per;
}

hipError_t launch_beam_word_stream_reset(int elem, const BeamGraphArgs &BG, int K, int max_frames, int B, void *state,
                                         const unsigned char *mask, hipStream_t stream, size_t stride) {
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    BeamStreamLayout lay = beam_word_stream_layout(elem, max_frames, K, cap);
    if (stride) lay.per = stride;                                           // (a slot with parts of the caller's behind it)
    const int tbits = word_table_bits(cap);
    const size_t C = (size_t) 1 << tbits;
    hipLaunchKernelGGL(beam_word_stream_reset_kernel, dim3(B, reset_blocks(C)), dim3(256), 0, stream, (char *) state, lay,
                       beam_word_work_layout(elem, max_frames, K, cap, tbits), (unsigned) C, elem, mask);
    return hipGetLastError();
}

namespace {

template <typename R, typename Keep>
hipError_t beam_word_stream_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                    const WordLookArgs *LA, int K, double theta, int cap, int max_frames, void *state,
                                    const BeamStreamLayout &lay, Keep keep, hipStream_t stream) {
    const int N = P.N;
    const int tbits = word_table_bits(cap);
    // the LDS of the one-shot decoder: control block, the set, and the transitions when they fit beside it
    const size_t beam = kFixedLds + (size_t) K * (sizeof(R) + 8);
    const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
    const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
#define ASG_BEAM_WORD_STREAM(TRL, LAF, LOOK)                                                                                 \
    do {                                                                                                                     \
        const void *fn = (const void *) beam_word_stream_advance_kernel<R, TRL, LAF, Keep>;                                 \
        if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);       \
        hipLaunchKernelGGL((beam_word_stream_advance_kernel<R, TRL, LAF, Keep>), dim3(P.B), dim3(kBT), dyn, stream, P, G,  \
                           BG, LM, K, (R) theta, cap, tbits, max_frames, (char *) state, lay, LOOK, keep);                   \
    } while (0)
    if (LA) { if (trl) ASG_BEAM_WORD_STREAM(true, true, *LA); else ASG_BEAM_WORD_STREAM(false, true, *LA); }
    else if (trl) ASG_BEAM_WORD_STREAM(true, false, WordNoLook{}); else ASG_BEAM_WORD_STREAM(false, false, WordNoLook{});
#undef ASG_BEAM_WORD_STREAM
    return hipGetLastError();
}

}  // namespace

template <typename R>
hipError_t launch_beam_word_stream_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                           const WordLookArgs *LA, int K, double theta, int max_frames, void *state,
                                           hipStream_t stream, bool lattice) {
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    if (lattice) {
        const BeamWordConfStreamLayout lay = beam_word_conf_stream_layout(sizeof(R), max_frames, K, cap, P.N);
        return beam_word_stream_advance<R>(P, G, BG, LM, LA, K, theta, cap, max_frames, state, lay.st,
                                           KeepLattice{lay.lat.cnt, lay.em}, stream);
    }
    return beam_word_stream_advance<R>(P, G, BG, LM, LA, K, theta, cap, max_frames, state,
                                       beam_word_stream_layout(sizeof(R), max_frames, K, cap), KeepNone{}, stream);
}
template hipError_t launch_beam_word_stream_advance<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &,
                                                           const WordLmArgs &, const WordLookArgs *, int, double, int, void *,
                                                           hipStream_t, bool);
template hipError_t launch_beam_word_stream_advance<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &,
                                                            const WordLmArgs &, const WordLookArgs *, int, double, int, void *,
                                                            hipStream_t, bool);

template <typename R>
hipError_t launch_beam_word_stream_result(const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                          const WordLookArgs *LA, int K, int max_frames, int B, const void *state, int final,
                                          void *scores, long long *path, long long *tokens,
                                          long long *tlen, long long *states, long long *lm_states, long long *words,
                                          long long *wlen, long long *frames, long long *status, hipStream_t stream,
                                          size_t stride) {
    const int cap = beam_word_cap(K, BG.max_out, BG.num_start);
    BeamStreamLayout lay = beam_word_stream_layout(sizeof(R), max_frames, K, cap);
    if (stride) lay.per = stride;                                           // (a slot with parts of the caller's behind it)
#define ASG_BEAM_WORD_STREAM_RESULT(LAF, LOOK)                                                                               \
    hipLaunchKernelGGL((beam_word_stream_result_kernel<R, LAF>), dim3(B), dim3(kBT), 0, stream, G, LM, K, cap,               \
                       word_table_bits(cap), max_frames, (const char *) state, lay, final, (R *) scores, path, tokens, tlen, \
                       states, lm_states, words, wlen, frames, status, LOOK)
    if (LA) ASG_BEAM_WORD_STREAM_RESULT(true, *LA); else ASG_BEAM_WORD_STREAM_RESULT(false, WordNoLook{});
#undef ASG_BEAM_WORD_STREAM_RESULT
    return hipGetLastError();
}
template hipError_t launch_beam_word_stream_result<float>(const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                                          const WordLookArgs *, int, int, int, const void *, int, void *, long long *, long long *, long long *,
                                                          long long *, long long *, long long *, long long *, long long *,
                                                          long long *, hipStream_t, size_t);
template hipError_t launch_beam_word_stream_result<double>(const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                                           const WordLookArgs *, int, int, int, const void *, int, void *, long long *, long long *, long long *,
                                                           long long *, long long *, long long *, long long *, long long *,
                                                           long long *, hipStream_t, size_t);

}  // namespace asg
