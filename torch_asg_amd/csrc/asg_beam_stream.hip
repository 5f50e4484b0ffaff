// torch_asg_amd/csrc/asg_beam_stream.hip -- STREAMING beam decoding on gfx950: the search of asg_beam_graph.hip carried across
// chunks of frames, so that a transcript exists while the utterance is still arriving.  The specification is
// include/asg_hip.h::asg_beam_stream_advance; tests/beam_stream_ref.py restates it.  Decoding an utterance in chunks gives the
// bits of decoding it in one call, for any chunking: the frames run the device code of the one-shot decoder (asg_beam_frame.h,
// compiled into both translation units), and the search never looks ahead.
//
// A stream state serves B utterance slots.  One slot (beam_stream_layout; every part 256-byte aligned):
//   the one-shot decoder's workspace of one utterance with T = max_frames (asg_beam_common.h, beam_work_layout): bq / bs int32
//     [max_frames][K] (product state and source slot of every kept state of every frame consumed so far), arg u64 [Q], val key
//     [Q], ckey key [cap], touched int32 [cap];
//   a 256-byte header: int32 pos (frames consumed), |A| (size of the stored set), overflow, and a word a plain state never reads
//     (asg_beam_stream_lat.h);
//   the stored set: values [K] (dtype), then product states int32 [K].
// A LATTICE-KEEPING state (asg_beam_stream_conf.hip) has this slot at its front and more behind it.  Its search is this unit's: the
// launchers take the slot's stride, and the advance kernel is a template over a keep policy (asg_beam_stream_lat.h)
// -- KeepNone, empty, for the plain state; KeepLattice, which also writes |A_t| of every frame and the chunk's emissions.
// Three kernels, each one launch, no host synchronisation, no copy, no memset:
//   beam_stream_reset_kernel    per chosen slot: the header zeroed, val = 0 and arg = none for all Q states.  The only
//                               place the Q entries are written: a frame empties what it touched, so they are empty between calls.
//   beam_stream_advance_kernel  one 1024-thread workgroup per slot: the transitions and the stored set into LDS, beam_frame for
//                               the chunk's frames with the back-pointers into rows pos .. pos+n-1, the set and pos back.
//   beam_stream_result_kernel   one workgroup per slot: beam_stream_hyp (asg_beam_stream_lat.h) -- the best end over the stored set
//                               (with or without the final weights), the backtrace over pos frames, the token collapse, the
//                               padding.  It only reads the state.
// What one call writes and the next reads crosses a kernel boundary, so plain stores and loads do; val / arg keep the
// device-scope atomics of the frame body.  Integer atomics only: bit-identical run to run.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_frame.h"
#include "asg_beam_stream_lat.h"

namespace asg {

namespace {

__global__ void __launch_bounds__(256) beam_stream_reset_kernel(char *state, BeamStreamLayout lay, BeamWorkLayout wl, int Q,
                                                                 int key_bytes, const unsigned char *mask) {
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;
    char *wb = state + (size_t) b * lay.per;
    beam_reset_tables(wb, wl, Q, key_bytes);
    if (blockIdx.y == 0 && threadIdx.x < kHdrWords) ((int *) (wb + lay.hdr))[threadIdx.x] = 0;      // pos, |A|, overflow, apos
}

template <typename R, bool TRL, typename Keep>
__global__ void __launch_bounds__(kBT) beam_stream_advance_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, int K, R theta, int cap,
                                                                  int max_frames, char *state, BeamStreamLayout lay, Keep keep) {
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
    int *hdr = (int *) (wb + lay.hdr);
    R *set_v = (R *) (wb + lay.set);                        // values [K], then product states [K]
    const int pos = stream_pos(hdr, max_frames);
    const int want = clamp_len(P.in_len, b, P.T);
    const int n = want < max_frames - pos ? want : max_frames - pos;
    if (n < want && tid == 0) hdr[2] = 1;                   // frames beyond max_frames are not consumed
    if (n < 1) return;
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    keep.chunk(wb, in, P, pos, n);
    const R *tr = (const R *) P.transition;
    BeamFrame<R> f;
    f.ctl = &ctl; f.cur_v = cur_v; f.cur_q = cur_q; f.trs = trs; f.tr = tr; f.ts0 = P.ts0; f.ts1 = P.ts1;
    f.N = N; f.Q = g.Q; f.K = K; f.G = beam_lanes_per_state(K); f.theta = theta;
    f.label = g.label; f.orow = bg.orow; f.start_q = bg.start_q; f.num_start = bg.num_start;
    f.oarc = (const int2 *) bg.oarc; f.ow = (const R *) bg.ow; f.sw = (const R *) g.start_w;
    int *bq, *bs;
    f.bind_work(wb, max_frames, cap, bq, bs);

    beam_load_set<R, TRL>(f, trs, set_v, stream_na(hdr, pos, K));

    int t = 0;
    for (; t < n; ++t) {
        const int gt = pos + t;                             // the frame's index in the utterance
        const int na = ctl.na;
        if (gt >= 1 && na == 0) break;                      // an empty beam stays empty
        beam_frame<R, TRL>(f, gt == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bs, gt);
        keep.frame(wb, gt, ctl.na < K ? ctl.na : K);
    }
    keep.skipped(wb, pos, t, n);

    const int na = beam_store_set<R>(f, set_v);
    if (tid == 0) { hdr[1] = na; hdr[0] = pos + n; }
}

template <typename R>
__global__ void __launch_bounds__(kBT) beam_stream_result_kernel(GraphArgs g, int K, int cap, int max_frames,
                                                                 const char *state, BeamStreamLayout lay, int final, R *scores,
                                                                 long long *path, long long *tokens, long long *tlen,
                                                                 long long *states, long long *frames, long long *status) {
    __shared__ Ctl<typename Key<R>::U> ctl;
    int len;
    beam_stream_hyp<R>(ctl, g, K, cap, max_frames, state + (size_t) blockIdx.x * lay.per, lay, final, scores, path, tokens, tlen,
                       states, frames, status, len);
}

}  // namespace

BeamStreamLayout beam_stream_layout(int elem, int max_frames, int Q, int K, int cap) {
    BeamStreamLayout l{};
    size_t off = beam_work_layout(elem, max_frames, Q, K, cap).end;       // the one-shot decoder's part, at the front
    l.hdr = off;  off += 256;
    l.set = off;  off += a256((size_t) K * (elem + 4));
    l.per = off;
    return l;
}

size_t beam_stream_state_bytes(int elem, int max_frames, int B, int Q, int K, int cap) {
    return (size_t) B * beam_stream_layout(elem, max_frames, Q, K, cap).per;
}

hipError_t launch_beam_stream_reset(int elem, const GraphArgs &G, const BeamGraphArgs &BG, int K, int max_frames, int B, void *state,
                                    const unsigned char *mask, hipStream_t stream, size_t stride) {
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    BeamStreamLayout lay = beam_stream_layout(elem, max_frames, G.Q, K, cap);
    if (stride) lay.per = stride;                                           // (a slot with parts of the caller's behind it)
    hipLaunchKernelGGL(beam_stream_reset_kernel, dim3(B, reset_blocks(G.Q)), dim3(256), 0, stream, (char *) state, lay,
                       beam_work_layout(elem, max_frames, G.Q, K, cap), G.Q, elem, mask);
    return hipGetLastError();
}

namespace {

template <typename R, typename Keep>
hipError_t beam_stream_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta, int cap,
                               int max_frames, void *state, const BeamStreamLayout &lay, Keep keep, hipStream_t stream) {
    const int N = P.N;
    // the LDS of the one-shot decoder: control block, the set, and the transitions when they fit beside it
    const size_t beam = kFixedLds + (size_t) K * (sizeof(R) + 4) + 8;
    const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
    const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
#define ASG_BEAM_STREAM(TRL)                                                                                               \
    do {                                                                                                                   \
        const void *fn = (const void *) beam_stream_advance_kernel<R, TRL, Keep>;                                         \
        if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);     \
        hipLaunchKernelGGL((beam_stream_advance_kernel<R, TRL, Keep>), dim3(P.B), dim3(kBT), dyn, stream, P, G, BG, K,   \
                           (R) theta, cap, max_frames, (char *) state, lay, keep);                                         \
    } while (0)
    if (trl) ASG_BEAM_STREAM(true); else ASG_BEAM_STREAM(false);
#undef ASG_BEAM_STREAM
    return hipGetLastError();
}

}  // namespace

template <typename R>
hipError_t launch_beam_stream_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta,
                                      int max_frames, void *state, hipStream_t stream, bool lattice) {
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    if (lattice) {
        const BeamConfStreamLayout lay = beam_conf_stream_layout(sizeof(R), max_frames, G.Q, K, cap, P.N);
        return beam_stream_advance<R>(P, G, BG, K, theta, cap, max_frames, state, lay.st, KeepLattice{lay.lat.cnt, lay.em}, stream);
    }
    return beam_stream_advance<R>(P, G, BG, K, theta, cap, max_frames, state, beam_stream_layout(sizeof(R), max_frames, G.Q, K, cap),
                                  KeepNone{}, stream);
}
template hipError_t launch_beam_stream_advance<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, double, int,
                                                      void *, hipStream_t, bool);
template hipError_t launch_beam_stream_advance<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, double, int,
                                                       void *, hipStream_t, bool);

template <typename R>
hipError_t launch_beam_stream_result(const GraphArgs &G, const BeamGraphArgs &BG, int K, int max_frames, int B, const void *state,
                                     int final, void *scores, long long *path, long long *tokens, long long *tlen,
                                     long long *states, long long *frames, long long *status, hipStream_t stream, size_t stride) {
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    BeamStreamLayout lay = beam_stream_layout(sizeof(R), max_frames, G.Q, K, cap);
    if (stride) lay.per = stride;                                           // (a slot with parts of the caller's behind it)
    hipLaunchKernelGGL((beam_stream_result_kernel<R>), dim3(B), dim3(kBT), 0, stream, G, K, cap, max_frames, (const char *) state,
                       lay, final, (R *) scores, path, tokens, tlen, states, frames, status);
    return hipGetLastError();
}
template hipError_t launch_beam_stream_result<float>(const GraphArgs &, const BeamGraphArgs &, int, int, int, const void *, int,
                                                     void *, long long *, long long *, long long *, long long *, long long *,
                                                     long long *, hipStream_t, size_t);
template hipError_t launch_beam_stream_result<double>(const GraphArgs &, const BeamGraphArgs &, int, int, int, const void *, int,
                                                      void *, long long *, long long *, long long *, long long *, long long *,
                                                      long long *, hipStream_t, size_t);

}  // namespace asg
