// torch_asg_amd/csrc/asg_beam_window.hip -- WINDOWED streaming beam decoding on gfx950: the stream of asg_beam_stream.hip in
// bounded memory.  The search is the same (asg_beam_frame.h, compiled into this translation unit as into the other two), but the
// back-pointers live in a RING of W rows -- frame u in row u mod W -- and the prefix of the transcript on which all surviving
// hypotheses agree is COMMITTED: handed out by the advance that finds it and never looked at again.  The specification is
// include/asg_hip.h::asg_beam_window_advance; tests/beam_window_ref.py restates it.  The window never touches the search: the
// frame body reads its sources from the set in LDS and writes the row it is given.
//
// One slot of the state (beam_window_layout; every part 256-byte aligned):
//   the one-shot decoder's workspace of one utterance with T = W (asg_beam_common.h, beam_work_layout): bq / bs int32 [W][K], arg
//     u64 [Q], val key [Q], ckey key [cap], touched int32 [cap];
//   a 256-byte header: int64 pos (frames consumed), int64 base (frames committed), int32 |A|, carry (label of the last committed
//     frame, -1: none), status (bit 0: a forced commit has happened);
//   the stored set: values [K] (dtype), then product states int32 [K].
// Three kernels, each one launch, no host synchronisation, no copy, no memset:
//   beam_window_reset_kernel    per chosen slot: the header zeroed (carry -1), val = 0 and arg = none for all Q states.
//   beam_window_advance_kernel  one 1024-thread workgroup per slot: the frames of the chunk through beam_frame, a commit attempt
//                               after every frame whose count is a multiple of P, the five outputs of the call with their padding.
//   beam_window_result_kernel   one workgroup per slot: the best end over the stored set, the backtrace over the uncommitted tail
//                               (at most W steps), its collapse started from carry.  It only reads the state.
// A commit attempt is the text of asg_beam_window_common.h, which asg_beam_word_window.hip compiles too: the convergence scan
// (window_converge) finds the latest frame at which every survivor has the same ancestor, window_commit walks that slot's chain
// down to `base` and collapses the labels, window_forced says when the ring is about to overwrite a live row; the clamp of a
// slot's header (window_header) is there as well.  This unit keeps its header, its control blocks and its call of beam_best_end.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_frame.h"
#include "asg_beam_window_common.h"   // the commit attempt, shared with asg_beam_word_window.hip
#include "asg_beam_window_lat.h"      // the keep policy: what a lattice-keeping state keeps besides (asg_beam_conf_window.hip)

namespace asg {

namespace {

constexpr size_t kWinCtlOff = 3072;    // the window's control block sits behind the search's inside the fixed LDS

// The header of a slot (asg_beam_window_common.h has it, for the n-best kernel that reads it).
using WinHdr = TokenWinHdr;

// What a commit attempt shares (LDS, behind Ctl inside the first kFixedLds bytes).
struct WinCtl {
    long long base;          // frames committed so far
    int carry, status;
    int ncommit, ntok;       // frames / tokens this call has appended to its outputs
    WinScan scan;
};
constexpr size_t kWinOutOff = kWinCtlOff + 64;

__global__ void __launch_bounds__(256) beam_window_reset_kernel(char *state, BeamStreamLayout lay, BeamWorkLayout wl, int Q,
                                                                 int key_bytes, const unsigned char *mask) {
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;
    char *wb = state + (size_t) b * lay.per;
    beam_reset_tables(wb, wl, Q, key_bytes);
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        WinHdr *h = (WinHdr *) (wb + lay.hdr);
        h->pos = 0; h->base = 0; h->na = 0; h->carry = -1; h->status = 0;
    }
}

// What the commits of one call write to, and the ring they read (LDS, behind WinCtl: a commit is rare, and the frame loop
// keeps its scalar registers for the search).
template <bool FR>
struct WinOutT {
    static constexpr bool kWords = false;    // (window_commit: no ring of LM states, no words)
    static constexpr bool kFrames = FR;      // (... and the tokens' start frames for a lattice-keeping state)
    const int *bq, *bs;          // the ring [W][K]
    int K, Q, W;
    const int *label, *state;
    long long *np, *ns, *nt;     // this slot's rows of new_path / new_states / new_tokens
    long long cols;              // W + Tc
    long long *tf;               // kFrames: this slot's row of new_token_frames
};
static_assert(sizeof(Ctl<unsigned long long>) <= kWinCtlOff && sizeof(WinCtl) <= 64 &&
              kWinOutOff + sizeof(WinOutT<true>) <= kFixedLds, "control blocks");

template <typename R, bool TRL, typename Keep>
__global__ void __launch_bounds__(kBT) beam_window_advance_kernel(Problem P, GraphArgs g, BeamGraphArgs bg, int K, R theta, int cap,
                                                                  int W, int CP, char *state, BeamStreamLayout lay,
                                                                  long long *new_path, long long *new_states,
                                                                  long long *new_tokens, long long *new_frames,
                                                                  long long *new_tlen, Keep keep) {
    using KT = Key<R>;
    using WinOut = WinOutT<Keep::kLattice>;
    using U = typename KT::U;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    Ctl<U> &ctl = *(Ctl<U> *) lds;
    WinCtl &wc = *(WinCtl *) (lds + kWinCtlOff);
    unsigned *mark = (unsigned *) (lds + kFixedLds);       // the two mark sets of the scan
    R *cur_v = (R *) (lds + kFixedLds + mark_bytes(K));    // [K]
    int *cur_q = (int *) (cur_v + K);                      // [K]
    R *trs = (R *) (cur_q + K + (K & 1));                  // [N][N] if TRL
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = P.N;
    char *wb = state + (size_t) b * lay.per;
    WinHdr *hdr = (WinHdr *) (wb + lay.hdr);
    R *set_v = (R *) (wb + lay.set);                        // values [K], then product states [K]
    const long long cols = (long long) W + P.T;
    WinOut &o = *(WinOut *) (lds + kWinOutOff);
    long long *np = new_path + (int64_t) b * cols, *ns = new_states + (int64_t) b * cols, *nt = new_tokens + (int64_t) b * cols;
    if (tid == 0) {
        o.bq = nullptr; o.bs = nullptr;
        o.K = K; o.Q = g.Q; o.W = W; o.label = g.label; o.state = g.state; o.cols = cols;
        o.np = np; o.ns = ns; o.nt = nt;
        if constexpr (Keep::kLattice) o.tf = keep.tf + (int64_t) b * cols;
    }

    long long pos = hdr->pos, base0 = hdr->base;
    int na0 = hdr->na;
    window_header(pos, base0, na0, K);
    if (na0 > 0) base0 = window_live_base(pos, base0, W);
    const int n = clamp_len(P.in_len, b, P.T);
    if (tid == 0) { wc.base = base0; wc.carry = hdr->carry; wc.status = hdr->status; wc.ncommit = 0; wc.ntok = 0; }
    keep.chunk(wb, (const R *) P.inputs + (int64_t) b * P.is1, P, pos, n);
    int logged = 0;                                         // (a lattice-keeping state's: the attempts in its log)

    if (n >= 1) {
        const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
        const R *tr = (const R *) P.transition;
        BeamFrame<R> f;
        f.ctl = &ctl; f.cur_v = cur_v; f.cur_q = cur_q; f.trs = trs; f.tr = tr; f.ts0 = P.ts0; f.ts1 = P.ts1;
        f.N = N; f.Q = g.Q; f.K = K; f.G = beam_lanes_per_state(K); f.theta = theta;
        f.label = g.label; f.orow = bg.orow; f.start_q = bg.start_q; f.num_start = bg.num_start;
        f.oarc = (const int2 *) bg.oarc; f.ow = (const R *) bg.ow; f.sw = (const R *) g.start_w;
        int *bq, *bs;
        f.bind_work(wb, W, cap, bq, bs);
        if (tid == 0) { o.bq = bq; o.bs = bs; }

        beam_load_set<R, TRL>(f, trs, set_v, na0);

        int row = (int) (pos % W), ph = (int) (pos % CP);   // the next frame's row, and pos mod P; both kept by stepping
        int ran = 0;
        for (int t = 0; t < n; ++t) {
            const long long gt = pos + t;                   // the frame's index in the utterance
            int na = ctl.na;
            if (gt >= 1 && na == 0) break;                  // an empty beam stays empty (and commits nothing more)
            const int fr = row;
            beam_frame<R, TRL>(f, gt == 0, na, in + (int64_t) t * P.is0, P.is2, bq, bs, fr);
            if constexpr (Keep::kLattice) {
                ran = t + 1;
                keep.frame(wb, gt, ctl.na < K ? ctl.na : K, bq + (int64_t) fr * K, K);
            }
            const long long p1 = gt + 1;                    // pos, counting this frame
            row = row + 1 == W ? 0 : row + 1;
            ph = ph + 1 == CP ? 0 : ph + 1;
            na = ctl.na;
            na = na < K ? na : K;
            if (ph != 0 || na == 0) continue;
            // ================================================================ commit attempt
            // ---- convergence: the latest frame at which every survivor has the same ancestor
            long long base = wc.base;
            const long long b0 = base;
            int tk0 = 0;
            if constexpr (Keep::kLattice) tk0 = wc.ntok;
            int cslot, crow;
            const long long c = window_converge(bs, K, W, na, p1, base, fr, mark, wc.scan, cslot, crow);
            if (c >= base) {
                window_commit(wc, o, c, crow, c, cslot);
                base = wc.base;
            }
            // ---- forced commit: the next CP frames must not overwrite a live row
            const long long F = window_forced(p1, base, W, CP);
            if (F > 0) {
                U bkey;
                int bqq, bk;
                beam_best_end<R>(ctl, cur_q, cur_v, na, nullptr, bkey, bqq, bk);
                __syncthreads();                            // (the reduction slots are read before anything reuses them)
                if (bk >= 0) {
                    if (tid == 0) wc.status |= 1;
                    window_commit(wc, o, p1 - 1, fr, base + F - 1, bk);
                }
            }
            if constexpr (Keep::kLattice) {                 // one attempt is one lattice end, whatever it committed
                const int tk1 = wc.ntok;
                if (tk1 > tk0) keep.attempt(wb, logged++, p1, b0, tk0, tk1);
            }
        }
        keep.skipped(wb, pos, ran, n);
        const int na = beam_store_set<R>(f, set_v);
        if (tid == 0) hdr->na = na;
    }
    __syncthreads();
    const int nc = wc.ncommit, ntk = wc.ntok;
    for (long long x = nc + tid; x < cols; x += kBT) { np[x] = -1; ns[x] = -1; }
    for (long long x = ntk + tid; x < cols; x += kBT) nt[x] = -1;
    keep.done(wb, logged, ntk, cols);
    if (tid == 0) {
        new_frames[b] = nc;
        new_tlen[b] = ntk;
        hdr->pos = pos + n; hdr->base = wc.base; hdr->carry = wc.carry; hdr->status = wc.status;
    }
}

template <typename R>
__global__ void __launch_bounds__(kBT) beam_window_result_kernel(GraphArgs g, int K, int cap, int W, const char *state,
                                                                 BeamStreamLayout lay, int final, R *scores, long long *path,
                                                                 long long *tokens, long long *tlen, long long *states,
                                                                 long long *frames, long long *committed, long long *status) {
    using U = typename Key<R>::U;
    __shared__ Ctl<U> ctl;
    const int tid = threadIdx.x, b = blockIdx.x;
    const R NINF = Num<R>::ninf();
    const char *wb = state + (size_t) b * lay.per;
    const WinHdr *hdr = (const WinHdr *) (wb + lay.hdr);
    const R *set_v = (const R *) (wb + lay.set);
    const int *set_q = (const int *) (set_v + K);
    const BeamWorkLayout wl = beam_work_layout(sizeof(R), W, g.Q, K, cap);
    const int *bq = (const int *) (wb + wl.bq), *bs = (const int *) (wb + wl.bs);             // the ring [W][K]
    long long *pb = path + (int64_t) b * W, *tk = tokens + (int64_t) b * W, *st = states + (int64_t) b * W;
    long long pos = hdr->pos, base = hdr->base;
    int na = hdr->na;
    window_header(pos, base, na, K);
    if (tid == 0) {
        frames[b] = pos;
        committed[b] = base;
        status[b] = (hdr->status & 1) | (pos >= 1 && na == 0 ? 2 : 0);
    }
    const R *fw = final ? (const R *) g.final_w : nullptr;
    U bkey;
    int bqq, bk;
    beam_best_end<R>(ctl, set_q, set_v, na, fw, bkey, bqq, bk);
    if (bkey == 0) {                                        // no frame yet, an empty set, or no finite end
        beam_no_path(W, pb, tk, st, tlen + b);
        if (tid == 0) scores[b] = NINF;
        return;
    }
    if (tid == 0) scores[b] = fw ? set_v[bk] + fw[bqq] : set_v[bk];
    base = window_live_base(pos, base, W);                  // (a set that is not empty has pos <= base + W)
    const int live = (int) (pos - base);                    // 0 .. W
    for (int t = live + tid; t < W; t += kBT) { pb[t] = -1; st[t] = -1; }
    if (tid == 0) {
        int k = bk;
        long long t = pos - 1;
        for (; t >= base; --t) {
            if ((unsigned) k >= (unsigned) K) break;         // (cannot happen: every kept state stored its source's slot)
            const int64_t at = (int64_t) (t % W) * K + k;
            int q = bq[at];
            q = (unsigned) q < (unsigned) g.Q ? q : 0;
            k = bs[at];
            pb[t - base] = g.label[q];
            st[t - base] = g.state[q];
        }
        for (; t >= base; --t) { pb[t - base] = -1; st[t - base] = -1; }
    }
    __threadfence();
    __syncthreads();
    if (tid < 64) {
        long long carry = hdr->carry;
        const int nt = collapse_tokens_from(pb, live, carry, tk, tid);
        for (int t = nt + tid; t < W; t += 64) tk[t] = -1;
        if (tid == 0) tlen[b] = nt;
    }
}

}  // namespace

// The slot of a window stream is the slot of a stream of W frames: the ring has the [frame][K] layout with W rows.
BeamStreamLayout beam_window_layout(int elem, int W, int Q, int K, int cap) { return beam_stream_layout(elem, W, Q, K, cap); }

size_t beam_window_state_bytes(int elem, int W, int B, int Q, int K, int cap) {
    return (size_t) B * beam_window_layout(elem, W, Q, K, cap).per;
}

hipError_t launch_beam_window_reset(int elem, const GraphArgs &G, const BeamGraphArgs &BG, int K, int W, int B, void *state,
                                    const unsigned char *mask, hipStream_t stream, size_t stride) {
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    BeamStreamLayout lay = beam_window_layout(elem, W, G.Q, K, cap);
    if (stride) lay.per = stride;                                           // (a slot with parts of the caller's behind it)
    hipLaunchKernelGGL(beam_window_reset_kernel, dim3(B, reset_blocks(G.Q)), dim3(256), 0, stream, (char *) state, lay,
                       beam_work_layout(elem, W, G.Q, K, cap), G.Q, elem, mask);
    return hipGetLastError();
}

namespace {

template <typename R, typename Keep>
hipError_t beam_window_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta, int cap, int W,
                               int CP, void *state, const BeamStreamLayout &lay, long long *new_path, long long *new_states,
                               long long *new_tokens, long long *new_frames, long long *new_tlen, Keep keep, hipStream_t stream) {
    const int N = P.N;
    // the LDS of the one-shot decoder plus the two mark sets: control blocks, marks, the set, and the transitions when they fit
    const size_t beam = kFixedLds + mark_bytes(K) + (size_t) K * (sizeof(R) + 4) + 8;
    const bool trl = beam + (size_t) N * N * sizeof(R) <= kLdsMax;
    const size_t dyn = beam + (trl ? (size_t) N * N * sizeof(R) : 0);
#define ASG_BEAM_WINDOW(TRL)                                                                                               \
    do {                                                                                                                   \
        const void *fn = (const void *) beam_window_advance_kernel<R, TRL, Keep>;                                         \
        if (dyn > 64 * 1024) (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dyn);     \
        hipLaunchKernelGGL((beam_window_advance_kernel<R, TRL, Keep>), dim3(P.B), dim3(kBT), dyn, stream, P, G, BG, K,   \
                           (R) theta, cap, W, CP, (char *) state, lay, new_path, new_states, new_tokens, new_frames,       \
                           new_tlen, keep);                                                                                \
    } while (0)
    if (trl) ASG_BEAM_WINDOW(true); else ASG_BEAM_WINDOW(false);
#undef ASG_BEAM_WINDOW
    return hipGetLastError();
}

}  // namespace

template <typename R>
hipError_t launch_beam_window_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta, int W,
                                      int CP, void *state, long long *new_path, long long *new_states, long long *new_tokens,
                                      long long *new_frames, long long *new_tlen, hipStream_t stream,
                                      const BeamConfWindowLayout *cw, long long *new_token_frames) {
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    if (cw) {
        WinKeepLattice keep{};
        keep.hdr = cw->st.hdr; keep.cnt = cw->lat.cnt; keep.em = cw->em; keep.U = cw->lat.U; keep.log = cw->log;
        keep.RW = cw->RW; keep.nlog = cw->nlog; keep.tf = new_token_frames;
        return beam_window_advance<R>(P, G, BG, K, theta, cap, W, CP, state, cw->st, new_path, new_states, new_tokens, new_frames,
                                      new_tlen, keep, stream);
    }
    return beam_window_advance<R>(P, G, BG, K, theta, cap, W, CP, state, beam_window_layout(sizeof(R), W, G.Q, K, cap), new_path,
                                  new_states, new_tokens, new_frames, new_tlen, WinKeepNone{}, stream);
}
template hipError_t launch_beam_window_advance<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, double, int,
                                                      int, void *, long long *, long long *, long long *, long long *, long long *,
                                                      hipStream_t, const BeamConfWindowLayout *, long long *);
template hipError_t launch_beam_window_advance<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, int, double, int,
                                                       int, void *, long long *, long long *, long long *, long long *,
                                                       long long *, hipStream_t, const BeamConfWindowLayout *, long long *);

template <typename R>
hipError_t launch_beam_window_result(const GraphArgs &G, const BeamGraphArgs &BG, int K, int W, int B, const void *state, int final,
                                     void *scores, long long *path, long long *tokens, long long *tlen, long long *states,
                                     long long *frames, long long *committed, long long *status, hipStream_t stream,
                                     size_t stride) {
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    BeamStreamLayout lay = beam_window_layout(sizeof(R), W, G.Q, K, cap);
    if (stride) lay.per = stride;                                           // (a slot with parts of the caller's behind it)
    hipLaunchKernelGGL((beam_window_result_kernel<R>), dim3(B), dim3(kBT), 0, stream, G, K, cap, W, (const char *) state, lay, final,
                       (R *) scores, path, tokens, tlen, states, frames, committed, status);
    return hipGetLastError();
}
template hipError_t launch_beam_window_result<float>(const GraphArgs &, const BeamGraphArgs &, int, int, int, const void *, int,
                                                     void *, long long *, long long *, long long *, long long *, long long *,
                                                     long long *, long long *, hipStream_t, size_t);
template hipError_t launch_beam_window_result<double>(const GraphArgs &, const BeamGraphArgs &, int, int, int, const void *, int,
                                                      void *, long long *, long long *, long long *, long long *, long long *,
                                                      long long *, long long *, hipStream_t, size_t);

}  // namespace asg
