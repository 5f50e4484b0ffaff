// torch_asg_amd/csrc/asg_api.hip -- the C ABI declared in include/asg_hip.h.
// Argument validation, state/scratch layout, path selection (small / generic), stream fork-join.
// No torch, no pybind: plain HIP runtime calls only.
#include "../../include/asg_hip.h"
#include "asg_kernels.h"
#include "asg_common.h"

#include <hip/hip_runtime.h>
#include <new>
#include <atomic>
#include <cstdlib>

using namespace asg;

namespace asg {
size_t bwd_scratch_bytes_small(int elem, int T, int B, int N, int S, int *chunk, int *nchunks) {
    // at most ~512 workgroups: the assembly kernel holds two workgroups per compute unit (243 VGPRs), so 512 are ONE round on 256
    // CUs; anything above it is a second, mostly empty round (round 3 rounded UP: B = 192 got 3 x 192 = 576 workgroups and ran
    // slower than B = 256 with 2 x 256).  At least 16 frames per workgroup.
    int target = 512;
#ifdef ASG_DEV_PROBES
    if (const char *ev = getenv("ASG_BWD_WGS")) target = atoi(ev) > 0 ? atoi(ev) : target;   // developer probe
#endif
    int nch = target / B;
    if (nch < 1) nch = 1;
    int ch = (T + nch - 1) / nch;
    if (ch < 16) ch = 16;
    ch = (ch + 15) / 16 * 16;      // whole 16-frame blocks (bwd_mfma_kernel)
    nch = (T + ch - 1) / ch;
    if (nch < 1) nch = 1;
    if (chunk) *chunk = ch;
    if (nchunks) *nchunks = nch;
    return (size_t) B * nch * N * N * elem;
}
}  // namespace asg

namespace asg {
namespace {
std::atomic<const Knobs *> g_knobs{nullptr};
int env_int(const char *name) { const char *v = getenv(name); return v ? atoi(v) : -1; }
const Knobs *read_knobs() {
    Knobs *k = new Knobs();          // (a handful per process at most: never freed, readers may still hold the old one)
    k->fork_in_capture = env_int("ASG_FORK_IN_CAPTURE");
    k->pair_min_b = env_int("ASG_PAIR_MIN_B");
    k->bwd_rowsum = env_int("ASG_BWD_ROWSUM");
    k->no_cluster = env_int("ASG_NO_CLUSTER");
    k->no_mid = env_int("ASG_NO_MID");
    k->no_tile_step = env_int("ASG_NO_TILE_STEP");
    k->step_one_tile = env_int("ASG_STEP_ONE_TILE");
    k->step_row_blocks = env_int("ASG_STEP_ROW_BLOCKS");
    k->step_full_tile = env_int("ASG_STEP_FULL_TILE");
    k->step_no_bf3 = env_int("ASG_STEP_NO_BF3");
    k->step_bf3_min_b = env_int("ASG_STEP_BF3_MIN_B");
    const char *ak = getenv("ASG_ALIGNED_KERNEL");
    k->aligned_kernel = ak ? ak[0] : 0;
    return k;
}
}  // namespace
const Knobs &knobs() {
    const Knobs *k = g_knobs.load(std::memory_order_acquire);
    if (!k) {
        const Knobs *fresh = read_knobs();
        if (g_knobs.compare_exchange_strong(k, fresh, std::memory_order_acq_rel)) k = fresh;
        else delete fresh;
    }
    return *k;
}
}  // namespace asg

// Host-side handles only (side stream + fork/join events of ASG_FLAG_STREAMS); no device memory, no per-call state:
// everything a call mutates on the device lives in the caller-owned `state` buffer of that call.
struct asg_ctx {
    hipStream_t side;
    hipEvent_t fork, join;
    int device;
};

namespace {

inline int hip_status(hipError_t e) { return e == hipSuccess ? ASG_OK : ASG_ERR_HIP_BASE + (int) e; }

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t) 255; }

struct Layout {
    size_t ah, bh, ab, bb, klog, ehat, fhat, rmax, cmax, etile, ftile, asu, asi, dbg, ticket, work, total;
    int npad;
};

inline bool small_full(int64_t N) { return N <= 64; }
inline bool small_aligned(int64_t S) { return S <= 64; }

Layout make_layout(const asg_problem *p) {
    Layout L{};
    const size_t e = p->dtype == ASG_DTYPE_F64 ? 8 : 4;
    const size_t T = p->T, B = p->B, N = p->N, S = p->S < 1 ? 1 : p->S;
    size_t off = 0;
    L.ah = off; off = align_up(off + B * T * N * e);
    L.bh = off; off = align_up(off + B * T * N * e);
    // aligned states: the problem's type on the small path, doubles from the long-target kernels (S > 64: asg_generic.hip, AlignedState)
    const size_t ea = small_aligned((int64_t) S) ? e : 8;
    L.ab = off; off = align_up(off + B * T * S * ea);
    L.bb = off; off = align_up(off + B * T * S * ea);
    if (small_full(p->N)) { L.klog = off; off = align_up(off + B * T * 2 * e); }      // scale log of the alpha pass (ScaleLog)
    L.npad = small_full(p->N) ? (int) ((N + 7) / 8 * 8) : (int) ((N + 3) / 4 * 4);
    L.ehat = off; off = align_up(off + N * L.npad * e);
    L.rmax = off; off = align_up(off + N * e);
    if (!small_full(p->N)) {
        L.fhat = off; off = align_up(off + N * L.npad * e);
        L.cmax = off; off = align_up(off + N * e);
        const size_t tb = step_tile_bytes_generic((int) e, (int) N, (int) B);
        L.etile = off; off = align_up(off + tb);
        L.ftile = off; off = align_up(off + tb);
    }
    L.asu = off; off = align_up(off + B * S * 2 * e);
    L.asi = off; off = align_up(off + B * S * 2 * sizeof(int));
    L.dbg = off; off = align_up(off + 512);      // developer timing stamps (ASG_PROBE builds only)
    L.ticket = off; off = align_up(off + 256);   // arrival ticket of the in-kernel loss reduction (zeroed per call)
    if (!small_full(p->N)) { L.work = off; off = align_up(off + fwd_work_bytes_generic((int) e, (int) T, (int) B, (int) N)); }
    L.total = off;
    return L;
}

int check_problem(const asg_problem *p, bool need_targets, bool allow_bf16 = false) {
    if (!p) return ASG_ERR_INVALID;
    if (p->dtype != ASG_DTYPE_F32 && p->dtype != ASG_DTYPE_F64) return ASG_ERR_INVALID;
    if (p->inputs_dtype != 0 && !(p->inputs_dtype == ASG_DTYPE_BF16 && p->dtype == ASG_DTYPE_F32)) return ASG_ERR_INVALID;
    if (p->inputs_dtype != 0 && !allow_bf16) return ASG_ERR_UNSUPPORTED;      // bfloat16 emissions: the fused pair only
    if (p->T < 1 || p->B < 1 || p->N < 1) return ASG_ERR_INVALID;
    if (!p->inputs || !p->transition) return ASG_ERR_INVALID;
    if (need_targets && (p->S < 1 || !p->targets)) return ASG_ERR_INVALID;
    if (p->T > (1 << 30) || p->B > (1 << 30) || p->N > (1 << 30) || p->S > (1 << 30)) return ASG_ERR_UNSUPPORTED;
    if (p->S > 8192) return ASG_ERR_UNSUPPORTED;              // aligned kernels: at most eight target positions per thread of a workgroup, a frame's states in LDS
    if (p->S > 1024 && (double) p->N * (p->dtype == ASG_DTYPE_F64 ? 8.0 : 4.0) > 150.0 * 1024.0) return ASG_ERR_UNSUPPORTED;   // ... and beyond 1024 the label scatter is one LDS row of N words (bwd_aligned_strip_kernel)
    {
        // the kernels address state and gradient rows through 32-bit buffer offsets
        const double e = p->dtype == ASG_DTYPE_F64 ? 8.0 : 4.0;
        const double w = (double) (p->N > p->S ? p->N : p->S);
        if ((double) p->T * (double) p->B * w * e >= 4294967296.0 && small_full(p->N)) return ASG_ERR_UNSUPPORTED;
    }
    return ASG_OK;
}

Problem to_problem(const asg_problem *p) {
    Problem P{};
    P.inputs = p->inputs;
    P.is0 = p->inputs_strides[0]; P.is1 = p->inputs_strides[1]; P.is2 = p->inputs_strides[2];
    P.transition = p->transition;
    P.ts0 = p->transition_strides[0]; P.ts1 = p->transition_strides[1];
    P.targets = p->targets;
    P.gs0 = p->targets_strides[0]; P.gs1 = p->targets_strides[1];
    P.in_len = p->input_lengths;
    P.tg_len = p->target_lengths;
    P.T = (int) p->T; P.B = (int) p->B; P.N = (int) p->N; P.S = (int) (p->S < 1 ? 1 : p->S);
    P.in_bf16 = p->inputs_dtype == ASG_DTYPE_BF16 ? 1 : 0;
    return P;
}

State to_state(const asg_problem *p, const void *state) {
    Layout L = make_layout(p);
    char *base = (char *) state;
    State W{};
    if (base) {
        W.ah = base + L.ah; W.bh = base + L.bh; W.ab = base + L.ab; W.bb = base + L.bb;
        W.ehat = base + L.ehat; W.rmax = base + L.rmax;
        if (!small_full(p->N)) { W.fhat = base + L.fhat; W.cmax = base + L.cmax; W.etile = base + L.etile; W.ftile = base + L.ftile; }
        W.asu = base + L.asu; W.asi = (int *) (base + L.asi);
        W.dbg = base + L.dbg;
        W.ticket = (unsigned *) (base + L.ticket);
        if (!small_full(p->N)) W.work = base + L.work;
        else W.klog = base + L.klog;
    }
    W.npad = L.npad;
    return W;
}

// Is `stream` being captured into a hipGraph?  (ASG_FORK_IN_CAPTURE=1 / 0: developer override of what run_forward does with it.)
inline bool capturing(hipStream_t stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) { (void) hipGetLastError(); return false; }
    return st == hipStreamCaptureStatusActive;
}

template <typename R>
int run_forward(asg_ctx *ctx, const asg_problem *p, void *state, void *full_scores, void *aligned_scores,
                int mask, bool store, int flags, hipStream_t stream, void *loss = nullptr, int reduction = 0,
                unsigned *ticket = nullptr) {
    Problem P = to_problem(p);
    // Two streams (fork / join through ctx) only help when the two lattices' kernels really run side by side.  Recorded into a
    // hipGraph, ROCm 7.2 replays the two branches of the SHORT kernels one after the other with ~12 us per cross-queue edge
    // (profiles/r04_streams_graph_trace.txt: cfg 3, fwd_duo_kernel 48.6 us, then a 13 us gap, then the aligned chains 37 us,
    // then 11 us before the backward launch): while capturing, the small path records its passes on the caller's stream.
    bool fork_ok = true;
    {
        const int mode = knobs().fork_in_capture;        // -1: default policy
        if (mode == 0) fork_ok = !capturing(stream);
        else if (mode < 0) fork_ok = !(small_full(p->N) && small_aligned(p->S) && capturing(stream));
    }
    State W = to_state(p, state);
    FwdOut O{};
    O.full_scores = full_scores;
    O.aligned_scores = aligned_scores;
    if (loss && small_full(p->N) && small_aligned(p->S)) {
        // the last beta pass to finish reduces the loss; its arrival ticket is part of THIS call's state buffer
        // and is zeroed on the launch stream ahead of the kernels (a memset node under graph capture)
        O.loss = loss;
        O.counter = ticket ? ticket : W.ticket;           // (the evaluation route has no state buffer: its caller lends 256 bytes)
        O.reduction = reduction;
        O.expected = 2 * (int) p->B;
        // (a kernel, not hipMemsetAsync: asg_common.h::zero_async says why)
        hipError_t me = zero_async(O.counter, 256, stream);
        if (me != hipSuccess) return hip_status(me);
    }
    if ((flags & ASG_FLAG_ALPHA_SCORES) && store) {
        if (full_scores) O.full_scores_alpha = (R *) full_scores + p->B;
        if (aligned_scores) O.aligned_scores_alpha = (R *) aligned_scores + p->B;
    }
#ifdef ASG_DEV_PROBES
    if (const char *dm = getenv("ASG_DEBUG_MASK")) mask &= atoi(dm);      // developer probe: time single passes
#endif
    const int full_mask = mask & (kFullAlpha | kFullBeta);
    const int ali_mask = mask & (kAlignedAlpha | kAlignedBeta);
    const bool sf = small_full(p->N), sa = small_aligned(p->S);
    if ((full_mask && !sf) || (ali_mask && !sa)) {
        // generic path (any N / S up to 1024)
        hipError_t e = hipSuccess;
        if (full_mask && !sf) {
            e = launch_prep_generic<R>(P, W, stream);
            if (e != hipSuccess) return hip_status(e);
        }
        // two streams also for the default launch mode: on this route the two lattices are separate launches anyway (one
        // launch per lattice, or per frame), and overlapping them is worth more than the fork / join costs (T=1000 B=64
        // N=40 S=200: 492 -> 420 us per step inside a hipGraph)
        bool two = (flags & (ASG_FLAG_STREAMS | ASG_FLAG_SINGLE_LAUNCH)) && ctx && full_mask && ali_mask && fork_ok;
        hipStream_t s2 = two ? ctx->side : stream;
        if (two) {
            if ((e = hipEventRecord(ctx->fork, stream)) != hipSuccess) return hip_status(e);
            if ((e = hipStreamWaitEvent(s2, ctx->fork, 0)) != hipSuccess) return hip_status(e);
        }
        if (full_mask) {
            e = sf ? launch_fwd_small<R>(P, W, O, full_mask, store, stream)
                   : launch_fwd_generic<R>(P, W, O, full_mask, store, stream);
            if (e != hipSuccess) return hip_status(e);
        }
        if (ali_mask) {
            e = sa ? launch_fwd_small<R>(P, W, O, ali_mask, store, s2)
                   : launch_fwd_generic<R>(P, W, O, ali_mask, store, s2);
            if (e != hipSuccess) return hip_status(e);
        }
        if (two) {
            if ((e = hipEventRecord(ctx->join, s2)) != hipSuccess) return hip_status(e);
            if ((e = hipStreamWaitEvent(stream, ctx->join, 0)) != hipSuccess) return hip_status(e);
        }
        return ASG_OK;
    }
    hipError_t e;
    if ((flags & ASG_FLAG_STREAMS) && ctx && full_mask && ali_mask && fork_ok) {
        // fork: aligned passes on the side stream, full passes on the caller's stream; join back.
        if ((e = hipEventRecord(ctx->fork, stream)) != hipSuccess) return hip_status(e);
        if ((e = hipStreamWaitEvent(ctx->side, ctx->fork, 0)) != hipSuccess) return hip_status(e);
        if ((e = launch_fwd_small<R>(P, W, O, full_mask, store, stream)) != hipSuccess) return hip_status(e);
        if ((e = launch_fwd_small<R>(P, W, O, ali_mask, store, ctx->side)) != hipSuccess) return hip_status(e);
        if ((e = hipEventRecord(ctx->join, ctx->side)) != hipSuccess) return hip_status(e);
        if ((e = hipStreamWaitEvent(stream, ctx->join, 0)) != hipSuccess) return hip_status(e);
        return ASG_OK;
    }
    if (flags & ASG_FLAG_SINGLE_LAUNCH) return hip_status(launch_fwd_small<R>(P, W, O, mask, store, stream));
    if (full_mask && (e = launch_fwd_small<R>(P, W, O, full_mask, store, stream)) != hipSuccess) return hip_status(e);
    if (ali_mask && (e = launch_fwd_small<R>(P, W, O, ali_mask, store, stream)) != hipSuccess) return hip_status(e);
    return ASG_OK;
}

template <typename R>
int run_backward(const asg_problem *p, const void *state, const void *grad_full, const void *grad_aligned,
                 void *scratch, size_t scratch_bytes, void *grad_transition, void *grad_inputs, int parts,
                 hipStream_t stream, int gstride = 1, double gscale = 1.0, int neg_aligned = 0) {
    Problem P = to_problem(p);
    State W = to_state(p, state);
    BwdArgs A{};
    A.grad_full = grad_full ? grad_full : grad_aligned;
    A.grad_aligned = grad_aligned;
    A.gstride = gstride;
    A.gscale = gscale;
    A.neg_aligned = neg_aligned;
    A.grad_inputs = grad_inputs;
    A.grad_transition = grad_transition;
    A.scratch = scratch;
    if (scratch_bytes < asg_scratch_bytes(p)) return ASG_ERR_WORKSPACE;
    const bool sf = small_full(p->N), sa = small_aligned(p->S);
    bwd_scratch_bytes_small((int) sizeof(R), P.T, P.B, P.N, P.S, &A.chunk, &A.nchunks);
    if (sf && (sa || !(parts & 2))) return hip_status(launch_bwd_small<R>(P, W, A, parts, stream));
    // mixed / generic: full-lattice part by whichever path owns N, aligned part by the generic kernels
    hipError_t e = hipSuccess;
    int gparts = 0;
    if (parts & 1) {
        if (sf) {
            if ((e = launch_bwd_small<R>(P, W, A, 1, stream)) != hipSuccess) return hip_status(e);
            gparts |= 4;
        } else {
            gparts |= 1;
        }
    }
    if (parts & 2) gparts |= 2;
    return hip_status(launch_bwd_generic<R>(P, W, A, gparts, stream));
}

}  // namespace

extern "C" {

int asg_hip_version(void) { return ASG_HIP_VERSION; }

const char *asg_hip_strerror(int status) {
    switch (status) {
        case ASG_OK: return "ok";
        case ASG_ERR_INVALID: return "invalid argument";
        case ASG_ERR_UNSUPPORTED: return "unsupported problem shape";
        case ASG_ERR_WORKSPACE: return "state or scratch buffer too small";
        default: break;
    }
    if (status >= ASG_ERR_HIP_BASE) return hipGetErrorString((hipError_t) (status - ASG_ERR_HIP_BASE));
    return "unknown error";
}

unsigned asg_cluster_timeouts(void) { return cluster_timeouts(); }

void asg_reload_env(void) { g_knobs.store(read_knobs(), std::memory_order_release); }

int asg_ctx_create(asg_ctx **out) {
    if (!out) return ASG_ERR_INVALID;
    asg_ctx *c = new (std::nothrow) asg_ctx();
    if (!c) return ASG_ERR_INVALID;
    hipError_t e = hipGetDevice(&c->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->join, hipEventDisableTiming);
    if (e != hipSuccess) { delete c; return hip_status(e); }
    *out = c;
    return ASG_OK;
}

int asg_stream_capture_id(void *stream, unsigned long long *id) {
    if (!id) return ASG_ERR_INVALID;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long cid = 0;
    hipError_t e = hipStreamGetCaptureInfo((hipStream_t) stream, &st, &cid);
    if (e != hipSuccess) return hip_status(e);
    *id = st == hipStreamCaptureStatusActive ? (cid ? cid : ~0ull) : 0;
    return ASG_OK;
}

int asg_ctx_destroy(asg_ctx *c) {
    if (!c) return ASG_OK;
    (void) hipEventDestroy(c->fork);
    (void) hipEventDestroy(c->join);
    (void) hipStreamDestroy(c->side);
    delete c;
    return ASG_OK;
}

size_t asg_state_bytes(const asg_problem *p) {
    if (!p || p->T < 1 || p->B < 1 || p->N < 1) return 0;
    asg_problem q = *p;
    if (q.S < 1) q.S = 1;
    return make_layout(&q).total;
}

size_t asg_loss_forward_only_scores_bytes(const asg_problem *p) {
    if (!p || p->B < 1) return 0;
    return align_up(2 * (size_t) p->B * (p->dtype == ASG_DTYPE_F64 ? 8 : 4)) + 256;
}

size_t asg_scratch_bytes(const asg_problem *p) {
    if (!p || p->T < 1 || p->B < 1 || p->N < 1) return 0;
    const int e = p->dtype == ASG_DTYPE_F64 ? 8 : 4;
    const int S = (int) (p->S < 1 ? 1 : p->S);
    size_t a = 256;
    if (small_full(p->N)) {
        size_t s = bwd_scratch_bytes_small(e, (int) p->T, (int) p->B, (int) p->N, S, nullptr, nullptr);
        if (s > a) a = s;
    }
    if (!small_full(p->N) || !small_aligned(S)) {
        size_t s = bwd_scratch_bytes_generic(e, (int) p->T, (int) p->B, (int) p->N, S);
        if (s > a) a = s;
    }
    return a;
}

#define ASG_DISPATCH(p, call_f32, call_f64) ((p)->dtype == ASG_DTYPE_F32 ? (call_f32) : (call_f64))

int asg_full_forward(const asg_problem *p, void *state, size_t state_bytes, void *scores, int flags, void *stream) {
    int rc = check_problem(p, false);
    if (rc) return rc;
    if (!state || !scores) return ASG_ERR_INVALID;
    if (state_bytes < asg_state_bytes(p)) return ASG_ERR_WORKSPACE;
    flags &= ~(ASG_FLAG_STREAMS | ASG_FLAG_SINGLE_LAUNCH);
    return ASG_DISPATCH(p,
        run_forward<float>(nullptr, p, state, scores, nullptr, kFullAlpha | kFullBeta, true, flags, (hipStream_t) stream),
        run_forward<double>(nullptr, p, state, scores, nullptr, kFullAlpha | kFullBeta, true, flags, (hipStream_t) stream));
}

int asg_aligned_forward(const asg_problem *p, void *state, size_t state_bytes, void *scores, int flags, void *stream) {
    int rc = check_problem(p, true);
    if (rc) return rc;
    if (!state || !scores) return ASG_ERR_INVALID;
    if (state_bytes < asg_state_bytes(p)) return ASG_ERR_WORKSPACE;
    flags &= ~(ASG_FLAG_STREAMS | ASG_FLAG_SINGLE_LAUNCH);
    return ASG_DISPATCH(p,
        run_forward<float>(nullptr, p, state, nullptr, scores, kAlignedAlpha | kAlignedBeta, true, flags, (hipStream_t) stream),
        run_forward<double>(nullptr, p, state, nullptr, scores, kAlignedAlpha | kAlignedBeta, true, flags, (hipStream_t) stream));
}

int asg_full_backward(const asg_problem *p, const void *state, size_t state_bytes, const void *grad_out,
                      void *scratch, size_t scratch_bytes, void *grad_transition, void *grad_inputs, void *stream) {
    int rc = check_problem(p, false);
    if (rc) return rc;
    if (!state || !grad_out || !scratch || !grad_transition || !grad_inputs) return ASG_ERR_INVALID;
    if (state_bytes < asg_state_bytes(p)) return ASG_ERR_WORKSPACE;
    return ASG_DISPATCH(p,
        run_backward<float>(p, state, grad_out, nullptr, scratch, scratch_bytes, grad_transition, grad_inputs, 1, (hipStream_t) stream),
        run_backward<double>(p, state, grad_out, nullptr, scratch, scratch_bytes, grad_transition, grad_inputs, 1, (hipStream_t) stream));
}

int asg_aligned_backward(const asg_problem *p, const void *state, size_t state_bytes, const void *grad_out,
                         void *scratch, size_t scratch_bytes, void *grad_transition, void *grad_inputs, void *stream) {
    int rc = check_problem(p, true);
    if (rc) return rc;
    if (!state || !grad_out || !scratch || !grad_transition || !grad_inputs) return ASG_ERR_INVALID;
    if (state_bytes < asg_state_bytes(p)) return ASG_ERR_WORKSPACE;
    return ASG_DISPATCH(p,
        run_backward<float>(p, state, nullptr, grad_out, scratch, scratch_bytes, grad_transition, grad_inputs, 2, (hipStream_t) stream),
        run_backward<double>(p, state, nullptr, grad_out, scratch, scratch_bytes, grad_transition, grad_inputs, 2, (hipStream_t) stream));
}

int asg_forward(asg_ctx *ctx, const asg_problem *p, void *state, size_t state_bytes,
                void *full_scores, void *aligned_scores, int flags, void *stream) {
    int rc = check_problem(p, true);
    if (rc) return rc;
    if (!state || !full_scores || !aligned_scores) return ASG_ERR_INVALID;
    if (state_bytes < asg_state_bytes(p)) return ASG_ERR_WORKSPACE;
    return ASG_DISPATCH(p,
        run_forward<float>(ctx, p, state, full_scores, aligned_scores, 15, true, flags, (hipStream_t) stream),
        run_forward<double>(ctx, p, state, full_scores, aligned_scores, 15, true, flags, (hipStream_t) stream));
}

int asg_forward_only(asg_ctx *ctx, const asg_problem *p, void *state, size_t state_bytes,
                     void *full_scores, void *aligned_scores, int flags, void *stream) {
    int rc = check_problem(p, true);
    if (rc) return rc;
    if (!full_scores || !aligned_scores) return ASG_ERR_INVALID;
    if (!small_full(p->N) || !small_aligned(p->S)) {
        if (!state) return ASG_ERR_INVALID;
        if (state_bytes < asg_state_bytes(p)) return ASG_ERR_WORKSPACE;
    } else {
        state = nullptr;
    }
    flags &= ~ASG_FLAG_ALPHA_SCORES;
    return ASG_DISPATCH(p,
        run_forward<float>(ctx, p, state, full_scores, aligned_scores, kFullBeta | kAlignedBeta, false, flags, (hipStream_t) stream),
        run_forward<double>(ctx, p, state, full_scores, aligned_scores, kFullBeta | kAlignedBeta, false, flags, (hipStream_t) stream));
}

size_t asg_viterbi_work_bytes(const asg_problem *p) {
    if (check_problem(p, true) != ASG_OK) return 0;
    return (size_t) p->B * (size_t) p->T * (size_t) ((p->S + 63) / 64) * sizeof(unsigned long long);
}

int asg_viterbi(asg_ctx *ctx, const asg_problem *p, void *work, size_t work_bytes, void *scores, int64_t *path,
                int flags, void *stream) {
    (void) ctx; (void) flags;
    int rc = check_problem(p, true);
    if (rc) return rc;
    if (!work || !scores || !path) return ASG_ERR_INVALID;
    if (work_bytes < asg_viterbi_work_bytes(p)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    return hip_status(ASG_DISPATCH(p, launch_viterbi_small<float>(P, work, scores, path, (hipStream_t) stream),
                                   launch_viterbi_small<double>(P, work, scores, path, (hipStream_t) stream)));
}

// Decoding reads no targets and keeps no lattice state: none of the loss's 32-bit-offset limits apply (every index into its
// workspace and outputs is 64-bit).  The one shape limit: the transpose grid of the streaming route (N / 64 <= 65536 per axis).
static int check_decode(const asg_problem *p) {
    if (!p) return ASG_ERR_INVALID;
    if (p->dtype != ASG_DTYPE_F32 && p->dtype != ASG_DTYPE_F64) return ASG_ERR_INVALID;
    if (p->inputs_dtype != 0)
        return (p->inputs_dtype == ASG_DTYPE_BF16 && p->dtype == ASG_DTYPE_F32) ? ASG_ERR_UNSUPPORTED : ASG_ERR_INVALID;
    if (p->T < 1 || p->B < 1 || p->N < 1) return ASG_ERR_INVALID;
    if (!p->inputs || !p->transition) return ASG_ERR_INVALID;
    if (p->T > (1 << 30) || p->B > (1 << 30) || p->N > (1 << 22)) return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

size_t asg_viterbi_decode_work_bytes(const asg_problem *p) {
    if (check_decode(p) != ASG_OK) return 0;
    return decode_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, (int) p->N);
}

int asg_viterbi_decode(asg_ctx *ctx, const asg_problem *p, void *work, size_t work_bytes, void *scores, int64_t *path,
                       int64_t *tokens, int64_t *token_lengths, int flags, void *stream) {
    (void) ctx; (void) flags;
    int rc = check_decode(p);
    if (rc) return rc;
    if (!work || !scores || !path || !tokens || !token_lengths) return ASG_ERR_INVALID;
    if (work_bytes < asg_viterbi_decode_work_bytes(p)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths;
    return hip_status(ASG_DISPATCH(p, launch_decode<float>(P, work, scores, pa, tk, tl, (hipStream_t) stream),
                                   launch_decode<double>(P, work, scores, pa, tk, tl, (hipStream_t) stream)));
}

static int check_decode_graph(const asg_problem *p, const asg_token_graph *g) {
    int rc = check_decode(p);
    if (rc) return rc;
    if (!g || g->dtype != p->dtype || g->N != p->N || g->Q < 0 || g->E < 0) return ASG_ERR_INVALID;
    if (g->Q >= (int64_t) 1 << 31 || g->E >= (int64_t) 1 << 31 || p->N > (1 << 16) || p->B > (1 << 22)) return ASG_ERR_UNSUPPORTED;
    if (g->Q > 0 && (!g->label || !g->state || !g->row || !g->start_w || !g->final_w)) return ASG_ERR_INVALID;
    if (g->E > 0 && (!g->src || !g->src_label || !g->edge_w)) return ASG_ERR_INVALID;
    return ASG_OK;
}

size_t asg_viterbi_decode_graph_work_bytes(const asg_problem *p, const asg_token_graph *g) {
    if (check_decode_graph(p, g) != ASG_OK) return 0;
    return graph_decode_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, (int) g->Q);
}

int asg_viterbi_decode_graph(asg_ctx *ctx, const asg_problem *p, const asg_token_graph *g, void *work, size_t work_bytes,
                             void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                             int flags, void *stream) {
    (void) ctx;
    int rc = check_decode_graph(p, g);
    if (rc) return rc;
    if (!work || !scores || !path || !tokens || !token_lengths || !states) return ASG_ERR_INVALID;
    if (work_bytes < asg_viterbi_decode_graph_work_bytes(p, g)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    GraphArgs G{};
    G.Q = (int) g->Q; G.E = (int) g->E;
    G.label = g->label; G.state = g->state; G.row = g->row; G.src = g->src; G.src_label = g->src_label;
    G.start_w = g->start_w; G.final_w = g->final_w; G.edge_w = g->edge_w;
    const int route = (flags & ASG_FLAG_DECODE_GRAPH_STREAMING) ? 1 : ((flags & ASG_FLAG_DECODE_GRAPH_RESIDENT) ? 2 : 0);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    return hip_status(ASG_DISPATCH(p, launch_decode_graph<float>(P, G, route, work, scores, pa, tk, tl, st, (hipStream_t) stream),
                                   launch_decode_graph<double>(P, G, route, work, scores, pa, tk, tl, st, (hipStream_t) stream)));
}

static int check_graph_loss(const asg_problem *p, const asg_token_graph_loss *gl) {
    if (!gl) return ASG_ERR_INVALID;
    int rc = check_decode_graph(p, gl->graph);
    if (rc) return rc;
    const asg_token_graph *g = gl->graph;
    if (gl->S < 1 || gl->start < 0 || gl->start >= gl->S) return ASG_ERR_INVALID;
    if (gl->S >= (int64_t) 1 << 31) return ASG_ERR_UNSUPPORTED;
    if (!gl->orow || !gl->lrow || !gl->next || !gl->arcw || !gl->finw) return ASG_ERR_INVALID;
    if (g->Q > 0 && !gl->lq) return ASG_ERR_INVALID;
    if (g->E > 0 && (!gl->tgt || !gl->oedge || !gl->pkey || !gl->pedge)) return ASG_ERR_INVALID;
    return ASG_OK;
}

static GraphArgs to_graph_args(const asg_token_graph *g) {
    GraphArgs G{};
    G.Q = (int) g->Q; G.E = (int) g->E;
    G.label = g->label; G.state = g->state; G.row = g->row; G.src = g->src; G.src_label = g->src_label;
    G.start_w = g->start_w; G.final_w = g->final_w; G.edge_w = g->edge_w;
    return G;
}

static int check_beam_graph(const asg_problem *p, const asg_token_graph_beam *gb, int beam_size) {
    if (!gb) return ASG_ERR_INVALID;
    int rc = check_decode_graph(p, gb->graph);
    if (rc) return rc;
    const asg_token_graph *g = gb->graph;
    if (beam_size < 1 || gb->num_start < 0 || gb->num_start > g->Q || gb->max_out < 0) return ASG_ERR_INVALID;
    if (g->Q > 0 && !gb->orow) return ASG_ERR_INVALID;
    if (g->E > 0 && (!gb->oarc || !gb->ow)) return ASG_ERR_INVALID;
    if (gb->num_start > 0 && !gb->start_q) return ASG_ERR_INVALID;
    if (beam_graph_k((int) g->Q, beam_size) > kBeamMaxK) return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

static BeamGraphArgs to_beam_graph_args(const asg_token_graph_beam *gb) {
    BeamGraphArgs BG{};
    BG.num_start = (int) gb->num_start; BG.max_out = gb->max_out;
    BG.orow = gb->orow; BG.oarc = gb->oarc; BG.ow = gb->ow; BG.start_q = gb->start_q;
    return BG;
}

size_t asg_beam_decode_graph_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, int beam_size) {
    if (check_beam_graph(p, gb, beam_size) != ASG_OK) return 0;
    const int Q = (int) gb->graph->Q, K = beam_graph_k(Q, beam_size);
    return beam_graph_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, Q, K,
                                 beam_graph_cap(Q, K, gb->max_out, (int) gb->num_start));
}

int asg_beam_decode_graph(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, int beam_size, double beam_threshold,
                          void *work, size_t work_bytes, void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                          int64_t *states, int flags, void *stream) {
    (void) ctx; (void) flags;
    int rc = check_beam_graph(p, gb, beam_size);
    if (rc) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!work || !scores || !path || !tokens || !token_lengths || !states) return ASG_ERR_INVALID;
    if (work_bytes < asg_beam_decode_graph_work_bytes(p, gb, beam_size)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    return hip_status(ASG_DISPATCH(p, launch_beam_graph<float>(P, G, BG, K, beam_threshold, work, scores, pa, tk, tl, st,
                                                               (hipStream_t) stream),
                                   launch_beam_graph<double>(P, G, BG, K, beam_threshold, work, scores, pa, tk, tl, st,
                                                             (hipStream_t) stream)));
}

static int check_beam_words(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size) {
    if (beam_size < 1) return ASG_ERR_INVALID;
    int rc = check_beam_graph(p, gb, 1);                       // the graph's own checks: its beam clamps to Q, this one does not
    if (rc) return rc;
    if (!lm || lm->dtype != p->dtype || lm->H < 1 || lm->A < 0 || lm->V < 1 || lm->S < 1) return ASG_ERR_INVALID;
    if (lm->start < 0 || lm->start >= lm->H || lm->separator < 0 || lm->separator >= p->N) return ASG_ERR_INVALID;
    if (!lm->row || !lm->backoff || !lm->bw || !lm->ew || !lm->word_of_state) return ASG_ERR_INVALID;
    if (lm->A > 0 && (!lm->word || !lm->next || !lm->lw)) return ASG_ERR_INVALID;
    if (beam_size > kBeamMaxK || lm->H > kBeamWordMaxIndex || gb->graph->Q > kBeamWordMaxIndex || lm->A >= (int64_t) 1 << 31)
        return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

static WordLmArgs to_word_lm_args(const asg_word_lm *lm) {
    WordLmArgs LM{};
    LM.H = (int) lm->H; LM.A = (int) lm->A; LM.start = lm->start; LM.sep = lm->separator;
    LM.row = lm->row; LM.word = lm->word; LM.next = lm->next; LM.backoff = lm->backoff; LM.word_of_state = lm->word_of_state;
    LM.lw = lm->lw; LM.bw = lm->bw; LM.ew = lm->ew;
    return LM;
}

size_t asg_beam_decode_words_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size) {
    if (check_beam_words(p, gb, lm, beam_size) != ASG_OK) return 0;
    return beam_word_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, beam_size,
                                beam_word_cap(beam_size, gb->max_out, (int) gb->num_start));
}

int asg_beam_decode_words(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size,
                          double beam_threshold, void *work, size_t work_bytes, void *scores, int64_t *path, int64_t *tokens,
                          int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths,
                          int flags, void *stream) {
    (void) ctx; (void) flags;
    int rc = check_beam_words(p, gb, lm, beam_size);
    if (rc) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!work || !scores || !path || !tokens || !token_lengths || !states || !lm_states || !words || !word_lengths)
        return ASG_ERR_INVALID;
    if (work_bytes < asg_beam_decode_words_work_bytes(p, gb, lm, beam_size)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *ls = (long long *) lm_states, *wd = (long long *) words, *wl = (long long *) word_lengths;
    return hip_status(ASG_DISPATCH(p, launch_beam_words<float>(P, G, BG, LM, beam_size, beam_threshold, work, scores, pa, tk, tl,
                                                               st, ls, wd, wl, (hipStream_t) stream),
                                   launch_beam_words<double>(P, G, BG, LM, beam_size, beam_threshold, work, scores, pa, tk, tl,
                                                             st, ls, wd, wl, (hipStream_t) stream)));
}

// The look-ahead of a (lexicon, LM) pair: its arrays, sized for that pair's S and H.
static int check_word_lookahead(int dtype, const asg_word_lm *lm, const asg_word_lookahead *la) {
    if (!la || la->dtype != dtype || la->S != lm->S || la->H != lm->H) return ASG_ERR_INVALID;
    if (la->A < 0 || la->A > lm->A || la->levels < 1 || la->levels > 31) return ASG_ERR_INVALID;
    if (la->A > 0 && ((int64_t) 1 << (la->levels - 1)) > la->A) return ASG_ERR_INVALID;      // a level no row can fill
    if (!la->rlo || !la->rhi || !la->la_state || !la->krow || !la->dense0) return ASG_ERR_INVALID;
    if (la->A > 0 && (!la->krank || !la->tab)) return ASG_ERR_INVALID;
    return ASG_OK;
}

static WordLookArgs to_word_look_args(const asg_word_lookahead *la) {
    WordLookArgs LA{};
    LA.A = (int) la->A; LA.levels = la->levels;
    LA.rlo = la->rlo; LA.rhi = la->rhi; LA.la_state = la->la_state; LA.krow = la->krow; LA.krank = la->krank; LA.tab = la->tab;
    LA.dense0 = la->dense0;
    return LA;
}

int asg_beam_decode_words_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                             const asg_word_lookahead *la, int beam_size, double beam_threshold, void *work, size_t work_bytes,
                             void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                             int64_t *lm_states, int64_t *words, int64_t *word_lengths, int flags, void *stream) {
    (void) ctx; (void) flags;
    int rc = check_beam_words(p, gb, lm, beam_size);
    if (rc) return rc;
    if ((rc = check_word_lookahead(p->dtype, lm, la)) != ASG_OK) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!work || !scores || !path || !tokens || !token_lengths || !states || !lm_states || !words || !word_lengths)
        return ASG_ERR_INVALID;
    if (work_bytes < asg_beam_decode_words_work_bytes(p, gb, lm, beam_size)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    const WordLookArgs LA = to_word_look_args(la);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *ls = (long long *) lm_states, *wd = (long long *) words, *wl = (long long *) word_lengths;
    return hip_status(ASG_DISPATCH(p, launch_beam_words_la<float>(P, G, BG, LM, LA, beam_size, beam_threshold, work, scores, pa, tk,
                                                                  tl, st, ls, wd, wl, (hipStream_t) stream),
                                   launch_beam_words_la<double>(P, G, BG, LM, LA, beam_size, beam_threshold, work, scores, pa, tk,
                                                                tl, st, ls, wd, wl, (hipStream_t) stream)));
}

static int check_beam_words_nbest(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size,
                                  int nbest) {
    int rc = check_beam_words(p, gb, lm, beam_size);
    if (rc) return rc;
    if (nbest < 1) return ASG_ERR_INVALID;
    if (nbest > kBeamMaxNbest) return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

size_t asg_beam_decode_words_nbest_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                              int beam_size, int nbest) {
    if (check_beam_words_nbest(p, gb, lm, beam_size, nbest) != ASG_OK) return 0;
    return beam_word_nbest_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, beam_size,
                                      beam_word_cap(beam_size, gb->max_out, (int) gb->num_start), nbest);
}

// asg_beam_decode_words_nbest with a look-ahead (`with_la`: la is checked as asg_beam_decode_words_la checks it, behind the LM) or
// without one.
static int beam_decode_words_nbest(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                   const asg_word_lookahead *la, bool with_la, int beam_size, double beam_threshold, int nbest,
                                   void *work, size_t work_bytes, void *scores, void *emission_scores, void *graph_scores,
                                   void *lm_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                                   int64_t *lm_states, int64_t *words, int64_t *word_lengths, int64_t *num_hyps, void *stream) {
    int rc = check_beam_words_nbest(p, gb, lm, beam_size, nbest);
    if (rc) return rc;
    if (with_la && (rc = check_word_lookahead(p->dtype, lm, la)) != ASG_OK) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!work || !scores || !emission_scores || !graph_scores || !lm_scores || !tokens || !token_lengths || !words ||
        !word_lengths || !num_hyps)
        return ASG_ERR_INVALID;
    if (work_bytes < asg_beam_decode_words_nbest_work_bytes(p, gb, lm, beam_size, nbest)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *ls = (long long *) lm_states, *wd = (long long *) words, *wl = (long long *) word_lengths;
    long long *nh = (long long *) num_hyps;
    if (with_la) {
        const WordLookArgs LA = to_word_look_args(la);
        return hip_status(ASG_DISPATCH(p, launch_beam_words_nbest_la<float>(P, G, BG, LM, LA, beam_size, beam_threshold, nbest, work,
                                                                            scores, emission_scores, graph_scores, lm_scores, pa, tk,
                                                                            tl, st, ls, wd, wl, nh, (hipStream_t) stream),
                                       launch_beam_words_nbest_la<double>(P, G, BG, LM, LA, beam_size, beam_threshold, nbest, work,
                                                                          scores, emission_scores, graph_scores, lm_scores, pa, tk,
                                                                          tl, st, ls, wd, wl, nh, (hipStream_t) stream)));
    }
    return hip_status(ASG_DISPATCH(p, launch_beam_words_nbest<float>(P, G, BG, LM, beam_size, beam_threshold, nbest, work, scores,
                                                                     emission_scores, graph_scores, lm_scores, pa, tk, tl, st, ls,
                                                                     wd, wl, nh, (hipStream_t) stream),
                                   launch_beam_words_nbest<double>(P, G, BG, LM, beam_size, beam_threshold, nbest, work, scores,
                                                                   emission_scores, graph_scores, lm_scores, pa, tk, tl, st, ls,
                                                                   wd, wl, nh, (hipStream_t) stream)));
}

int asg_beam_decode_words_nbest(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                int beam_size, double beam_threshold, int nbest, void *work, size_t work_bytes, void *scores,
                                void *emission_scores, void *graph_scores, void *lm_scores, int64_t *path, int64_t *tokens,
                                int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths,
                                int64_t *num_hyps, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_decode_words_nbest(p, gb, lm, nullptr, false, beam_size, beam_threshold, nbest, work, work_bytes, scores,
                                   emission_scores, graph_scores, lm_scores, path, tokens, token_lengths, states, lm_states, words,
                                   word_lengths, num_hyps, stream);
}

int asg_beam_decode_words_nbest_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                   const asg_word_lookahead *la, int beam_size, double beam_threshold, int nbest, void *work,
                                   size_t work_bytes, void *scores, void *emission_scores, void *graph_scores, void *lm_scores,
                                   int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states,
                                   int64_t *words, int64_t *word_lengths, int64_t *num_hyps, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_decode_words_nbest(p, gb, lm, la, true, beam_size, beam_threshold, nbest, work, work_bytes, scores, emission_scores,
                                   graph_scores, lm_scores, path, tokens, token_lengths, states, lm_states, words, word_lengths,
                                   num_hyps, stream);
}

static int check_beam_nbest(const asg_problem *p, const asg_token_graph_beam *gb, int beam_size, int nbest) {
    int rc = check_beam_graph(p, gb, beam_size);
    if (rc) return rc;
    if (nbest < 1) return ASG_ERR_INVALID;
    if (nbest > kBeamMaxNbest) return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

size_t asg_beam_decode_graph_nbest_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, int beam_size, int nbest) {
    if (check_beam_nbest(p, gb, beam_size, nbest) != ASG_OK) return 0;
    const int Q = (int) gb->graph->Q, K = beam_graph_k(Q, beam_size);
    return beam_nbest_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, Q, K,
                                 beam_graph_cap(Q, K, gb->max_out, (int) gb->num_start), nbest);
}

int asg_beam_decode_graph_nbest(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, int beam_size,
                                double beam_threshold, int nbest, void *work, size_t work_bytes, void *scores,
                                void *emission_scores, void *graph_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                                int64_t *states, int64_t *num_hyps, int flags, void *stream) {
    (void) ctx; (void) flags;
    int rc = check_beam_nbest(p, gb, beam_size, nbest);
    if (rc) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!work || !scores || !emission_scores || !graph_scores || !tokens || !token_lengths || !num_hyps) return ASG_ERR_INVALID;
    if (work_bytes < asg_beam_decode_graph_nbest_work_bytes(p, gb, beam_size, nbest)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *nh = (long long *) num_hyps;
    return hip_status(ASG_DISPATCH(p, launch_beam_nbest<float>(P, G, BG, K, beam_threshold, nbest, work, scores, emission_scores,
                                                               graph_scores, pa, tk, tl, st, nh, (hipStream_t) stream),
                                   launch_beam_nbest<double>(P, G, BG, K, beam_threshold, nbest, work, scores, emission_scores,
                                                             graph_scores, pa, tk, tl, st, nh, (hipStream_t) stream)));
}

// A stream state is sized like a problem of max_frames frames: the graph, B, the dtype and the beam are checked through a
// problem of that shape (its emissions are not read: any non-null pointer stands in for them).
static int check_beam_stream(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t max_frames) {
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    asg_problem q{};
    q.inputs = gb; q.transition = gb;
    q.T = max_frames; q.B = B; q.N = gb->graph->N; q.S = 1; q.dtype = dtype;
    return check_beam_graph(&q, gb, beam_size);
}

static size_t beam_stream_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t max_frames) {
    const int Q = (int) gb->graph->Q, K = beam_graph_k(Q, beam_size);
    return beam_stream_state_bytes(dtype == ASG_DTYPE_F64 ? 8 : 4, (int) max_frames, (int) B, Q, K,
                                   beam_graph_cap(Q, K, gb->max_out, (int) gb->num_start));
}

size_t asg_beam_stream_state_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t max_frames) {
    if (check_beam_stream(gb, B, dtype, beam_size, max_frames) != ASG_OK) return 0;
    return beam_stream_bytes(gb, B, dtype, beam_size, max_frames);
}

// ONE host path for the calls a growing token-graph stream has with a plain state (asg_beam_stream_*) and with a lattice-keeping
// one (asg_beam_conf_stream_*): reset, advance, result, n-best.  gl: the loss view a lattice-keeping state is checked and sized
// through (gb is its beam view), null for a plain state.  The kernels are the same; what differs is the state's checks, its
// bytes, the stride of a slot, and the advance kernel's keep policy.
static int check_beam_conf_stream(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size, int64_t max_frames);
static size_t beam_conf_stream_bytes(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size, int64_t max_frames);

static int check_stream_state(const asg_token_graph_beam *gb, const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size,
                              int64_t max_frames) {
    return gl ? check_beam_conf_stream(gl, B, dtype, beam_size, max_frames) : check_beam_stream(gb, B, dtype, beam_size, max_frames);
}

static size_t stream_state_bytes(const asg_token_graph_beam *gb, const asg_token_graph_beam_loss *gl, int64_t B, int dtype,
                                 int beam_size, int64_t max_frames) {
    return gl ? beam_conf_stream_bytes(gl, B, dtype, beam_size, max_frames) : beam_stream_bytes(gb, B, dtype, beam_size, max_frames);
}

// the stride of a slot for the launchers: 0 (their own layout's) for a plain state
static size_t stream_state_per(const asg_token_graph_beam_loss *gl, int dtype, int beam_size, int64_t max_frames) {
    return gl ? beam_conf_stream_bytes(gl, 1, dtype, beam_size, max_frames) : 0;
}

static int beam_stream_reset(const asg_token_graph_beam *gb, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size,
                             int64_t max_frames, void *state, size_t state_bytes, const uint8_t *mask, void *stream) {
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const int dtype = gb->graph->dtype;
    int rc = check_stream_state(gb, gl, B, dtype, beam_size, max_frames);
    if (rc) return rc;
    if (!state) return ASG_ERR_INVALID;
    if (state_bytes < stream_state_bytes(gb, gl, B, dtype, beam_size, max_frames)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(gb->graph);
    return hip_status(launch_beam_stream_reset(dtype == ASG_DTYPE_F64 ? 8 : 4, G, to_beam_graph_args(gb),
                                               beam_graph_k(G.Q, beam_size), (int) max_frames, (int) B, state, mask,
                                               (hipStream_t) stream, stream_state_per(gl, dtype, beam_size, max_frames)));
}

static int beam_stream_advance(const asg_problem *p, const asg_token_graph_beam *gb, const asg_token_graph_beam_loss *gl,
                               int beam_size, double beam_threshold, int64_t max_frames, void *state, size_t state_bytes,
                               void *stream) {
    if (!p) return ASG_ERR_INVALID;
    int rc = check_stream_state(gb, gl, p->B, p->dtype, beam_size, max_frames);
    if (rc) return rc;
    if (p->T < 0 || p->N != gb->graph->N) return ASG_ERR_INVALID;
    if (p->T > 0 && (rc = check_beam_graph(p, gb, beam_size)) != ASG_OK) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!state) return ASG_ERR_INVALID;
    if (state_bytes < stream_state_bytes(gb, gl, p->B, p->dtype, beam_size, max_frames)) return ASG_ERR_WORKSPACE;
    if (p->T == 0) return ASG_OK;                                          // no frame: the state stays as it is
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    return hip_status(ASG_DISPATCH(p, launch_beam_stream_advance<float>(P, G, BG, K, beam_threshold, (int) max_frames, state,
                                                                        (hipStream_t) stream, gl != nullptr),
                                   launch_beam_stream_advance<double>(P, G, BG, K, beam_threshold, (int) max_frames, state,
                                                                      (hipStream_t) stream, gl != nullptr)));
}

static int beam_stream_result(const asg_token_graph_beam *gb, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size,
                              int64_t max_frames, const void *state, size_t state_bytes, int final, void *scores, int64_t *path,
                              int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *frames, int64_t *status,
                              void *stream) {
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const asg_token_graph *g = gb->graph;
    int rc = check_stream_state(gb, gl, B, g->dtype, beam_size, max_frames);
    if (rc) return rc;
    if (!state || !scores || !path || !tokens || !token_lengths || !states || !frames || !status) return ASG_ERR_INVALID;
    if (state_bytes < stream_state_bytes(gb, gl, B, g->dtype, beam_size, max_frames)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    const size_t per = stream_state_per(gl, g->dtype, beam_size, max_frames);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *fr = (long long *) frames, *su = (long long *) status;
    return hip_status(ASG_DISPATCH(g, launch_beam_stream_result<float>(G, BG, K, (int) max_frames, (int) B, state, final, scores, pa,
                                                                       tk, tl, st, fr, su, (hipStream_t) stream, per),
                                   launch_beam_stream_result<double>(G, BG, K, (int) max_frames, (int) B, state, final, scores, pa,
                                                                     tk, tl, st, fr, su, (hipStream_t) stream, per)));
}

int asg_beam_stream_reset(asg_ctx *ctx, const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t max_frames, void *state,
                          size_t state_bytes, const uint8_t *mask, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_stream_reset(gb, nullptr, B, beam_size, max_frames, state, state_bytes, mask, stream);
}

int asg_beam_stream_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, int beam_size,
                            double beam_threshold, int64_t max_frames, void *state, size_t state_bytes, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_stream_advance(p, gb, nullptr, beam_size, beam_threshold, max_frames, state, state_bytes, stream);
}

int asg_beam_stream_result(asg_ctx *ctx, const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t max_frames,
                           const void *state, size_t state_bytes, int final, void *scores, int64_t *path, int64_t *tokens,
                           int64_t *token_lengths, int64_t *states, int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_stream_result(gb, nullptr, B, beam_size, max_frames, state, state_bytes, final, scores, path, tokens, token_lengths,
                              states, frames, status, stream);
}

// A word stream state is sized like a problem of max_frames frames, as a stream state is: the checks of asg_beam_decode_words
// through a problem of that shape (there is no clamp of the beam to Q).
static int check_beam_word_stream(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype, int beam_size,
                                  int64_t max_frames) {
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    asg_problem q{};
    q.inputs = gb; q.transition = gb;
    q.T = max_frames; q.B = B; q.N = gb->graph->N; q.S = 1; q.dtype = dtype;
    return check_beam_words(&q, gb, lm, beam_size);
}

static size_t beam_word_stream_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t max_frames) {
    return beam_word_stream_state_bytes(dtype == ASG_DTYPE_F64 ? 8 : 4, (int) max_frames, (int) B, beam_size,
                                        beam_word_cap(beam_size, gb->max_out, (int) gb->num_start));
}

size_t asg_beam_word_stream_state_bytes(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype, int beam_size,
                                        int64_t max_frames) {
    if (check_beam_word_stream(gb, lm, B, dtype, beam_size, max_frames) != ASG_OK) return 0;
    return beam_word_stream_bytes(gb, B, dtype, beam_size, max_frames);
}

// ONE host path for the calls a growing word stream has with a plain state (asg_beam_word_stream_*) and with a lattice-keeping
// one (asg_beam_word_conf_stream_*): reset, advance, result, n-best, each with a look-ahead or without.  `lattice` chooses the
// state's checks, its bytes, the stride of a slot and the advance kernel's keep policy; the kernels are the same.
static int check_beam_word_conf_stream(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype, int beam_size,
                                       int64_t max_frames);
static size_t beam_word_conf_stream_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t max_frames);

static int check_word_stream_state(const asg_token_graph_beam *gb, const asg_word_lm *lm, bool lattice, int64_t B, int dtype,
                                   int beam_size, int64_t max_frames) {
    return lattice ? check_beam_word_conf_stream(gb, lm, B, dtype, beam_size, max_frames)
                   : check_beam_word_stream(gb, lm, B, dtype, beam_size, max_frames);
}

static size_t word_stream_state_bytes(const asg_token_graph_beam *gb, bool lattice, int64_t B, int dtype, int beam_size,
                                      int64_t max_frames) {
    return lattice ? beam_word_conf_stream_bytes(gb, B, dtype, beam_size, max_frames)
                   : beam_word_stream_bytes(gb, B, dtype, beam_size, max_frames);
}

// the stride of a slot for the launchers: 0 (their own layout's) for a plain state
static size_t word_stream_state_per(const asg_token_graph_beam *gb, bool lattice, int dtype, int beam_size, int64_t max_frames) {
    return lattice ? beam_word_conf_stream_bytes(gb, 1, dtype, beam_size, max_frames) : 0;
}

static int beam_word_stream_reset(const asg_token_graph_beam *gb, const asg_word_lm *lm, bool lattice, int64_t B, int beam_size,
                                  int64_t max_frames, void *state, size_t state_bytes, const uint8_t *mask, void *stream) {
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const int dtype = gb->graph->dtype;
    int rc = check_word_stream_state(gb, lm, lattice, B, dtype, beam_size, max_frames);
    if (rc) return rc;
    if (!state) return ASG_ERR_INVALID;
    if (state_bytes < word_stream_state_bytes(gb, lattice, B, dtype, beam_size, max_frames)) return ASG_ERR_WORKSPACE;
    return hip_status(launch_beam_word_stream_reset(dtype == ASG_DTYPE_F64 ? 8 : 4, to_beam_graph_args(gb), beam_size,
                                                    (int) max_frames, (int) B, state, mask, (hipStream_t) stream,
                                                    word_stream_state_per(gb, lattice, dtype, beam_size, max_frames)));
}

int asg_beam_word_stream_reset(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                               int64_t max_frames, void *state, size_t state_bytes, const uint8_t *mask, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_reset(gb, lm, false, B, beam_size, max_frames, state, state_bytes, mask, stream);
}

// The four calls of the word streams that run the search or read its values, with a look-ahead (`with_la`: la is checked as
// asg_beam_decode_words_la checks it, behind the LM) or without one: asg_beam_word_{stream,window}_{advance,result}[_la].
static int beam_word_stream_advance(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                    const asg_word_lookahead *la, bool with_la, bool lattice, int beam_size, double beam_threshold,
                                    int64_t max_frames, void *state, size_t state_bytes, void *stream) {
    if (!p) return ASG_ERR_INVALID;
    int rc = check_word_stream_state(gb, lm, lattice, p->B, p->dtype, beam_size, max_frames);
    if (rc) return rc;
    if (with_la && (rc = check_word_lookahead(p->dtype, lm, la)) != ASG_OK) return rc;
    if (p->T < 0 || p->N != gb->graph->N) return ASG_ERR_INVALID;
    if (p->T > 0 && (rc = check_beam_words(p, gb, lm, beam_size)) != ASG_OK) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!state) return ASG_ERR_INVALID;
    if (state_bytes < word_stream_state_bytes(gb, lattice, p->B, p->dtype, beam_size, max_frames)) return ASG_ERR_WORKSPACE;
    if (p->T == 0) return ASG_OK;                                          // no frame: the state stays as it is
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    const WordLookArgs LA = with_la ? to_word_look_args(la) : WordLookArgs{};
    const WordLookArgs *look = with_la ? &LA : nullptr;
    return hip_status(ASG_DISPATCH(p, launch_beam_word_stream_advance<float>(P, G, BG, LM, look, beam_size, beam_threshold,
                                                                             (int) max_frames, state, (hipStream_t) stream, lattice),
                                   launch_beam_word_stream_advance<double>(P, G, BG, LM, look, beam_size, beam_threshold,
                                                                           (int) max_frames, state, (hipStream_t) stream, lattice)));
}

int asg_beam_word_stream_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                 int beam_size, double beam_threshold, int64_t max_frames, void *state, size_t state_bytes,
                                 int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_advance(p, gb, lm, nullptr, false, false, beam_size, beam_threshold, max_frames, state, state_bytes,
                                    stream);
}

int asg_beam_word_stream_advance_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                    const asg_word_lookahead *la, int beam_size, double beam_threshold, int64_t max_frames,
                                    void *state, size_t state_bytes, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_advance(p, gb, lm, la, true, false, beam_size, beam_threshold, max_frames, state, state_bytes, stream);
}

static int beam_word_stream_result(const asg_token_graph_beam *gb, const asg_word_lm *lm, const asg_word_lookahead *la, bool with_la,
                                   bool lattice, int64_t B, int beam_size, int64_t max_frames, const void *state, size_t state_bytes,
                                   int final,
                                   void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                                   int64_t *lm_states, int64_t *words, int64_t *word_lengths, int64_t *frames, int64_t *status,
                                   void *stream) {
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const asg_token_graph *g = gb->graph;
    int rc = check_word_stream_state(gb, lm, lattice, B, g->dtype, beam_size, max_frames);
    if (rc) return rc;
    if (with_la && (rc = check_word_lookahead(g->dtype, lm, la)) != ASG_OK) return rc;
    if (!state || !scores || !path || !tokens || !token_lengths || !states || !lm_states || !words || !word_lengths || !frames ||
        !status)
        return ASG_ERR_INVALID;
    if (state_bytes < word_stream_state_bytes(gb, lattice, B, g->dtype, beam_size, max_frames)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    const size_t per = word_stream_state_per(gb, lattice, g->dtype, beam_size, max_frames);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *ls = (long long *) lm_states, *wd = (long long *) words, *wl = (long long *) word_lengths;
    long long *fr = (long long *) frames, *su = (long long *) status;
    const WordLookArgs LA = with_la ? to_word_look_args(la) : WordLookArgs{};
    const WordLookArgs *look = with_la ? &LA : nullptr;
    return hip_status(ASG_DISPATCH(g, launch_beam_word_stream_result<float>(G, BG, LM, look, beam_size, (int) max_frames, (int) B,
                                                                            state, final, scores, pa, tk, tl, st, ls, wd, wl, fr,
                                                                            su, (hipStream_t) stream, per),
                                   launch_beam_word_stream_result<double>(G, BG, LM, look, beam_size, (int) max_frames, (int) B,
                                                                          state, final, scores, pa, tk, tl, st, ls, wd, wl, fr,
                                                                          su, (hipStream_t) stream, per)));
}

int asg_beam_word_stream_result(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                                int64_t max_frames, const void *state, size_t state_bytes, int final, void *scores, int64_t *path,
                                int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                int64_t *word_lengths, int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_result(gb, lm, nullptr, false, false, B, beam_size, max_frames, state, state_bytes, final, scores, path,
                                   tokens, token_lengths, states, lm_states, words, word_lengths, frames, status, stream);
}

int asg_beam_word_stream_result_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                   const asg_word_lookahead *la, int64_t B, int beam_size, int64_t max_frames, const void *state,
                                   size_t state_bytes, int final, void *scores, int64_t *path, int64_t *tokens,
                                   int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                   int64_t *word_lengths, int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_result(gb, lm, la, true, false, B, beam_size, max_frames, state, state_bytes, final, scores, path,
                                   tokens, token_lengths, states, lm_states, words, word_lengths, frames, status, stream);
}

static int check_beam_word_stream_nbest(const asg_token_graph_beam *gb, const asg_word_lm *lm, bool lattice, int64_t B, int dtype,
                                        int beam_size, int64_t max_frames, int nbest) {
    int rc = check_word_stream_state(gb, lm, lattice, B, dtype, beam_size, max_frames);
    if (rc) return rc;
    if (nbest < 1) return ASG_ERR_INVALID;
    if (nbest > kBeamMaxNbest) return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

size_t asg_beam_word_stream_nbest_work_bytes(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype,
                                             int beam_size, int64_t max_frames, int nbest) {
    if (check_beam_word_stream_nbest(gb, lm, false, B, dtype, beam_size, max_frames, nbest) != ASG_OK) return 0;
    return beam_word_stream_nbest_work_bytes((int) max_frames, (int) B, beam_size, nbest);
}

// asg_beam_word_stream_nbest with a look-ahead (`with_la`, checked behind the LM) or without one.
static int beam_word_stream_nbest(const asg_token_graph_beam *gb, const asg_word_lm *lm, const asg_word_lookahead *la, bool with_la,
                                  bool lattice, int64_t B, int beam_size, int64_t max_frames, const void *state, size_t state_bytes,
                                  int final,
                                  int nbest, void *work, size_t work_bytes, void *scores, void *graph_scores, void *lm_scores,
                                  int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states,
                                  int64_t *words, int64_t *word_lengths, int64_t *num_hyps, int64_t *frames, int64_t *status,
                                  void *stream) {
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const asg_token_graph *g = gb->graph;
    int rc = check_beam_word_stream_nbest(gb, lm, lattice, B, g->dtype, beam_size, max_frames, nbest);
    if (rc) return rc;
    if (with_la && (rc = check_word_lookahead(g->dtype, lm, la)) != ASG_OK) return rc;
    if (!state || !work || !scores || !graph_scores || !lm_scores || !tokens || !token_lengths || !words || !word_lengths ||
        !num_hyps || !frames || !status)
        return ASG_ERR_INVALID;
    if (state_bytes < word_stream_state_bytes(gb, lattice, B, g->dtype, beam_size, max_frames)) return ASG_ERR_WORKSPACE;
    if (work_bytes < beam_word_stream_nbest_work_bytes((int) max_frames, (int) B, beam_size, nbest)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    const size_t per = word_stream_state_per(gb, lattice, g->dtype, beam_size, max_frames);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *ls = (long long *) lm_states, *wd = (long long *) words, *wl = (long long *) word_lengths;
    long long *nh = (long long *) num_hyps, *fr = (long long *) frames, *su = (long long *) status;
    if (with_la) {
        const WordLookArgs LA = to_word_look_args(la);
        return hip_status(ASG_DISPATCH(g, launch_beam_word_stream_nbest_la<float>(G, BG, LM, LA, beam_size, (int) max_frames, (int) B,
                                                                                  state, final, nbest, work, scores, graph_scores,
                                                                                  lm_scores, pa, tk, tl, st, ls, wd, wl, nh, fr, su,
                                                                                  (hipStream_t) stream, per),
                                       launch_beam_word_stream_nbest_la<double>(G, BG, LM, LA, beam_size, (int) max_frames, (int) B,
                                                                                state, final, nbest, work, scores, graph_scores,
                                                                                lm_scores, pa, tk, tl, st, ls, wd, wl, nh, fr, su,
                                                                                (hipStream_t) stream, per)));
    }
    return hip_status(ASG_DISPATCH(g, launch_beam_word_stream_nbest<float>(G, BG, LM, beam_size, (int) max_frames, (int) B, state,
                                                                           final, nbest, work, scores, graph_scores, lm_scores, pa,
                                                                           tk, tl, st, ls, wd, wl, nh, fr, su, (hipStream_t) stream,
                                                                           per),
                                   launch_beam_word_stream_nbest<double>(G, BG, LM, beam_size, (int) max_frames, (int) B, state,
                                                                         final, nbest, work, scores, graph_scores, lm_scores, pa,
                                                                         tk, tl, st, ls, wd, wl, nh, fr, su, (hipStream_t) stream,
                                                                         per)));
}

int asg_beam_word_stream_nbest(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                               int64_t max_frames, const void *state, size_t state_bytes, int final, int nbest, void *work,
                               size_t work_bytes, void *scores, void *graph_scores, void *lm_scores, int64_t *path, int64_t *tokens,
                               int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths,
                               int64_t *num_hyps, int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_nbest(gb, lm, nullptr, false, false, B, beam_size, max_frames, state, state_bytes, final, nbest, work,
                                  work_bytes, scores, graph_scores, lm_scores, path, tokens, token_lengths, states, lm_states, words,
                                  word_lengths, num_hyps, frames, status, stream);
}

int asg_beam_word_stream_nbest_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                  const asg_word_lookahead *la, int64_t B, int beam_size, int64_t max_frames, const void *state,
                                  size_t state_bytes, int final, int nbest, void *work, size_t work_bytes, void *scores,
                                  void *graph_scores, void *lm_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                                  int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths, int64_t *num_hyps,
                                  int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_nbest(gb, lm, la, true, false, B, beam_size, max_frames, state, state_bytes, final, nbest, work,
                                  work_bytes, scores, graph_scores, lm_scores, path, tokens, token_lengths, states, lm_states, words,
                                  word_lengths, num_hyps, frames, status, stream);
}

// A window stream state is sized like a problem of W frames (the ring); P is the commit period.
static int check_beam_window(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t W, int64_t P) {
    if (W < 1 || P < 1 || P > W) return ASG_ERR_INVALID;
    return check_beam_stream(gb, B, dtype, beam_size, W);
}

static size_t beam_window_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t W) {
    const int Q = (int) gb->graph->Q, K = beam_graph_k(Q, beam_size);
    return beam_window_state_bytes(dtype == ASG_DTYPE_F64 ? 8 : 4, (int) W, (int) B, Q, K,
                                   beam_graph_cap(Q, K, gb->max_out, (int) gb->num_start));
}

size_t asg_beam_window_state_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t W, int64_t P) {
    if (check_beam_window(gb, B, dtype, beam_size, W, P) != ASG_OK) return 0;
    return beam_window_bytes(gb, B, dtype, beam_size, W);
}

int asg_beam_window_reset(asg_ctx *ctx, const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t W, int64_t P, void *state,
                          size_t state_bytes, const uint8_t *mask, int flags, void *stream) {
    (void) ctx; (void) flags;
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const int dtype = gb->graph->dtype;
    int rc = check_beam_window(gb, B, dtype, beam_size, W, P);
    if (rc) return rc;
    if (!state) return ASG_ERR_INVALID;
    if (state_bytes < beam_window_bytes(gb, B, dtype, beam_size, W)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(gb->graph);
    return hip_status(launch_beam_window_reset(dtype == ASG_DTYPE_F64 ? 8 : 4, G, to_beam_graph_args(gb),
                                               beam_graph_k(G.Q, beam_size), (int) W, (int) B, state, mask, (hipStream_t) stream));
}

int asg_beam_window_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, int beam_size,
                            double beam_threshold, int64_t W, int64_t P, void *state, size_t state_bytes, int64_t *new_path,
                            int64_t *new_states, int64_t *new_tokens, int64_t *new_frames, int64_t *new_token_lengths, int flags,
                            void *stream) {
    (void) ctx; (void) flags;
    if (!p) return ASG_ERR_INVALID;
    int rc = check_beam_window(gb, p->B, p->dtype, beam_size, W, P);
    if (rc) return rc;
    if (p->T < 0 || p->N != gb->graph->N) return ASG_ERR_INVALID;
    if (p->T > 0 && (rc = check_beam_graph(p, gb, beam_size)) != ASG_OK) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!state || !new_path || !new_states || !new_tokens || !new_frames || !new_token_lengths) return ASG_ERR_INVALID;
    if (state_bytes < beam_window_bytes(gb, p->B, p->dtype, beam_size, W)) return ASG_ERR_WORKSPACE;
    const Problem Pr = to_problem(p);                                      // (no frame: the launch still writes the empty outputs)
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    long long *np = (long long *) new_path, *ns = (long long *) new_states, *nt = (long long *) new_tokens;
    long long *nf = (long long *) new_frames, *nl = (long long *) new_token_lengths;
    return hip_status(ASG_DISPATCH(p, launch_beam_window_advance<float>(Pr, G, BG, K, beam_threshold, (int) W, (int) P, state, np, ns,
                                                                        nt, nf, nl, (hipStream_t) stream),
                                   launch_beam_window_advance<double>(Pr, G, BG, K, beam_threshold, (int) W, (int) P, state, np, ns,
                                                                      nt, nf, nl, (hipStream_t) stream)));
}

int asg_beam_window_result(asg_ctx *ctx, const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t W, int64_t P,
                           const void *state, size_t state_bytes, int final, void *scores, int64_t *path, int64_t *tokens,
                           int64_t *token_lengths, int64_t *states, int64_t *frames, int64_t *committed, int64_t *status, int flags,
                           void *stream) {
    (void) ctx; (void) flags;
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const asg_token_graph *g = gb->graph;
    int rc = check_beam_window(gb, B, g->dtype, beam_size, W, P);
    if (rc) return rc;
    if (!state || !scores || !path || !tokens || !token_lengths || !states || !frames || !committed || !status)
        return ASG_ERR_INVALID;
    if (state_bytes < beam_window_bytes(gb, B, g->dtype, beam_size, W)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *fr = (long long *) frames, *co = (long long *) committed, *su = (long long *) status;
    return hip_status(ASG_DISPATCH(g, launch_beam_window_result<float>(G, BG, K, (int) W, (int) B, state, final, scores, pa, tk, tl,
                                                                       st, fr, co, su, (hipStream_t) stream),
                                   launch_beam_window_result<double>(G, BG, K, (int) W, (int) B, state, final, scores, pa, tk, tl,
                                                                     st, fr, co, su, (hipStream_t) stream)));
}

// The n best of the token-graph streams: the checks of the corresponding _result call, then nbest.
static int check_beam_stream_nbest(const asg_token_graph_beam *gb, const asg_token_graph_beam_loss *gl, int64_t B, int dtype,
                                   int beam_size, int64_t max_frames, int nbest) {
    int rc = check_stream_state(gb, gl, B, dtype, beam_size, max_frames);
    if (rc) return rc;
    if (nbest < 1) return ASG_ERR_INVALID;
    if (nbest > kBeamMaxNbest) return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

static size_t beam_stream_nbest_bytes(const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t rows, int nbest) {
    return beam_stream_nbest_work_bytes((int) rows, (int) B, beam_graph_k((int) gb->graph->Q, beam_size), nbest);
}

size_t asg_beam_stream_nbest_work_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t max_frames,
                                        int nbest) {
    if (check_beam_stream_nbest(gb, nullptr, B, dtype, beam_size, max_frames, nbest) != ASG_OK) return 0;
    return beam_stream_nbest_bytes(gb, B, beam_size, max_frames, nbest);
}

// gl: as for beam_stream_result
static int beam_stream_nbest(const asg_token_graph_beam *gb, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size,
                             int64_t max_frames, const void *state, size_t state_bytes, int final, int nbest, void *work,
                             size_t work_bytes, void *scores, void *graph_scores, int64_t *path, int64_t *tokens,
                             int64_t *token_lengths, int64_t *states, int64_t *num_hyps, int64_t *frames, int64_t *status,
                             void *stream) {
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const asg_token_graph *g = gb->graph;
    int rc = check_beam_stream_nbest(gb, gl, B, g->dtype, beam_size, max_frames, nbest);
    if (rc) return rc;
    if (!state || !work || !scores || !graph_scores || !tokens || !token_lengths || !num_hyps || !frames || !status)
        return ASG_ERR_INVALID;
    if (state_bytes < stream_state_bytes(gb, gl, B, g->dtype, beam_size, max_frames)) return ASG_ERR_WORKSPACE;
    if (work_bytes < beam_stream_nbest_bytes(gb, B, beam_size, max_frames, nbest)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    const size_t per = stream_state_per(gl, g->dtype, beam_size, max_frames);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *nh = (long long *) num_hyps, *fr = (long long *) frames, *su = (long long *) status;
    return hip_status(ASG_DISPATCH(g, launch_beam_stream_nbest<float>(G, BG, K, (int) max_frames, (int) B, state, final, nbest, work,
                                                                      scores, graph_scores, pa, tk, tl, st, nh, fr, su,
                                                                      (hipStream_t) stream, per),
                                   launch_beam_stream_nbest<double>(G, BG, K, (int) max_frames, (int) B, state, final, nbest, work,
                                                                    scores, graph_scores, pa, tk, tl, st, nh, fr, su,
                                                                    (hipStream_t) stream, per)));
}

int asg_beam_stream_nbest(asg_ctx *ctx, const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t max_frames,
                          const void *state, size_t state_bytes, int final, int nbest, void *work, size_t work_bytes, void *scores,
                          void *graph_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                          int64_t *num_hyps, int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_stream_nbest(gb, nullptr, B, beam_size, max_frames, state, state_bytes, final, nbest, work, work_bytes, scores,
                             graph_scores, path, tokens, token_lengths, states, num_hyps, frames, status, stream);
}

static int check_beam_window_nbest(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t W, int64_t P,
                                   int nbest) {
    int rc = check_beam_window(gb, B, dtype, beam_size, W, P);
    if (rc) return rc;
    if (nbest < 1) return ASG_ERR_INVALID;
    if (nbest > kBeamMaxNbest) return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

size_t asg_beam_window_nbest_work_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t W, int64_t P,
                                        int nbest) {
    if (check_beam_window_nbest(gb, B, dtype, beam_size, W, P, nbest) != ASG_OK) return 0;
    return beam_stream_nbest_bytes(gb, B, beam_size, W, nbest);
}

int asg_beam_window_nbest(asg_ctx *ctx, const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t W, int64_t P,
                          const void *state, size_t state_bytes, int final, int nbest, void *work, size_t work_bytes, void *scores,
                          int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *num_hyps,
                          int64_t *frames, int64_t *committed, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const asg_token_graph *g = gb->graph;
    int rc = check_beam_window_nbest(gb, B, g->dtype, beam_size, W, P, nbest);
    if (rc) return rc;
    if (!state || !work || !scores || !tokens || !token_lengths || !num_hyps || !frames || !committed || !status)
        return ASG_ERR_INVALID;
    if (state_bytes < beam_window_bytes(gb, B, g->dtype, beam_size, W)) return ASG_ERR_WORKSPACE;
    if (work_bytes < beam_stream_nbest_bytes(gb, B, beam_size, W, nbest)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *nh = (long long *) num_hyps, *fr = (long long *) frames, *co = (long long *) committed, *su = (long long *) status;
    return hip_status(ASG_DISPATCH(g, launch_beam_window_nbest<float>(G, BG, K, (int) W, (int) B, state, final, nbest, work, scores,
                                                                      pa, tk, tl, st, nh, fr, co, su, (hipStream_t) stream),
                                   launch_beam_window_nbest<double>(G, BG, K, (int) W, (int) B, state, final, nbest, work, scores,
                                                                    pa, tk, tl, st, nh, fr, co, su, (hipStream_t) stream)));
}

// A word window stream state is sized like a word stream of W frames (the rings); P is the commit period.
static int check_beam_word_window(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype, int beam_size,
                                  int64_t W, int64_t P) {
    if (W < 1 || P < 1 || P > W) return ASG_ERR_INVALID;
    return check_beam_word_stream(gb, lm, B, dtype, beam_size, W);
}

static size_t beam_word_window_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t W) {
    return beam_word_window_state_bytes(dtype == ASG_DTYPE_F64 ? 8 : 4, (int) W, (int) B, beam_size,
                                        beam_word_cap(beam_size, gb->max_out, (int) gb->num_start));
}

// The number of automaton states word_of_state is indexed by, as the kernels clamp to it.
static int word_lm_states(const asg_word_lm *lm) { return lm->S < ((int64_t) 1 << 31) - 1 ? (int) lm->S : (1 << 31) - 1; }

size_t asg_beam_word_window_state_bytes(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype, int beam_size,
                                        int64_t W, int64_t P) {
    if (check_beam_word_window(gb, lm, B, dtype, beam_size, W, P) != ASG_OK) return 0;
    return beam_word_window_bytes(gb, B, dtype, beam_size, W);
}

int asg_beam_word_window_reset(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                               int64_t W, int64_t P, void *state, size_t state_bytes, const uint8_t *mask, int flags, void *stream) {
    (void) ctx; (void) flags;
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const int dtype = gb->graph->dtype;
    int rc = check_beam_word_window(gb, lm, B, dtype, beam_size, W, P);
    if (rc) return rc;
    if (!state) return ASG_ERR_INVALID;
    if (state_bytes < beam_word_window_bytes(gb, B, dtype, beam_size, W)) return ASG_ERR_WORKSPACE;
    return hip_status(launch_beam_word_window_reset(dtype == ASG_DTYPE_F64 ? 8 : 4, to_beam_graph_args(gb), beam_size, (int) W,
                                                    (int) B, state, mask, (hipStream_t) stream));
}

static int beam_word_window_advance(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                    const asg_word_lookahead *la, bool with_la, int beam_size, double beam_threshold, int64_t W,
                                    int64_t P, void *state, size_t state_bytes, int64_t *new_path, int64_t *new_states,
                                    int64_t *new_lm_states, int64_t *new_tokens, int64_t *new_words, int64_t *new_frames,
                                    int64_t *new_token_lengths, int64_t *new_word_lengths, void *stream) {
    if (!p) return ASG_ERR_INVALID;
    int rc = check_beam_word_window(gb, lm, p->B, p->dtype, beam_size, W, P);
    if (rc) return rc;
    if (with_la && (rc = check_word_lookahead(p->dtype, lm, la)) != ASG_OK) return rc;
    if (p->T < 0 || p->N != gb->graph->N) return ASG_ERR_INVALID;
    if (p->T > 0 && (rc = check_beam_words(p, gb, lm, beam_size)) != ASG_OK) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!state || !new_path || !new_states || !new_lm_states || !new_tokens || !new_words || !new_frames || !new_token_lengths ||
        !new_word_lengths)
        return ASG_ERR_INVALID;
    if (state_bytes < beam_word_window_bytes(gb, p->B, p->dtype, beam_size, W)) return ASG_ERR_WORKSPACE;
    const Problem Pr = to_problem(p);                                      // (no frame: the launch still writes the empty outputs)
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    const int S = word_lm_states(lm);
    long long *np = (long long *) new_path, *ns = (long long *) new_states, *nl = (long long *) new_lm_states;
    long long *nt = (long long *) new_tokens, *nw = (long long *) new_words, *nf = (long long *) new_frames;
    long long *tl = (long long *) new_token_lengths, *wl = (long long *) new_word_lengths;
    const WordLookArgs LA = with_la ? to_word_look_args(la) : WordLookArgs{};
    const WordLookArgs *look = with_la ? &LA : nullptr;
    return hip_status(ASG_DISPATCH(p, launch_beam_word_window_advance<float>(Pr, G, BG, LM, look, S, beam_size, beam_threshold,
                                                                             (int) W, (int) P, state, np, ns, nl, nt, nw, nf, tl,
                                                                             wl, (hipStream_t) stream),
                                   launch_beam_word_window_advance<double>(Pr, G, BG, LM, look, S, beam_size, beam_threshold,
                                                                           (int) W, (int) P, state, np, ns, nl, nt, nw, nf, tl,
                                                                           wl, (hipStream_t) stream)));
}

int asg_beam_word_window_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                 int beam_size, double beam_threshold, int64_t W, int64_t P, void *state, size_t state_bytes,
                                 int64_t *new_path, int64_t *new_states, int64_t *new_lm_states, int64_t *new_tokens,
                                 int64_t *new_words, int64_t *new_frames, int64_t *new_token_lengths, int64_t *new_word_lengths,
                                 int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_window_advance(p, gb, lm, nullptr, false, beam_size, beam_threshold, W, P, state, state_bytes, new_path,
                                    new_states, new_lm_states, new_tokens, new_words, new_frames, new_token_lengths,
                                    new_word_lengths, stream);
}

int asg_beam_word_window_advance_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                    const asg_word_lookahead *la, int beam_size, double beam_threshold, int64_t W, int64_t P,
                                    void *state, size_t state_bytes, int64_t *new_path, int64_t *new_states,
                                    int64_t *new_lm_states, int64_t *new_tokens, int64_t *new_words, int64_t *new_frames,
                                    int64_t *new_token_lengths, int64_t *new_word_lengths, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_window_advance(p, gb, lm, la, true, beam_size, beam_threshold, W, P, state, state_bytes, new_path, new_states,
                                    new_lm_states, new_tokens, new_words, new_frames, new_token_lengths, new_word_lengths, stream);
}

static int beam_word_window_result(const asg_token_graph_beam *gb, const asg_word_lm *lm, const asg_word_lookahead *la, bool with_la,
                                   int64_t B, int beam_size, int64_t W, int64_t P, const void *state, size_t state_bytes, int final,
                                   void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                                   int64_t *lm_states, int64_t *words, int64_t *word_lengths, int64_t *frames, int64_t *committed,
                                   int64_t *status, void *stream) {
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const asg_token_graph *g = gb->graph;
    int rc = check_beam_word_window(gb, lm, B, g->dtype, beam_size, W, P);
    if (rc) return rc;
    if (with_la && (rc = check_word_lookahead(g->dtype, lm, la)) != ASG_OK) return rc;
    if (!state || !scores || !path || !tokens || !token_lengths || !states || !lm_states || !words || !word_lengths || !frames ||
        !committed || !status)
        return ASG_ERR_INVALID;
    if (state_bytes < beam_word_window_bytes(gb, B, g->dtype, beam_size, W)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    const int S = word_lm_states(lm);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *ls = (long long *) lm_states, *wd = (long long *) words, *wl = (long long *) word_lengths;
    long long *fr = (long long *) frames, *co = (long long *) committed, *su = (long long *) status;
    const WordLookArgs LA = with_la ? to_word_look_args(la) : WordLookArgs{};
    const WordLookArgs *look = with_la ? &LA : nullptr;
    return hip_status(ASG_DISPATCH(g, launch_beam_word_window_result<float>(G, BG, LM, look, S, beam_size, (int) W, (int) B, state,
                                                                            final, scores, pa, tk, tl, st, ls, wd, wl, fr, co, su,
                                                                            (hipStream_t) stream),
                                   launch_beam_word_window_result<double>(G, BG, LM, look, S, beam_size, (int) W, (int) B, state,
                                                                          final, scores, pa, tk, tl, st, ls, wd, wl, fr, co, su,
                                                                          (hipStream_t) stream)));
}

int asg_beam_word_window_result(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                                int64_t W, int64_t P, const void *state, size_t state_bytes, int final, void *scores, int64_t *path,
                                int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                int64_t *word_lengths, int64_t *frames, int64_t *committed, int64_t *status, int flags,
                                void *stream) {
    (void) ctx; (void) flags;
    return beam_word_window_result(gb, lm, nullptr, false, B, beam_size, W, P, state, state_bytes, final, scores, path, tokens,
                                   token_lengths, states, lm_states, words, word_lengths, frames, committed, status, stream);
}

int asg_beam_word_window_result_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                   const asg_word_lookahead *la, int64_t B, int beam_size, int64_t W, int64_t P, const void *state,
                                   size_t state_bytes, int final, void *scores, int64_t *path, int64_t *tokens,
                                   int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                   int64_t *word_lengths, int64_t *frames, int64_t *committed, int64_t *status, int flags,
                                   void *stream) {
    (void) ctx; (void) flags;
    return beam_word_window_result(gb, lm, la, true, B, beam_size, W, P, state, state_bytes, final, scores, path, tokens,
                                   token_lengths, states, lm_states, words, word_lengths, frames, committed, status, stream);
}

static int check_beam_word_window_nbest(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype, int beam_size,
                                        int64_t W, int64_t P, int nbest) {
    int rc = check_beam_word_window(gb, lm, B, dtype, beam_size, W, P);
    if (rc) return rc;
    if (nbest < 1) return ASG_ERR_INVALID;
    if (nbest > kBeamMaxNbest) return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

size_t asg_beam_word_window_nbest_work_bytes(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype,
                                             int beam_size, int64_t W, int64_t P, int nbest) {
    if (check_beam_word_window_nbest(gb, lm, B, dtype, beam_size, W, P, nbest) != ASG_OK) return 0;
    return beam_word_window_nbest_work_bytes((int) W, (int) B, beam_size, nbest);
}

// asg_beam_word_window_nbest with a look-ahead (`with_la`, checked behind the LM) or without one.
static int beam_word_window_nbest(const asg_token_graph_beam *gb, const asg_word_lm *lm, const asg_word_lookahead *la, bool with_la,
                                  int64_t B, int beam_size, int64_t W, int64_t P, const void *state, size_t state_bytes, int final,
                                  int nbest, void *work, size_t work_bytes, void *scores, int64_t *path, int64_t *tokens,
                                  int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                  int64_t *word_lengths, int64_t *num_hyps, int64_t *frames, int64_t *committed, int64_t *status,
                                  void *stream) {
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const asg_token_graph *g = gb->graph;
    int rc = check_beam_word_window_nbest(gb, lm, B, g->dtype, beam_size, W, P, nbest);
    if (rc) return rc;
    if (with_la && (rc = check_word_lookahead(g->dtype, lm, la)) != ASG_OK) return rc;
    if (!state || !work || !scores || !tokens || !token_lengths || !words || !word_lengths || !num_hyps || !frames || !committed ||
        !status)
        return ASG_ERR_INVALID;
    if (state_bytes < beam_word_window_bytes(gb, B, g->dtype, beam_size, W)) return ASG_ERR_WORKSPACE;
    if (work_bytes < beam_word_window_nbest_work_bytes((int) W, (int) B, beam_size, nbest)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    const int S = word_lm_states(lm);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *ls = (long long *) lm_states, *wd = (long long *) words, *wl = (long long *) word_lengths;
    long long *nh = (long long *) num_hyps, *fr = (long long *) frames, *co = (long long *) committed, *su = (long long *) status;
    const WordLookArgs LA = with_la ? to_word_look_args(la) : WordLookArgs{};
    const WordLookArgs *look = with_la ? &LA : nullptr;
    return hip_status(ASG_DISPATCH(g, launch_beam_word_window_nbest<float>(G, BG, LM, look, S, beam_size, (int) W, (int) B, state,
                                                                           final, nbest, work, scores, pa, tk, tl, st, ls, wd, wl,
                                                                           nh, fr, co, su, (hipStream_t) stream),
                                   launch_beam_word_window_nbest<double>(G, BG, LM, look, S, beam_size, (int) W, (int) B, state,
                                                                         final, nbest, work, scores, pa, tk, tl, st, ls, wd, wl,
                                                                         nh, fr, co, su, (hipStream_t) stream)));
}

int asg_beam_word_window_nbest(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                               int64_t W, int64_t P, const void *state, size_t state_bytes, int final, int nbest, void *work,
                               size_t work_bytes, void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                               int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths, int64_t *num_hyps,
                               int64_t *frames, int64_t *committed, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_window_nbest(gb, lm, nullptr, false, B, beam_size, W, P, state, state_bytes, final, nbest, work, work_bytes,
                                  scores, path, tokens, token_lengths, states, lm_states, words, word_lengths, num_hyps, frames,
                                  committed, status, stream);
}

int asg_beam_word_window_nbest_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                  const asg_word_lookahead *la, int64_t B, int beam_size, int64_t W, int64_t P, const void *state,
                                  size_t state_bytes, int final, int nbest, void *work, size_t work_bytes, void *scores,
                                  int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states,
                                  int64_t *words, int64_t *word_lengths, int64_t *num_hyps, int64_t *frames, int64_t *committed,
                                  int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_window_nbest(gb, lm, la, true, B, beam_size, W, P, state, state_bytes, final, nbest, work, work_bytes, scores,
                                  path, tokens, token_lengths, states, lm_states, words, word_lengths, num_hyps, frames, committed,
                                  status, stream);
}

// What the two beam-pruned losses check alike behind their search's own checks: the targets, the limits of the lattice pass and
// whether a frame's set of M = K + nf members fits the family's kernels.
static int check_lattice(const asg_problem *p, int K, bool (*fits)(int, int, int)) {
    if (p->targets && p->S < 1) return ASG_ERR_INVALID;
    if (p->N > kBeamLossMaxN || p->T > (1 << 20)) return ASG_ERR_UNSUPPORTED;
    const int64_t nf = p->targets ? (p->S < p->T ? p->S : p->T) : 0;
    if (nf > kBeamLossMaxForced) return ASG_ERR_UNSUPPORTED;
    if (!fits(p->dtype == ASG_DTYPE_F64 ? 8 : 4, K + (int) nf, (int) p->N)) return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

// The two *_full_backward entry points: rc is the family's check (the two sizes are 0 when it fails), then the buffers, their
// sizes, the flag, and `launch` (const Problem &, bool accumulate, element type tag) on the dtype of the problem.
extern "C++" template <typename Launch>
static int lattice_full_backward(const asg_problem *p, int rc, size_t work_need, size_t scratch_need, const void *work,
                                 size_t work_bytes, const void *scores, const void *grad_scores, void *grad_inputs,
                                 void *grad_transition, void *scratch, size_t scratch_bytes, int flags, Launch launch) {
    if (rc) return rc;
    if (!work || !scores || !grad_scores || !grad_inputs || !grad_transition || !scratch) return ASG_ERR_INVALID;
    if (work_bytes < work_need || scratch_bytes < scratch_need) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const bool acc = (flags & ASG_FLAG_BEAM_LOSS_ACCUMULATE) != 0;
    return hip_status(ASG_DISPATCH(p, launch(P, acc, float()), launch(P, acc, double())));
}

static int check_beam_loss(const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size) {
    if (!gl) return ASG_ERR_INVALID;
    int rc = check_beam_graph(p, gl->beam, beam_size);
    if (rc) return rc;
    if (gl->S < 1 || gl->start < 0 || gl->start >= gl->S || !gl->next) return ASG_ERR_INVALID;
    if (gl->S >= (int64_t) 1 << 31) return ASG_ERR_UNSUPPORTED;
    return check_lattice(p, beam_graph_k((int) gl->beam->graph->Q, beam_size), beam_loss_fits);
}

static int beam_loss_nf(const asg_problem *p) { return p->targets ? (int) (p->S < p->T ? p->S : p->T) : 0; }

size_t asg_beam_graph_full_work_bytes(const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size, int store) {
    if (check_beam_loss(p, gl, beam_size) != ASG_OK) return 0;
    const asg_token_graph_beam *gb = gl->beam;
    const int Q = (int) gb->graph->Q, K = beam_graph_k(Q, beam_size);
    return beam_loss_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, Q, K,
                                beam_graph_cap(Q, K, gb->max_out, (int) gb->num_start), beam_loss_nf(p), store != 0);
}

size_t asg_beam_graph_full_scratch_bytes(const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size) {
    if (check_beam_loss(p, gl, beam_size) != ASG_OK) return 0;
    const int K = beam_graph_k((int) gl->beam->graph->Q, beam_size);
    return (size_t) p->B * beam_loss_scratch_per(p->dtype == ASG_DTYPE_F64 ? 8 : 4, K + beam_loss_nf(p), (int) p->N);
}

int asg_beam_graph_full_forward(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                                double beam_threshold, void *work, size_t work_bytes, void *scores, int flags, void *stream) {
    (void) ctx;
    int rc = check_beam_loss(p, gl, beam_size);
    if (rc) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!work || !scores) return ASG_ERR_INVALID;
    const bool store = (flags & ASG_FLAG_GRAPH_LOSS_KEEP_ALPHA) != 0;
    if (work_bytes < asg_beam_graph_full_work_bytes(p, gl, beam_size, store)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gl->beam->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gl->beam);
    BeamLossArgs L{};
    L.S = (int) gl->S; L.start = gl->start; L.next = gl->next;
    const int K = beam_graph_k(G.Q, beam_size);
    return hip_status(ASG_DISPATCH(p,
        launch_beam_loss_forward<float>(P, G, BG, L, K, beam_threshold, store, work, scores, (hipStream_t) stream),
        launch_beam_loss_forward<double>(P, G, BG, L, K, beam_threshold, store, work, scores, (hipStream_t) stream)));
}

int asg_beam_graph_full_backward(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                                 const void *work, size_t work_bytes, const void *scores, const void *grad_scores,
                                 void *grad_inputs, void *grad_transition, void *scratch, size_t scratch_bytes, int flags,
                                 void *stream) {
    (void) ctx;
    return lattice_full_backward(
        p, check_beam_loss(p, gl, beam_size), asg_beam_graph_full_work_bytes(p, gl, beam_size, 1),
        asg_beam_graph_full_scratch_bytes(p, gl, beam_size), work, work_bytes, scores, grad_scores, grad_inputs, grad_transition, scratch, scratch_bytes, flags,
        [&](const Problem &P, bool acc, auto r) {
            const GraphArgs G = to_graph_args(gl->beam->graph);
            return launch_beam_loss_backward<decltype(r)>(P, G, to_beam_graph_args(gl->beam), beam_graph_k(G.Q, beam_size), work, scores,
                                                          grad_scores, grad_inputs, grad_transition, scratch, acc,
                                                          (hipStream_t) stream);
        });
}

// The token confidences: the checks of the beam-pruned loss WITHOUT targets (targets in the problem are not looked at).
static int check_beam_conf(const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size) {
    if (!p) return ASG_ERR_INVALID;
    asg_problem q = *p;
    q.targets = nullptr;
    return check_beam_loss(&q, gl, beam_size);
}

size_t asg_beam_graph_confidence_work_bytes(const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size) {
    if (check_beam_conf(p, gl, beam_size) != ASG_OK) return 0;
    const asg_token_graph_beam *gb = gl->beam;
    const int Q = (int) gb->graph->Q, K = beam_graph_k(Q, beam_size);
    return beam_conf_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, Q, K,
                                beam_graph_cap(Q, K, gb->max_out, (int) gb->num_start));
}

int asg_beam_graph_confidence(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                              double beam_threshold, int frame_tolerance, void *work, size_t work_bytes, void *scores,
                              int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *token_frames,
                              void *token_confidences, void *normalisers, int flags, void *stream) {
    (void) ctx; (void) flags;
    int rc = check_beam_conf(p, gl, beam_size);
    if (rc) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (frame_tolerance < 0) return ASG_ERR_INVALID;
    if (frame_tolerance > kBeamConfMaxTol) return ASG_ERR_UNSUPPORTED;
    if (!work || !scores || !path || !tokens || !token_lengths || !states || !token_frames || !token_confidences || !normalisers)
        return ASG_ERR_INVALID;
    if (work_bytes < asg_beam_graph_confidence_work_bytes(p, gl, beam_size)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gl->beam->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gl->beam);
    BeamLossArgs L{};
    L.S = (int) gl->S; L.start = gl->start; L.next = gl->next;
    const int K = beam_graph_k(G.Q, beam_size);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *tf = (long long *) token_frames;
    return hip_status(ASG_DISPATCH(p,
        launch_beam_conf<float>(P, G, BG, L, K, beam_threshold, frame_tolerance, work, scores, pa, tk, tl, st, tf, token_confidences,
                                normalisers, (hipStream_t) stream),
        launch_beam_conf<double>(P, G, BG, L, K, beam_threshold, frame_tolerance, work, scores, pa, tk, tl, st, tf, token_confidences,
                                 normalisers, (hipStream_t) stream)));
}

// The lattice-keeping stream: the checks of a plain stream state through the beam view, then those of the token confidences
// through a problem of max_frames frames without targets (its emissions are not read).
static int check_beam_conf_stream(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size, int64_t max_frames) {
    if (!gl) return ASG_ERR_INVALID;
    int rc = check_beam_stream(gl->beam, B, dtype, beam_size, max_frames);
    if (rc) return rc;
    asg_problem q{};
    q.inputs = gl; q.transition = gl;
    q.T = max_frames; q.B = B; q.N = gl->beam->graph->N; q.S = 1; q.dtype = dtype;
    return check_beam_loss(&q, gl, beam_size);
}

static size_t beam_conf_stream_bytes(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size, int64_t max_frames) {
    const asg_token_graph_beam *gb = gl->beam;
    const int Q = (int) gb->graph->Q, K = beam_graph_k(Q, beam_size);
    return beam_conf_stream_state_bytes(dtype == ASG_DTYPE_F64 ? 8 : 4, (int) max_frames, (int) B, Q, K,
                                        beam_graph_cap(Q, K, gb->max_out, (int) gb->num_start), (int) gb->graph->N);
}

size_t asg_beam_conf_stream_state_bytes(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size,
                                        int64_t max_frames) {
    if (check_beam_conf_stream(gl, B, dtype, beam_size, max_frames) != ASG_OK) return 0;
    return beam_conf_stream_bytes(gl, B, dtype, beam_size, max_frames);
}

// reset, advance, result and n-best: the plain stream's host path (beam_stream_reset and its siblings above) with the loss view
int asg_beam_conf_stream_reset(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t max_frames,
                               void *state, size_t state_bytes, const uint8_t *mask, int flags, void *stream) {
    (void) ctx; (void) flags;
    if (!gl) return ASG_ERR_INVALID;
    return beam_stream_reset(gl->beam, gl, B, beam_size, max_frames, state, state_bytes, mask, stream);
}

int asg_beam_conf_stream_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                                 double beam_threshold, int64_t max_frames, void *state, size_t state_bytes, int flags,
                                 void *stream) {
    (void) ctx; (void) flags;
    if (!gl) return ASG_ERR_INVALID;
    return beam_stream_advance(p, gl->beam, gl, beam_size, beam_threshold, max_frames, state, state_bytes, stream);
}

int asg_beam_conf_stream_result(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t max_frames,
                                const void *state, size_t state_bytes, int final, void *scores, int64_t *path, int64_t *tokens,
                                int64_t *token_lengths, int64_t *states, int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    if (!gl) return ASG_ERR_INVALID;
    return beam_stream_result(gl->beam, gl, B, beam_size, max_frames, state, state_bytes, final, scores, path, tokens, token_lengths,
                              states, frames, status, stream);
}

size_t asg_beam_conf_stream_nbest_work_bytes(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size,
                                             int64_t max_frames, int nbest) {
    if (!gl || check_beam_stream_nbest(gl->beam, gl, B, dtype, beam_size, max_frames, nbest) != ASG_OK) return 0;
    return beam_stream_nbest_bytes(gl->beam, B, beam_size, max_frames, nbest);
}

int asg_beam_conf_stream_nbest(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t max_frames,
                               const void *state, size_t state_bytes, int final, int nbest, void *work, size_t work_bytes,
                               void *scores, void *graph_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                               int64_t *states, int64_t *num_hyps, int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    if (!gl) return ASG_ERR_INVALID;
    return beam_stream_nbest(gl->beam, gl, B, beam_size, max_frames, state, state_bytes, final, nbest, work, work_bytes, scores,
                             graph_scores, path, tokens, token_lengths, states, num_hyps, frames, status, stream);
}

int asg_beam_conf_stream_confidence(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t max_frames,
                                    void *state, size_t state_bytes, const void *transition, const int64_t *transition_strides,
                                    int final, int frame_tolerance, void *scores, int64_t *path, int64_t *tokens,
                                    int64_t *token_lengths, int64_t *states, int64_t *token_frames, void *token_confidences,
                                    void *normalisers, int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    if (!gl || !gl->beam || !gl->beam->graph) return ASG_ERR_INVALID;
    const asg_token_graph_beam *gb = gl->beam;
    const asg_token_graph *g = gb->graph;
    int rc = check_beam_conf_stream(gl, B, g->dtype, beam_size, max_frames);
    if (rc) return rc;
    if (frame_tolerance < 0) return ASG_ERR_INVALID;
    if (frame_tolerance > kBeamConfMaxTol) return ASG_ERR_UNSUPPORTED;
    if (!state || !transition || !transition_strides || !scores || !path || !tokens || !token_lengths || !states || !token_frames ||
        !token_confidences || !normalisers || !frames || !status)
        return ASG_ERR_INVALID;
    if (state_bytes < beam_conf_stream_bytes(gl, B, g->dtype, beam_size, max_frames)) return ASG_ERR_WORKSPACE;
    Problem P{};
    P.transition = transition; P.ts0 = transition_strides[0]; P.ts1 = transition_strides[1];
    P.T = (int) max_frames; P.B = (int) B; P.N = g->N; P.S = 1;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *tf = (long long *) token_frames, *fr = (long long *) frames, *su = (long long *) status;
    return hip_status(ASG_DISPATCH(g,
        launch_beam_conf_stream_confidence<float>(P, G, BG, K, (int) max_frames, state, final, frame_tolerance, scores, pa, tk, tl, st,
                                                  tf, token_confidences, normalisers, fr, su, (hipStream_t) stream),
        launch_beam_conf_stream_confidence<double>(P, G, BG, K, (int) max_frames, state, final, frame_tolerance, scores, pa, tk, tl, st,
                                                   tf, token_confidences, normalisers, fr, su, (hipStream_t) stream)));
}

// The lattice-keeping window stream: the checks of a plain window state through the beam view, the two parameters that size the
// ring, then those of the token confidences through a problem of W frames without targets (its emissions are not read).
static int check_beam_conf_window(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size, int64_t W, int64_t P,
                                  int frame_tolerance, int64_t max_chunk) {
    if (!gl) return ASG_ERR_INVALID;
    int rc = check_beam_window(gl->beam, B, dtype, beam_size, W, P);
    if (rc) return rc;
    if (frame_tolerance < 0 || max_chunk < 1) return ASG_ERR_INVALID;
    if (frame_tolerance > kBeamConfMaxTol) return ASG_ERR_UNSUPPORTED;
    if (W + frame_tolerance + 1 + max_chunk > (int64_t) 0x7FFFFFFF) return ASG_ERR_UNSUPPORTED;      // the rows of the ring
    if (max_chunk / P + 1 > kBeamConfWindowMaxLog) return ASG_ERR_UNSUPPORTED;      // the log's entries are the pull's grid rows
    asg_problem q{};
    q.inputs = gl; q.transition = gl;
    q.T = W; q.B = B; q.N = gl->beam->graph->N; q.S = 1; q.dtype = dtype;
    return check_beam_loss(&q, gl, beam_size);
}

static size_t beam_conf_window_bytes(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size, int64_t W, int64_t P,
                                     int frame_tolerance, int64_t max_chunk) {
    const asg_token_graph_beam *gb = gl->beam;
    const int Q = (int) gb->graph->Q, K = beam_graph_k(Q, beam_size);
    return beam_conf_window_state_bytes(dtype == ASG_DTYPE_F64 ? 8 : 4, (int) W, (int) P, frame_tolerance, (int) max_chunk, (int) B, Q,
                                        K, beam_graph_cap(Q, K, gb->max_out, (int) gb->num_start), (int) gb->graph->N);
}

size_t asg_beam_conf_window_state_bytes(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size, int64_t W,
                                        int64_t P, int frame_tolerance, int64_t max_chunk) {
    if (check_beam_conf_window(gl, B, dtype, beam_size, W, P, frame_tolerance, max_chunk) != ASG_OK) return 0;
    return beam_conf_window_bytes(gl, B, dtype, beam_size, W, P, frame_tolerance, max_chunk);
}

// reset, result and n-best: the plain window's kernels over the wider slot
int asg_beam_conf_window_reset(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t W, int64_t P,
                               int frame_tolerance, int64_t max_chunk, void *state, size_t state_bytes, const uint8_t *mask,
                               int flags, void *stream) {
    (void) ctx; (void) flags;
    if (!gl || !gl->beam || !gl->beam->graph) return ASG_ERR_INVALID;
    const asg_token_graph_beam *gb = gl->beam;
    const int dtype = gb->graph->dtype;
    int rc = check_beam_conf_window(gl, B, dtype, beam_size, W, P, frame_tolerance, max_chunk);
    if (rc) return rc;
    if (!state) return ASG_ERR_INVALID;
    if (state_bytes < beam_conf_window_bytes(gl, B, dtype, beam_size, W, P, frame_tolerance, max_chunk)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(gb->graph);
    return hip_status(launch_beam_window_reset(dtype == ASG_DTYPE_F64 ? 8 : 4, G, to_beam_graph_args(gb),
                                               beam_graph_k(G.Q, beam_size), (int) W, (int) B, state, mask, (hipStream_t) stream,
                                               beam_conf_window_bytes(gl, 1, dtype, beam_size, W, P, frame_tolerance, max_chunk)));
}

int asg_beam_conf_window_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                                 double beam_threshold, int64_t W, int64_t P, int frame_tolerance, int64_t max_chunk, void *state,
                                 size_t state_bytes, int64_t *new_path, int64_t *new_states, int64_t *new_tokens,
                                 int64_t *new_frames, int64_t *new_token_lengths, int64_t *new_token_frames,
                                 void *new_token_confidences, int flags, void *stream) {
    (void) ctx; (void) flags;
    if (!p || !gl || !gl->beam || !gl->beam->graph) return ASG_ERR_INVALID;
    const asg_token_graph_beam *gb = gl->beam;
    int rc = check_beam_conf_window(gl, p->B, p->dtype, beam_size, W, P, frame_tolerance, max_chunk);
    if (rc) return rc;
    if (p->T < 0 || p->N != gb->graph->N) return ASG_ERR_INVALID;
    if (p->T > max_chunk) return ASG_ERR_UNSUPPORTED;                      // the ring holds max_chunk frames behind an attempt
    if (p->T > 0 && (rc = check_beam_graph(p, gb, beam_size)) != ASG_OK) return rc;
    if (!p->transition) return ASG_ERR_INVALID;                            // (the catch-up reads it also when no frame comes)
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!state || !new_path || !new_states || !new_tokens || !new_frames || !new_token_lengths || !new_token_frames ||
        !new_token_confidences)
        return ASG_ERR_INVALID;
    if (state_bytes < beam_conf_window_bytes(gl, p->B, p->dtype, beam_size, W, P, frame_tolerance, max_chunk))
        return ASG_ERR_WORKSPACE;
    const Problem Pr = to_problem(p);                                      // (no frame: the launches still write the empty outputs)
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    long long *np = (long long *) new_path, *ns = (long long *) new_states, *nt = (long long *) new_tokens;
    long long *nf = (long long *) new_frames, *nl = (long long *) new_token_lengths, *tf = (long long *) new_token_frames;
    return hip_status(ASG_DISPATCH(p,
        launch_beam_conf_window_advance<float>(Pr, G, BG, K, beam_threshold, (int) W, (int) P, frame_tolerance, (int) max_chunk, state,
                                               np, ns, nt, nf, nl, tf, new_token_confidences, (hipStream_t) stream),
        launch_beam_conf_window_advance<double>(Pr, G, BG, K, beam_threshold, (int) W, (int) P, frame_tolerance, (int) max_chunk,
                                                state, np, ns, nt, nf, nl, tf, new_token_confidences, (hipStream_t) stream)));
}

int asg_beam_conf_window_result(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t W, int64_t P,
                                int frame_tolerance, int64_t max_chunk, const void *state, size_t state_bytes, int final,
                                void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                                int64_t *frames, int64_t *committed, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    if (!gl || !gl->beam || !gl->beam->graph) return ASG_ERR_INVALID;
    const asg_token_graph_beam *gb = gl->beam;
    const asg_token_graph *g = gb->graph;
    int rc = check_beam_conf_window(gl, B, g->dtype, beam_size, W, P, frame_tolerance, max_chunk);
    if (rc) return rc;
    if (!state || !scores || !path || !tokens || !token_lengths || !states || !frames || !committed || !status)
        return ASG_ERR_INVALID;
    if (state_bytes < beam_conf_window_bytes(gl, B, g->dtype, beam_size, W, P, frame_tolerance, max_chunk)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    const size_t per = beam_conf_window_bytes(gl, 1, g->dtype, beam_size, W, P, frame_tolerance, max_chunk);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *fr = (long long *) frames, *co = (long long *) committed, *su = (long long *) status;
    return hip_status(ASG_DISPATCH(g, launch_beam_window_result<float>(G, BG, K, (int) W, (int) B, state, final, scores, pa, tk, tl,
                                                                       st, fr, co, su, (hipStream_t) stream, per),
                                   launch_beam_window_result<double>(G, BG, K, (int) W, (int) B, state, final, scores, pa, tk, tl,
                                                                     st, fr, co, su, (hipStream_t) stream, per)));
}

static int check_beam_conf_window_nbest(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size, int64_t W,
                                        int64_t P, int frame_tolerance, int64_t max_chunk, int nbest) {
    int rc = check_beam_conf_window(gl, B, dtype, beam_size, W, P, frame_tolerance, max_chunk);
    if (rc) return rc;
    if (nbest < 1) return ASG_ERR_INVALID;
    if (nbest > kBeamMaxNbest) return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

size_t asg_beam_conf_window_nbest_work_bytes(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size, int64_t W,
                                             int64_t P, int frame_tolerance, int64_t max_chunk, int nbest) {
    if (check_beam_conf_window_nbest(gl, B, dtype, beam_size, W, P, frame_tolerance, max_chunk, nbest) != ASG_OK) return 0;
    return beam_stream_nbest_bytes(gl->beam, B, beam_size, W, nbest);
}

int asg_beam_conf_window_nbest(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t W, int64_t P,
                               int frame_tolerance, int64_t max_chunk, const void *state, size_t state_bytes, int final, int nbest,
                               void *work, size_t work_bytes, void *scores, int64_t *path, int64_t *tokens,
                               int64_t *token_lengths, int64_t *states, int64_t *num_hyps, int64_t *frames, int64_t *committed,
                               int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    if (!gl || !gl->beam || !gl->beam->graph) return ASG_ERR_INVALID;
    const asg_token_graph_beam *gb = gl->beam;
    const asg_token_graph *g = gb->graph;
    int rc = check_beam_conf_window_nbest(gl, B, g->dtype, beam_size, W, P, frame_tolerance, max_chunk, nbest);
    if (rc) return rc;
    if (!state || !work || !scores || !tokens || !token_lengths || !num_hyps || !frames || !committed || !status)
        return ASG_ERR_INVALID;
    if (state_bytes < beam_conf_window_bytes(gl, B, g->dtype, beam_size, W, P, frame_tolerance, max_chunk)) return ASG_ERR_WORKSPACE;
    if (work_bytes < beam_stream_nbest_bytes(gb, B, beam_size, W, nbest)) return ASG_ERR_WORKSPACE;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    const size_t per = beam_conf_window_bytes(gl, 1, g->dtype, beam_size, W, P, frame_tolerance, max_chunk);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *nh = (long long *) num_hyps, *fr = (long long *) frames, *co = (long long *) committed, *su = (long long *) status;
    return hip_status(ASG_DISPATCH(g, launch_beam_window_nbest<float>(G, BG, K, (int) W, (int) B, state, final, nbest, work, scores,
                                                                      pa, tk, tl, st, nh, fr, co, su, (hipStream_t) stream, per),
                                   launch_beam_window_nbest<double>(G, BG, K, (int) W, (int) B, state, final, nbest, work, scores,
                                                                    pa, tk, tl, st, nh, fr, co, su, (hipStream_t) stream, per)));
}

int asg_beam_conf_window_confidence(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t W,
                                    int64_t P, int frame_tolerance, int64_t max_chunk, void *state, size_t state_bytes,
                                    const void *transition, const int64_t *transition_strides, int final, void *scores,
                                    int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *token_frames,
                                    void *token_confidences, void *normalisers, int64_t *frames, int64_t *committed,
                                    int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    if (!gl || !gl->beam || !gl->beam->graph) return ASG_ERR_INVALID;
    const asg_token_graph_beam *gb = gl->beam;
    const asg_token_graph *g = gb->graph;
    int rc = check_beam_conf_window(gl, B, g->dtype, beam_size, W, P, frame_tolerance, max_chunk);
    if (rc) return rc;
    if (!state || !transition || !transition_strides || !scores || !path || !tokens || !token_lengths || !states || !token_frames ||
        !token_confidences || !normalisers || !frames || !committed || !status)
        return ASG_ERR_INVALID;
    if (state_bytes < beam_conf_window_bytes(gl, B, g->dtype, beam_size, W, P, frame_tolerance, max_chunk)) return ASG_ERR_WORKSPACE;
    Problem Pr{};
    Pr.transition = transition; Pr.ts0 = transition_strides[0]; Pr.ts1 = transition_strides[1];
    Pr.T = (int) W; Pr.B = (int) B; Pr.N = g->N; Pr.S = 1;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const int K = beam_graph_k(G.Q, beam_size);
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *tf = (long long *) token_frames, *fr = (long long *) frames, *co = (long long *) committed, *su = (long long *) status;
    return hip_status(ASG_DISPATCH(g,
        launch_beam_conf_window_confidence<float>(Pr, G, BG, K, (int) W, (int) P, frame_tolerance, (int) max_chunk, state, final, scores,
                                                  pa, tk, tl, st, tf, token_confidences, normalisers, fr, co, su,
                                                  (hipStream_t) stream),
        launch_beam_conf_window_confidence<double>(Pr, G, BG, K, (int) W, (int) P, frame_tolerance, (int) max_chunk, state, final,
                                                   scores, pa, tk, tl, st, tf, token_confidences, normalisers, fr, co, su,
                                                   (hipStream_t) stream)));
}

// The n-best token confidences: the checks of asg_beam_graph_confidence, then those of asg_beam_decode_graph_nbest.
static int check_beam_nbest_conf(const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size, int nbest) {
    int rc = check_beam_conf(p, gl, beam_size);
    if (rc) return rc;
    if (nbest < 1) return ASG_ERR_INVALID;
    if (nbest > kBeamMaxNbest) return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

size_t asg_beam_graph_nbest_confidence_work_bytes(const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                                                  int nbest) {
    if (check_beam_nbest_conf(p, gl, beam_size, nbest) != ASG_OK) return 0;
    const asg_token_graph_beam *gb = gl->beam;
    const int Q = (int) gb->graph->Q, K = beam_graph_k(Q, beam_size);
    return beam_nbest_conf_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, Q, K,
                                      beam_graph_cap(Q, K, gb->max_out, (int) gb->num_start), nbest);
}

// The order of the checks: the one-best confidence's, the n-best's, the tolerance and the limit of the row sink, then threshold,
// buffers and workspace as everywhere.
int asg_beam_graph_nbest_confidence(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                                    double beam_threshold, int nbest, int frame_tolerance, void *work, size_t work_bytes,
                                    void *scores, void *emission_scores, void *graph_scores, int64_t *path, int64_t *tokens,
                                    int64_t *token_lengths, int64_t *states, int64_t *num_hyps, int64_t *token_frames,
                                    void *token_confidences, void *normalisers, int flags, void *stream) {
    (void) ctx; (void) flags;
    int rc = check_beam_nbest_conf(p, gl, beam_size, nbest);
    if (rc) return rc;
    if (frame_tolerance < 0) return ASG_ERR_INVALID;
    if (frame_tolerance > kBeamConfMaxTol) return ASG_ERR_UNSUPPORTED;
    const int K = beam_graph_k((int) gl->beam->graph->Q, beam_size);
    if (!beam_nbest_conf_fits(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, K, nbest, frame_tolerance)) return ASG_ERR_UNSUPPORTED;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!work || !scores || !emission_scores || !graph_scores || !tokens || !token_lengths || !num_hyps || !token_frames ||
        !token_confidences || !normalisers)
        return ASG_ERR_INVALID;
    if (work_bytes < asg_beam_graph_nbest_confidence_work_bytes(p, gl, beam_size, nbest)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gl->beam->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gl->beam);
    BeamLossArgs L{};
    L.S = (int) gl->S; L.start = gl->start; L.next = gl->next;
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *nh = (long long *) num_hyps, *tf = (long long *) token_frames;
    return hip_status(ASG_DISPATCH(p,
        launch_beam_nbest_conf<float>(P, G, BG, L, K, beam_threshold, nbest, frame_tolerance, work, scores, emission_scores,
                                      graph_scores, pa, tk, tl, st, nh, tf, token_confidences, normalisers, (hipStream_t) stream),
        launch_beam_nbest_conf<double>(P, G, BG, L, K, beam_threshold, nbest, frame_tolerance, work, scores, emission_scores,
                                       graph_scores, pa, tk, tl, st, nh, tf, token_confidences, normalisers, (hipStream_t) stream)));
}

static int check_beam_words_loss(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size) {
    int rc = check_beam_words(p, gb, lm, beam_size);
    if (rc) return rc;
    return check_lattice(p, beam_size, beam_word_loss_fits);
}

size_t asg_beam_words_full_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size,
                                      int store) {
    if (check_beam_words_loss(p, gb, lm, beam_size) != ASG_OK) return 0;
    return beam_word_loss_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, beam_size,
                                     beam_word_cap(beam_size, gb->max_out, (int) gb->num_start), beam_loss_nf(p), store != 0);
}

size_t asg_beam_words_full_scratch_bytes(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size) {
    if (check_beam_words_loss(p, gb, lm, beam_size) != ASG_OK) return 0;
    return (size_t) p->B * beam_word_loss_scratch_per(p->dtype == ASG_DTYPE_F64 ? 8 : 4, beam_size + beam_loss_nf(p), (int) p->N);
}

// asg_beam_words_full_forward with a look-ahead (`with_la`: la is checked as asg_beam_decode_words_la checks it, behind the LM) or
// without one.  Only the search reads it; the workspace has the same bytes either way.
static int beam_words_full_forward(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                   const asg_word_lookahead *la, bool with_la, int beam_size, double beam_threshold, void *work,
                                   size_t work_bytes, void *scores, int flags, void *stream) {
    int rc = check_beam_words_loss(p, gb, lm, beam_size);
    if (rc) return rc;
    if (with_la && (rc = check_word_lookahead(p->dtype, lm, la)) != ASG_OK) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!work || !scores) return ASG_ERR_INVALID;
    const bool store = (flags & ASG_FLAG_GRAPH_LOSS_KEEP_ALPHA) != 0;
    if (work_bytes < asg_beam_words_full_work_bytes(p, gb, lm, beam_size, store)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    const WordLookArgs LA = with_la ? to_word_look_args(la) : WordLookArgs{};
    const WordLookArgs *look = with_la ? &LA : nullptr;
    return hip_status(ASG_DISPATCH(p,
        launch_beam_word_loss_forward<float>(P, G, BG, LM, look, beam_size, beam_threshold, store, work, scores, (hipStream_t) stream),
        launch_beam_word_loss_forward<double>(P, G, BG, LM, look, beam_size, beam_threshold, store, work, scores, (hipStream_t) stream)));
}

int asg_beam_words_full_forward(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                int beam_size, double beam_threshold, void *work, size_t work_bytes, void *scores, int flags,
                                void *stream) {
    (void) ctx;
    return beam_words_full_forward(p, gb, lm, nullptr, false, beam_size, beam_threshold, work, work_bytes, scores, flags, stream);
}

int asg_beam_words_full_forward_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                   const asg_word_lookahead *la, int beam_size, double beam_threshold, void *work, size_t work_bytes,
                                   void *scores, int flags, void *stream) {
    (void) ctx;
    return beam_words_full_forward(p, gb, lm, la, true, beam_size, beam_threshold, work, work_bytes, scores, flags, stream);
}

int asg_beam_words_full_backward(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                 int beam_size, const void *work, size_t work_bytes, const void *scores, const void *grad_scores,
                                 void *grad_inputs, void *grad_transition, void *scratch, size_t scratch_bytes, int flags,
                                 void *stream) {
    (void) ctx;
    return lattice_full_backward(
        p, check_beam_words_loss(p, gb, lm, beam_size), asg_beam_words_full_work_bytes(p, gb, lm, beam_size, 1),
        asg_beam_words_full_scratch_bytes(p, gb, lm, beam_size), work, work_bytes, scores, grad_scores, grad_inputs,
        grad_transition, scratch, scratch_bytes, flags, [&](const Problem &P, bool acc, auto r) {
            return launch_beam_word_loss_backward<decltype(r)>(P, to_graph_args(gb->graph), to_beam_graph_args(gb), to_word_lm_args(lm),
                                                               beam_size, work, scores, grad_scores, grad_inputs, grad_transition,
                                                               scratch, acc, (hipStream_t) stream);
        });
}

int asg_words_target_scores(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, void *out,
                            void *stream) {
    (void) ctx;
    int rc = check_beam_words(p, gb, lm, 1);
    if (rc) return rc;
    if (!out || !p->targets || p->S < 1) return ASG_ERR_INVALID;
    if (p->S > (1 << 30)) return ASG_ERR_UNSUPPORTED;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    return hip_status(ASG_DISPATCH(p, launch_beam_word_target_scores<float>(P, G, BG, LM, out, (hipStream_t) stream),
                                   launch_beam_word_target_scores<double>(P, G, BG, LM, out, (hipStream_t) stream)));
}

// The word confidences: the checks of the pair loss WITHOUT targets (targets in the problem are not looked at).
static int check_beam_words_conf(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size) {
    int rc = check_beam_words(p, gb, lm, beam_size);
    if (rc) return rc;
    asg_problem q = *p;
    q.targets = nullptr;
    return check_lattice(&q, beam_size, beam_word_loss_fits);
}

size_t asg_beam_words_confidence_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                            int beam_size) {
    if (check_beam_words_conf(p, gb, lm, beam_size) != ASG_OK) return 0;
    return beam_word_conf_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, beam_size,
                                     beam_word_cap(beam_size, gb->max_out, (int) gb->num_start));
}

// asg_beam_words_confidence with a look-ahead (`with_la`: la is checked as asg_beam_decode_words_la checks it, behind the LM) or
// without one.  Only the search reads it; the workspace has the same bytes either way.
static int beam_words_confidence(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                 const asg_word_lookahead *la, bool with_la, int beam_size, double beam_threshold,
                                 int frame_tolerance, void *work, size_t work_bytes, void *scores, int64_t *path, int64_t *tokens,
                                 int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                 int64_t *word_lengths, int64_t *word_frames, void *word_confidences, void *normalisers,
                                 void *stream) {
    int rc = check_beam_words_conf(p, gb, lm, beam_size);
    if (rc) return rc;
    if (with_la && (rc = check_word_lookahead(p->dtype, lm, la)) != ASG_OK) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (frame_tolerance < 0) return ASG_ERR_INVALID;
    if (frame_tolerance > kBeamWordConfMaxTol) return ASG_ERR_UNSUPPORTED;
    if (!work || !scores || !path || !tokens || !token_lengths || !states || !lm_states || !words || !word_lengths ||
        !word_frames || !word_confidences || !normalisers)
        return ASG_ERR_INVALID;
    if (work_bytes < asg_beam_words_confidence_work_bytes(p, gb, lm, beam_size)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    const WordLookArgs LA = with_la ? to_word_look_args(la) : WordLookArgs{};
    const WordLookArgs *look = with_la ? &LA : nullptr;
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *ls = (long long *) lm_states, *wd = (long long *) words, *wl = (long long *) word_lengths;
    long long *wf = (long long *) word_frames;
    return hip_status(ASG_DISPATCH(p,
        launch_beam_word_conf<float>(P, G, BG, LM, look, beam_size, beam_threshold, frame_tolerance, work, scores, pa, tk, tl, st, ls,
                                     wd, wl, wf, word_confidences, normalisers, (hipStream_t) stream),
        launch_beam_word_conf<double>(P, G, BG, LM, look, beam_size, beam_threshold, frame_tolerance, work, scores, pa, tk, tl, st, ls,
                                      wd, wl, wf, word_confidences, normalisers, (hipStream_t) stream)));
}

int asg_beam_words_confidence(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                              int beam_size, double beam_threshold, int frame_tolerance, void *work, size_t work_bytes,
                              void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                              int64_t *lm_states, int64_t *words, int64_t *word_lengths, int64_t *word_frames,
                              void *word_confidences, void *normalisers, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_words_confidence(p, gb, lm, nullptr, false, beam_size, beam_threshold, frame_tolerance, work, work_bytes, scores,
                                 path, tokens, token_lengths, states, lm_states, words, word_lengths, word_frames, word_confidences,
                                 normalisers, stream);
}

int asg_beam_words_confidence_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                 const asg_word_lookahead *la, int beam_size, double beam_threshold, int frame_tolerance, void *work,
                                 size_t work_bytes, void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                                 int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths, int64_t *word_frames,
                                 void *word_confidences, void *normalisers, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_words_confidence(p, gb, lm, la, true, beam_size, beam_threshold, frame_tolerance, work, work_bytes, scores, path,
                                 tokens, token_lengths, states, lm_states, words, word_lengths, word_frames, word_confidences,
                                 normalisers, stream);
}

// The lattice-keeping word stream: the checks of a plain word stream state, then those of the word confidences through a problem
// of max_frames frames without targets (its emissions are not read).
static int check_beam_word_conf_stream(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype, int beam_size,
                                       int64_t max_frames) {
    int rc = check_beam_word_stream(gb, lm, B, dtype, beam_size, max_frames);
    if (rc) return rc;
    asg_problem q{};
    q.inputs = gb; q.transition = gb;
    q.T = max_frames; q.B = B; q.N = gb->graph->N; q.S = 1; q.dtype = dtype;
    return check_lattice(&q, beam_size, beam_word_loss_fits);
}

static size_t beam_word_conf_stream_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t max_frames) {
    return beam_word_conf_stream_state_bytes(dtype == ASG_DTYPE_F64 ? 8 : 4, (int) max_frames, (int) B, beam_size,
                                             beam_word_cap(beam_size, gb->max_out, (int) gb->num_start), (int) gb->graph->N);
}

size_t asg_beam_word_conf_stream_state_bytes(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype,
                                             int beam_size, int64_t max_frames) {
    if (check_beam_word_conf_stream(gb, lm, B, dtype, beam_size, max_frames) != ASG_OK) return 0;
    return beam_word_conf_stream_bytes(gb, B, dtype, beam_size, max_frames);
}

// reset, advance, result and n-best: the plain word stream's host path (beam_word_stream_reset and its siblings) with lattice = true
int asg_beam_word_conf_stream_reset(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                                    int64_t max_frames, void *state, size_t state_bytes, const uint8_t *mask, int flags,
                                    void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_reset(gb, lm, true, B, beam_size, max_frames, state, state_bytes, mask, stream);
}

int asg_beam_word_conf_stream_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                      int beam_size, double beam_threshold, int64_t max_frames, void *state, size_t state_bytes,
                                      int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_advance(p, gb, lm, nullptr, false, true, beam_size, beam_threshold, max_frames, state, state_bytes,
                                    stream);
}

int asg_beam_word_conf_stream_advance_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                         const asg_word_lookahead *la, int beam_size, double beam_threshold, int64_t max_frames,
                                         void *state, size_t state_bytes, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_advance(p, gb, lm, la, true, true, beam_size, beam_threshold, max_frames, state, state_bytes, stream);
}

int asg_beam_word_conf_stream_result(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                                     int64_t max_frames, const void *state, size_t state_bytes, int final, void *scores,
                                     int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states,
                                     int64_t *words, int64_t *word_lengths, int64_t *frames, int64_t *status, int flags,
                                     void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_result(gb, lm, nullptr, false, true, B, beam_size, max_frames, state, state_bytes, final, scores, path,
                                   tokens, token_lengths, states, lm_states, words, word_lengths, frames, status, stream);
}

int asg_beam_word_conf_stream_result_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                        const asg_word_lookahead *la, int64_t B, int beam_size, int64_t max_frames,
                                        const void *state, size_t state_bytes, int final, void *scores, int64_t *path,
                                        int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                        int64_t *word_lengths, int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_result(gb, lm, la, true, true, B, beam_size, max_frames, state, state_bytes, final, scores, path, tokens,
                                   token_lengths, states, lm_states, words, word_lengths, frames, status, stream);
}

size_t asg_beam_word_conf_stream_nbest_work_bytes(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype,
                                                  int beam_size, int64_t max_frames, int nbest) {
    if (check_beam_word_stream_nbest(gb, lm, true, B, dtype, beam_size, max_frames, nbest) != ASG_OK) return 0;
    return beam_word_stream_nbest_work_bytes((int) max_frames, (int) B, beam_size, nbest);
}

int asg_beam_word_conf_stream_nbest(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                                    int64_t max_frames, const void *state, size_t state_bytes, int final, int nbest, void *work,
                                    size_t work_bytes, void *scores, void *graph_scores, void *lm_scores, int64_t *path,
                                    int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                    int64_t *word_lengths, int64_t *num_hyps, int64_t *frames, int64_t *status, int flags,
                                    void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_nbest(gb, lm, nullptr, false, true, B, beam_size, max_frames, state, state_bytes, final, nbest, work,
                                  work_bytes, scores, graph_scores, lm_scores, path, tokens, token_lengths, states, lm_states, words,
                                  word_lengths, num_hyps, frames, status, stream);
}

int asg_beam_word_conf_stream_nbest_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                       const asg_word_lookahead *la, int64_t B, int beam_size, int64_t max_frames, const void *state,
                                       size_t state_bytes, int final, int nbest, void *work, size_t work_bytes, void *scores,
                                       void *graph_scores, void *lm_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                                       int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths,
                                       int64_t *num_hyps, int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_stream_nbest(gb, lm, la, true, true, B, beam_size, max_frames, state, state_bytes, final, nbest, work,
                                  work_bytes, scores, graph_scores, lm_scores, path, tokens, token_lengths, states, lm_states, words,
                                  word_lengths, num_hyps, frames, status, stream);
}

static int beam_word_conf_stream_confidence(const asg_token_graph_beam *gb, const asg_word_lm *lm, const asg_word_lookahead *la,
                                            bool with_la, int64_t B, int beam_size, int64_t max_frames, void *state,
                                            size_t state_bytes, const void *transition, const int64_t *transition_strides,
                                            int final, int frame_tolerance, void *scores, int64_t *path, int64_t *tokens,
                                            int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                            int64_t *word_lengths, int64_t *word_frames, void *word_confidences, void *normalisers,
                                            int64_t *frames, int64_t *status, void *stream) {
    if (!gb || !gb->graph) return ASG_ERR_INVALID;
    const asg_token_graph *g = gb->graph;
    int rc = check_beam_word_conf_stream(gb, lm, B, g->dtype, beam_size, max_frames);
    if (rc) return rc;
    if (with_la && (rc = check_word_lookahead(g->dtype, lm, la)) != ASG_OK) return rc;
    if (frame_tolerance < 0) return ASG_ERR_INVALID;
    if (frame_tolerance > kBeamWordConfMaxTol) return ASG_ERR_UNSUPPORTED;
    if (!state || !transition || !transition_strides || !scores || !path || !tokens || !token_lengths || !states || !lm_states ||
        !words || !word_lengths || !word_frames || !word_confidences || !normalisers || !frames || !status)
        return ASG_ERR_INVALID;
    if (state_bytes < beam_word_conf_stream_bytes(gb, B, g->dtype, beam_size, max_frames)) return ASG_ERR_WORKSPACE;
    Problem P{};
    P.transition = transition; P.ts0 = transition_strides[0]; P.ts1 = transition_strides[1];
    P.T = (int) max_frames; P.B = (int) B; P.N = g->N; P.S = 1;
    const GraphArgs G = to_graph_args(g);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    const WordLookArgs LA = with_la ? to_word_look_args(la) : WordLookArgs{};
    const WordLookArgs *look = with_la ? &LA : nullptr;
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *ls = (long long *) lm_states, *wd = (long long *) words, *wl = (long long *) word_lengths;
    long long *wf = (long long *) word_frames, *fr = (long long *) frames, *su = (long long *) status;
    return hip_status(ASG_DISPATCH(g,
        launch_beam_word_conf_stream_confidence<float>(P, G, BG, LM, look, beam_size, (int) max_frames, state, final, frame_tolerance,
                                                       scores, pa, tk, tl, st, ls, wd, wl, wf, word_confidences, normalisers, fr, su,
                                                       (hipStream_t) stream),
        launch_beam_word_conf_stream_confidence<double>(P, G, BG, LM, look, beam_size, (int) max_frames, state, final, frame_tolerance,
                                                        scores, pa, tk, tl, st, ls, wd, wl, wf, word_confidences, normalisers, fr, su,
                                                        (hipStream_t) stream)));
}

int asg_beam_word_conf_stream_confidence(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B,
                                         int beam_size, int64_t max_frames, void *state, size_t state_bytes, const void *transition,
                                         const int64_t *transition_strides, int final, int frame_tolerance, void *scores,
                                         int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states,
                                         int64_t *words, int64_t *word_lengths, int64_t *word_frames, void *word_confidences,
                                         void *normalisers, int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_conf_stream_confidence(gb, lm, nullptr, false, B, beam_size, max_frames, state, state_bytes, transition,
                                            transition_strides, final, frame_tolerance, scores, path, tokens, token_lengths, states,
                                            lm_states, words, word_lengths, word_frames, word_confidences, normalisers, frames,
                                            status, stream);
}

int asg_beam_word_conf_stream_confidence_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                            const asg_word_lookahead *la, int64_t B, int beam_size, int64_t max_frames, void *state,
                                            size_t state_bytes, const void *transition, const int64_t *transition_strides, int final,
                                            int frame_tolerance, void *scores, int64_t *path, int64_t *tokens,
                                            int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                            int64_t *word_lengths, int64_t *word_frames, void *word_confidences, void *normalisers,
                                            int64_t *frames, int64_t *status, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_word_conf_stream_confidence(gb, lm, la, true, B, beam_size, max_frames, state, state_bytes, transition,
                                            transition_strides, final, frame_tolerance, scores, path, tokens, token_lengths, states,
                                            lm_states, words, word_lengths, word_frames, word_confidences, normalisers, frames,
                                            status, stream);
}

// The n-best confidences: the checks of asg_beam_words_confidence, then those of asg_beam_decode_words_nbest.
static int check_beam_words_nbest_conf(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size,
                                       int nbest) {
    int rc = check_beam_words_conf(p, gb, lm, beam_size);
    if (rc) return rc;
    if (nbest < 1) return ASG_ERR_INVALID;
    if (nbest > kBeamMaxNbest) return ASG_ERR_UNSUPPORTED;
    return ASG_OK;
}

size_t asg_beam_words_nbest_confidence_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                                  int beam_size, int nbest) {
    if (check_beam_words_nbest_conf(p, gb, lm, beam_size, nbest) != ASG_OK) return 0;
    return beam_word_nbest_conf_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, beam_size,
                                           beam_word_cap(beam_size, gb->max_out, (int) gb->num_start), nbest);
}

// asg_beam_words_nbest_confidence with a look-ahead (`with_la`) or without one.  The order of the checks: the decoder's, the
// n-best's, the tolerance and the limit of the row sink, the look-ahead's, then threshold, buffers and workspace as everywhere.
static int beam_words_nbest_confidence(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                       const asg_word_lookahead *la, bool with_la, int beam_size, double beam_threshold, int nbest,
                                       int frame_tolerance, void *work, size_t work_bytes, void *scores, void *emission_scores,
                                       void *graph_scores, void *lm_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                                       int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths,
                                       int64_t *num_hyps, int64_t *word_frames, void *word_confidences, void *normalisers,
                                       void *stream) {
    int rc = check_beam_words_nbest_conf(p, gb, lm, beam_size, nbest);
    if (rc) return rc;
    if (frame_tolerance < 0) return ASG_ERR_INVALID;
    if (frame_tolerance > kBeamWordConfMaxTol) return ASG_ERR_UNSUPPORTED;
    if (!beam_word_nbest_conf_fits(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, beam_size, nbest, frame_tolerance))
        return ASG_ERR_UNSUPPORTED;
    if (with_la && (rc = check_word_lookahead(p->dtype, lm, la)) != ASG_OK) return rc;
    if (!(beam_threshold >= 0.0)) return ASG_ERR_INVALID;                  // negative or NaN
    if (!work || !scores || !emission_scores || !graph_scores || !lm_scores || !tokens || !token_lengths || !words ||
        !word_lengths || !num_hyps || !word_frames || !word_confidences || !normalisers)
        return ASG_ERR_INVALID;
    if (work_bytes < asg_beam_words_nbest_confidence_work_bytes(p, gb, lm, beam_size, nbest)) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gb->graph);
    const BeamGraphArgs BG = to_beam_graph_args(gb);
    const WordLmArgs LM = to_word_lm_args(lm);
    const WordLookArgs LA = with_la ? to_word_look_args(la) : WordLookArgs{};
    const WordLookArgs *look = with_la ? &LA : nullptr;
    long long *pa = (long long *) path, *tk = (long long *) tokens, *tl = (long long *) token_lengths, *st = (long long *) states;
    long long *ls = (long long *) lm_states, *wd = (long long *) words, *wl = (long long *) word_lengths;
    long long *nh = (long long *) num_hyps, *wf = (long long *) word_frames;
    return hip_status(ASG_DISPATCH(p,
        launch_beam_word_nbest_conf<float>(P, G, BG, LM, look, beam_size, beam_threshold, nbest, frame_tolerance, work, scores,
                                           emission_scores, graph_scores, lm_scores, pa, tk, tl, st, ls, wd, wl, nh, wf,
                                           word_confidences, normalisers, (hipStream_t) stream),
        launch_beam_word_nbest_conf<double>(P, G, BG, LM, look, beam_size, beam_threshold, nbest, frame_tolerance, work, scores,
                                            emission_scores, graph_scores, lm_scores, pa, tk, tl, st, ls, wd, wl, nh, wf,
                                            word_confidences, normalisers, (hipStream_t) stream)));
}

int asg_beam_words_nbest_confidence(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                    int beam_size, double beam_threshold, int nbest, int frame_tolerance, void *work,
                                    size_t work_bytes, void *scores, void *emission_scores, void *graph_scores, void *lm_scores,
                                    int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states,
                                    int64_t *words, int64_t *word_lengths, int64_t *num_hyps, int64_t *word_frames,
                                    void *word_confidences, void *normalisers, int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_words_nbest_confidence(p, gb, lm, nullptr, false, beam_size, beam_threshold, nbest, frame_tolerance, work, work_bytes,
                                       scores, emission_scores, graph_scores, lm_scores, path, tokens, token_lengths, states,
                                       lm_states, words, word_lengths, num_hyps, word_frames, word_confidences, normalisers, stream);
}

int asg_beam_words_nbest_confidence_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                       const asg_word_lookahead *la, int beam_size, double beam_threshold, int nbest,
                                       int frame_tolerance, void *work, size_t work_bytes, void *scores, void *emission_scores,
                                       void *graph_scores, void *lm_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                                       int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths,
                                       int64_t *num_hyps, int64_t *word_frames, void *word_confidences, void *normalisers,
                                       int flags, void *stream) {
    (void) ctx; (void) flags;
    return beam_words_nbest_confidence(p, gb, lm, la, true, beam_size, beam_threshold, nbest, frame_tolerance, work, work_bytes, scores,
                                       emission_scores, graph_scores, lm_scores, path, tokens, token_lengths, states, lm_states,
                                       words, word_lengths, num_hyps, word_frames, word_confidences, normalisers, stream);
}

static GraphLossArgs to_graph_loss_args(const asg_token_graph_loss *gl) {
    GraphLossArgs L{};
    L.S = (int) gl->S; L.start = gl->start;
    L.tgt = gl->tgt; L.orow = gl->orow; L.oedge = gl->oedge; L.lrow = gl->lrow; L.lq = gl->lq; L.pedge = gl->pedge;
    L.next = gl->next; L.pkey = gl->pkey; L.arcw = gl->arcw; L.finw = gl->finw;
    return L;
}

static int graph_loss_route(int flags) {
    return (flags & ASG_FLAG_GRAPH_LOSS_STREAMING) ? 1 : ((flags & ASG_FLAG_GRAPH_LOSS_RESIDENT) ? 2 : 0);
}

size_t asg_graph_full_work_bytes(const asg_problem *p, const asg_token_graph_loss *gl, int store) {
    if (check_graph_loss(p, gl) != ASG_OK) return 0;
    return graph_loss_work_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->T, (int) p->B, (int) gl->graph->Q, store != 0);
}

size_t asg_graph_full_scratch_bytes(const asg_problem *p, const asg_token_graph_loss *gl) {
    if (check_graph_loss(p, gl) != ASG_OK) return 0;
    return graph_loss_scratch_bytes(p->dtype == ASG_DTYPE_F64 ? 8 : 4, (int) p->B, (int) gl->graph->Q, (int) gl->graph->E);
}

int asg_graph_full_forward(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_loss *gl, void *work, size_t work_bytes,
                           void *scores, int flags, void *stream) {
    (void) ctx;
    int rc = check_graph_loss(p, gl);
    if (rc) return rc;
    const bool store = (flags & ASG_FLAG_GRAPH_LOSS_KEEP_ALPHA) != 0;
    const size_t need = asg_graph_full_work_bytes(p, gl, store);
    if (!scores || (need && !work)) return ASG_ERR_INVALID;
    if (work_bytes < need) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gl->graph);
    const int route = graph_loss_route(flags);
    return hip_status(ASG_DISPATCH(p, launch_graph_loss_forward<float>(P, G, route, store, work, scores, (hipStream_t) stream),
                                   launch_graph_loss_forward<double>(P, G, route, store, work, scores, (hipStream_t) stream)));
}

int asg_graph_full_backward(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_loss *gl, const void *work,
                            size_t work_bytes, const void *scores, const void *grad_scores, void *grad_inputs,
                            void *grad_transition, void *scratch, size_t scratch_bytes, int flags, void *stream) {
    (void) ctx;
    int rc = check_graph_loss(p, gl);
    if (rc) return rc;
    const size_t wneed = asg_graph_full_work_bytes(p, gl, 1), sneed = asg_graph_full_scratch_bytes(p, gl);
    if (!scores || !grad_scores || !grad_inputs || !grad_transition || (wneed && !work) || (sneed && !scratch))
        return ASG_ERR_INVALID;
    if (work_bytes < wneed || scratch_bytes < sneed) return ASG_ERR_WORKSPACE;
    const Problem P = to_problem(p);
    const GraphArgs G = to_graph_args(gl->graph);
    const GraphLossArgs L = to_graph_loss_args(gl);
    const int route = graph_loss_route(flags);
    return hip_status(ASG_DISPATCH(p,
        launch_graph_loss_backward<float>(P, G, L, route, work, scores, grad_scores, grad_inputs, grad_transition, scratch,
                                          (hipStream_t) stream),
        launch_graph_loss_backward<double>(P, G, L, route, work, scores, grad_scores, grad_inputs, grad_transition, scratch,
                                           (hipStream_t) stream)));
}

int asg_graph_target_scores(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_loss *gl, void *out, void *stream) {
    (void) ctx;
    int rc = check_graph_loss(p, gl);
    if (rc) return rc;
    if (!out || !p->targets || p->S < 1) return ASG_ERR_INVALID;
    if (p->S > (1 << 30)) return ASG_ERR_UNSUPPORTED;
    const Problem P = to_problem(p);
    const GraphLossArgs L = to_graph_loss_args(gl);
    return hip_status(ASG_DISPATCH(p, launch_graph_target_scores<float>(P, L, out, (hipStream_t) stream),
                                   launch_graph_target_scores<double>(P, L, out, (hipStream_t) stream)));
}

int asg_backward(asg_ctx *ctx, const asg_problem *p, const void *state, size_t state_bytes,
                 const void *grad_full, const void *grad_aligned, void *scratch, size_t scratch_bytes,
                 void *grad_transition, void *grad_inputs, int flags, void *stream) {
    (void) ctx; (void) flags;
    int rc = check_problem(p, true);
    if (rc) return rc;
    if (!state || !grad_full || !grad_aligned || !scratch || !grad_transition || !grad_inputs) return ASG_ERR_INVALID;
    if (state_bytes < asg_state_bytes(p)) return ASG_ERR_WORKSPACE;
    return ASG_DISPATCH(p,
        run_backward<float>(p, state, grad_full, grad_aligned, scratch, scratch_bytes, grad_transition, grad_inputs, 3, (hipStream_t) stream),
        run_backward<double>(p, state, grad_full, grad_aligned, scratch, scratch_bytes, grad_transition, grad_inputs, 3, (hipStream_t) stream));
}

int asg_loss_forward(asg_ctx *ctx, const asg_problem *p, void *state, size_t state_bytes, int reduction,
                     void *loss, void *scores, int flags, void *stream) {
    if (reduction < 0 || reduction > 2 || !loss || !scores) return ASG_ERR_INVALID;
    int rc = check_problem(p, true);
    if (rc) return rc;
    if (!state) return ASG_ERR_INVALID;
    if (state_bytes < asg_state_bytes(p)) return ASG_ERR_WORKSPACE;
    const size_t e = p->dtype == ASG_DTYPE_F64 ? 8 : 4;
    char *sc = (char *) scores;
    void *full = sc, *ali = sc + (size_t) p->B * e;
    flags &= ~ASG_FLAG_ALPHA_SCORES;
    const bool in_kernel = small_full(p->N) && small_aligned(p->S);
    rc = ASG_DISPATCH(p,
        run_forward<float>(ctx, p, state, full, ali, 15, true, flags, (hipStream_t) stream, loss, reduction),
        run_forward<double>(ctx, p, state, full, ali, 15, true, flags, (hipStream_t) stream, loss, reduction));
    if (rc || in_kernel) return rc;
    return hip_status(ASG_DISPATCH(p,
        launch_loss_reduce<float>(full, ali, (int) p->B, reduction, loss, (hipStream_t) stream),
        launch_loss_reduce<double>(full, ali, (int) p->B, reduction, loss, (hipStream_t) stream)));
}

int asg_loss_forward_only(asg_ctx *ctx, const asg_problem *p, void *state, size_t state_bytes, int reduction,
                          void *loss, void *scores, size_t scores_bytes, int flags, void *stream) {
    if (reduction < 0 || reduction > 2 || !loss || !scores) return ASG_ERR_INVALID;
    int rc = check_problem(p, true);
    if (rc) return rc;
    const size_t e = p->dtype == ASG_DTYPE_F64 ? 8 : 4;
    if (scores_bytes < asg_loss_forward_only_scores_bytes(p)) return ASG_ERR_WORKSPACE;
    const bool in_kernel = small_full(p->N) && small_aligned(p->S);
    if (!in_kernel) {
        if (!state) return ASG_ERR_INVALID;
        if (state_bytes < asg_state_bytes(p)) return ASG_ERR_WORKSPACE;
    } else {
        state = nullptr;
    }
    char *sc = (char *) scores;
    void *full = sc, *ali = sc + (size_t) p->B * e;
    unsigned *ticket = (unsigned *) (sc + align_up(2 * (size_t) p->B * e));
    flags &= ~ASG_FLAG_ALPHA_SCORES;
    rc = ASG_DISPATCH(p,
        run_forward<float>(ctx, p, state, full, ali, kFullBeta | kAlignedBeta, false, flags, (hipStream_t) stream, loss, reduction, ticket),
        run_forward<double>(ctx, p, state, full, ali, kFullBeta | kAlignedBeta, false, flags, (hipStream_t) stream, loss, reduction, ticket));
    if (rc || in_kernel) return rc;
    return hip_status(ASG_DISPATCH(p,
        launch_loss_reduce<float>(full, ali, (int) p->B, reduction, loss, (hipStream_t) stream),
        launch_loss_reduce<double>(full, ali, (int) p->B, reduction, loss, (hipStream_t) stream)));
}

int asg_loss_backward(asg_ctx *ctx, const asg_problem *p, const void *state, size_t state_bytes, int reduction,
                      const void *grad_loss, void *scratch, size_t scratch_bytes, void *grad_transition,
                      void *grad_inputs, int flags, void *stream) {
    (void) ctx; (void) flags;
    int rc = check_problem(p, true);
    if (rc) return rc;
    if (reduction < 0 || reduction > 2) return ASG_ERR_INVALID;
    if (!state || !grad_loss || !scratch || !grad_transition || !grad_inputs) return ASG_ERR_INVALID;
    if (state_bytes < asg_state_bytes(p)) return ASG_ERR_WORKSPACE;
    const int gstride = reduction == 0 ? 1 : 0;
    const double gscale = reduction == 2 ? 1.0 / (double) p->B : 1.0;
    return ASG_DISPATCH(p,
        run_backward<float>(p, state, grad_loss, nullptr, scratch, scratch_bytes, grad_transition, grad_inputs, 3, (hipStream_t) stream, gstride, gscale, 1),
        run_backward<double>(p, state, grad_loss, nullptr, scratch, scratch_bytes, grad_transition, grad_inputs, 3, (hipStream_t) stream, gstride, gscale, 1));
}

/* ---- fused training step (asg_fused.hip) ------------------------------------------------------------------ */

namespace {
struct FusedLayout { size_t tiles, flags, dump, ticket2, p2, edges, ascore, fscore, xstate, aoff, rows, in32, total; };
FusedLayout fused_layout(const asg_problem *p) {
    FusedLayout L{};
    size_t off = 0;
    L.tiles = off; off = align_up(off + (size_t) p->B * 2 * p->N * p->N * 4);
    L.flags = off; off = align_up(off + (size_t) p->B * 4);
    L.dump = off; off = align_up(off + (size_t) p->B * 3 * 4);
    L.ticket2 = off; off = align_up(off + 256);
    L.p2 = off; off = align_up(off + (size_t) p->B * 2 * (p->T + 8) * (p->S < 1 ? 1 : p->S) * 4);
    L.edges = off; off = align_up(off + (size_t) p->B * 2 * 3 * 128 * 8);
    L.ascore = off; off = align_up(off + (size_t) p->B * 8);
    L.fscore = off; off = align_up(off + (size_t) p->B * 8);
    L.xstate = off; off = align_up(off + (size_t) p->B * 2 * ((p->T + 7) / 8 + 2) * 2048);
    L.aoff = off; off = align_up(off + (size_t) p->B * 2 * ((p->T + 15) / 16 + 1) * 2 * 8);
    if (p->inputs_dtype == ASG_DTYPE_BF16) {
        L.rows = off; off = align_up(off + (size_t) p->T * p->B * p->N * 4);
        L.in32 = off; off = align_up(off + (size_t) p->T * p->B * p->N * 4);
    }
    L.total = off;
    return L;
}
FusedArgs fused_args(const asg_problem *p, void *scratch, int reduction) {
    const FusedLayout L = fused_layout(p);
    char *base = (char *) scratch;
    FusedArgs F{};
    F.tiles = base + L.tiles;
    F.flags = (int *) (base + L.flags);
    F.dump = base + L.dump;
    F.ticket2 = (unsigned *) (base + L.ticket2);
    F.p2 = base + L.p2;
    F.edges = base + L.edges;
    F.ascore = base + L.ascore;
    F.fscore = base + L.fscore;
    F.xstate = base + L.xstate;
    F.aoff = base + L.aoff;
    if (p->inputs_dtype == ASG_DTYPE_BF16) { F.rows = base + L.rows; F.in32 = base + L.in32; }
    F.reduction = reduction;
    F.gscale = reduction == 2 ? (float) (1.0 / (double) p->B) : 1.0f;
    return F;
}
}  // namespace

int asg_loss_fused_supported(const asg_problem *p) {
    if (check_problem(p, true, true) != ASG_OK) return 0;
    if (p->dtype != ASG_DTYPE_F32 || p->N >= 64 || p->S > 64) return 0;
    const double fr = (double) (p->T - 1) * (double) p->inputs_strides[0] * 4.0, ln = 63.0 * (double) p->inputs_strides[2] * 4.0;
    if (p->inputs_strides[0] < 0 || p->inputs_strides[2] < 0 || fr >= 4294967296.0 || ln >= 2147483648.0) return 0;
    if ((double) p->T * (double) p->B * (double) p->N * 4.0 >= 4294967296.0) return 0;
    if (p->T > 4000) return 0;              // per-block offset tables of the aligned finishers (asg_fused.hip: kMaxBlk)
    return 1;
}

size_t asg_loss_fused_scratch_bytes(const asg_problem *p) {
    if (!p || p->T < 1 || p->B < 1 || p->N < 1) return 0;
    return fused_layout(p).total;
}

size_t asg_loss_fused_sync_bytes(const asg_problem *p) {
    if (!p || p->B < 1) return 0;
    return align_up(256 + (size_t) p->B * 64);
}

int asg_loss_fused_forward(const asg_problem *p, void *state, size_t state_bytes, int reduction, void *loss, void *scores,
                           void *scratch, size_t scratch_bytes, void *grad_inputs, void *sync, int flags, void *stream) {
    (void) flags;
    if (reduction < 0 || reduction > 2 || !loss || !scores || !scratch || !grad_inputs || !sync || !state) return ASG_ERR_INVALID;
    if (!asg_loss_fused_supported(p)) return check_problem(p, true, true) != ASG_OK ? check_problem(p, true, true) : ASG_ERR_UNSUPPORTED;
    if (state_bytes < asg_state_bytes(p) || scratch_bytes < asg_loss_fused_scratch_bytes(p)) return ASG_ERR_WORKSPACE;
    FusedArgs F = fused_args(p, scratch, reduction);
    F.loss = loss;
    F.scores = scores;
    F.grad_inputs = grad_inputs;
    if (!F.rows) F.rows = grad_inputs;
    F.sync = (unsigned *) sync;
    return hip_status(launch_fused_forward(to_problem(p), to_state(p, state), F, (hipStream_t) stream));
}

int asg_loss_fused_backward(const asg_problem *p, void *state, size_t state_bytes, int reduction, const void *grad_loss,
                            void *scratch, size_t scratch_bytes, void *grad_inputs, void *grad_transition, int flags,
                            void *stream) {
    (void) flags;
    if (reduction < 0 || reduction > 2 || !grad_loss || !scratch || !grad_inputs || !grad_transition || !state) return ASG_ERR_INVALID;
    if (!asg_loss_fused_supported(p)) return check_problem(p, true, true) != ASG_OK ? check_problem(p, true, true) : ASG_ERR_UNSUPPORTED;
    if (state_bytes < asg_state_bytes(p) || scratch_bytes < asg_loss_fused_scratch_bytes(p)) return ASG_ERR_WORKSPACE;
    FusedArgs F = fused_args(p, scratch, reduction);
    F.grad_inputs = grad_inputs;
    if (!F.rows) F.rows = grad_inputs;
    F.grad_loss = grad_loss;
    F.grad_transition = grad_transition;
    return hip_status(launch_fused_backward(to_problem(p), to_state(p, state), F, (hipStream_t) stream));
}

}  // extern "C"
