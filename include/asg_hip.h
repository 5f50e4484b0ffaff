/* include/asg_hip.h -- C ABI of libasg_hip.so: the MI355X (gfx950) ASG forward-backward hot path.
 *
 * Drop-in boundary for the native layer of zh217/torch-asg.  The reference binds its native code
 * through a pybind11 module `torch_asg_native` with seven functions
 * (/root/reference/torch_asg/native/extension.cpp:15-29); each entry point below names the one it
 * replaces.  Differences from the reference ABI, by design:
 *   - plain C: raw DEVICE pointers, explicit element strides, explicit sizes, explicit stream;
 *     no torch / ATen / pybind types anywhere;
 *   - the CALLER owns every buffer (state, scratch, outputs); the library never allocates device
 *     memory and never touches the thread's current stream;
 *   - no path_contrib tensors: the O(T*B*N*N) buffer of fully_connected_lattice.cpp:77 is never
 *     materialised -- the saved state is O(T*B*(N+S));
 *   - returns an int status (0 = ok) instead of throwing.
 *
 * All device pointers must be valid on the current HIP device.  Lengths/targets are int64
 * (the reference asserts kLong: utils.cpp:28,46).  `dtype` selects float32 / float64 for every
 * floating-point buffer of the call (utils.h:33-39 dispatch).
 */
#ifndef ASG_HIP_H
#define ASG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASG_HIP_VERSION 230

#define ASG_DTYPE_F32 0
#define ASG_DTYPE_F64 1
#define ASG_DTYPE_BF16 2            /* only as asg_problem::inputs_dtype (see there) */

/* status codes */
#define ASG_OK 0
#define ASG_ERR_INVALID 1       /* null pointer / bad dtype / negative size */
#define ASG_ERR_UNSUPPORTED 2   /* shape outside what this build supports */
#define ASG_ERR_WORKSPACE 3     /* state/scratch buffer too small */
#define ASG_ERR_HIP_BASE 1000   /* 1000 + hipError_t */

/* flags */
#define ASG_FLAG_STREAMS 1          /* run the full-lattice and force-aligned passes on two HIP streams
                                       (the reference's multi-stream route, streamlined_fast_gpu.cpp:104-230);
                                       without it everything is issued on `stream` in order
                                       (= ASGLoss(gpu_no_stream_impl=True), asg.py:124) */
#define ASG_FLAG_SINGLE_LAUNCH 2    /* all four recursions in ONE kernel launch (blockIdx.y = pass) */
#define ASG_FLAG_ALPHA_SCORES 8     /* debugging: forward also writes the scores obtained from the alpha passes
                                       into full_scores[B..2B) / aligned_scores[B..2B) */

/* One batch of utterances, as the reference's ASGLoss.forward receives it (asg.py:109). */
typedef struct asg_problem {
    const void *inputs;            /* [T,B,N] emissions (time-major), element strides below       */
    int64_t inputs_strides[3];
    const void *transition;        /* [N,N]; transition[i][j] = score of going from label j to i  */
    int64_t transition_strides[2];
    const int64_t *targets;        /* [B,S] int64                                                  */
    int64_t targets_strides[2];
    const int64_t *input_lengths;  /* [B] int64, or NULL = all T   (asg.py:116-117)               */
    const int64_t *target_lengths; /* [B] int64, or NULL = all S   (asg.py:113-114)               */
    int64_t T, B, N, S;
    int32_t dtype;                 /* ASG_DTYPE_*                                                  */
    int32_t inputs_dtype;          /* 0: emissions have `dtype`.  ASG_DTYPE_BF16 (with dtype = ASG_DTYPE_F32): emissions are
                                      bfloat16, everything else float32 (bf16 in, fp32 accumulate), and grad_inputs
                                      comes back as bfloat16.  Accepted by the asg_loss_fused_* pair only. */
} asg_problem;

/* Opaque context: the side stream + fork/join events of ASG_FLAG_STREAMS -- host handles only, no device memory and
 * no per-call state (the reference keeps none either: it borrows streams from the CUDA stream pool,
 * streamlined_fast_gpu.cpp:121-129).  Calls that use the SAME context are ordered through its events, so use one
 * context per calling stream (or thread); everything else in this library is re-entrant: whatever a call mutates on
 * the device lives in the buffers the caller passed to that call. */
typedef struct asg_ctx asg_ctx;

int asg_hip_version(void);
const char *asg_hip_strerror(int status);

/* Fault report (no reference counterpart): how many launches of the resident-slice forward kernel (256 < N <= 2048 in fp32, <= 1024 in
 * fp64: a grid of co-resident workgroups that wait for each other) of THIS process ran out of their bounded waits -- part of the grid
 * never became resident.  Such a call is REPAIRED IN STREAM: the launch raises a word in the call's own work area, and a repair kernel
 * that the same call enqueued behind it redoes the full-lattice recursion with no dependence between workgroups (exact; tens of
 * milliseconds; a no-op of ~2 us when nothing timed out) before the scores are computed -- the call's results are right, no NaN, no
 * error at a later call.  From then on the library takes the per-frame launches (no co-residency needed, 2-3x slower): this count is
 * what tells a caller that the fast route is gone.  Read from host-pinned memory, no synchronisation; the count of a call is visible once
 * that call has run. */
unsigned asg_cluster_timeouts(void);

/* Developer / test switches (ASG_FORK_IN_CAPTURE, ASG_PAIR_MIN_B, ASG_BWD_ROWSUM, ASG_NO_CLUSTER, ASG_NO_MID, ASG_NO_TILE_STEP, ASG_STEP_ONE_TILE, ASG_STEP_ROW_BLOCKS, ASG_STEP_FULL_TILE, ASG_STEP_NO_BF3, ASG_STEP_BF3_MIN_B,
 * ASG_ALIGNED_KERNEL) are read from the environment ONCE, at the first call that needs one -- no getenv on the per-call path.
 * A process that changes them afterwards (the test-suite does) calls this to have them read again.  No reference counterpart.
 * NOT for use while another thread is inside a call of this library: a forward call reads the switches more than once (the layout of
 * the operand-order matrices is chosen when they are built and again when they are read), and a reload between the two with another
 * ASG_STEP_* setting would make them disagree.  Each call keeps the previous block of switches alive (readers may still hold it): a few
 * dozen bytes per reload, never freed. */
void asg_reload_env(void);

int asg_ctx_create(asg_ctx **out);
int asg_ctx_destroy(asg_ctx *ctx);

/* *id = the identifier of the hipGraph capture `stream` is recording into, 0 when it is not capturing.  Host bindings
 * use it to give every capture its own `sync` region (asg_loss_fused_forward) without allocating under capture. */
int asg_stream_capture_id(void *stream, unsigned long long *id);

/* Bytes of saved lattice state (forward -> backward) and of backward scratch for a problem shape.
 * Only T,B,N,S,dtype of `p` are read.
 * The backward entry points take the SAME problem as their forward call: `inputs` and `transition` are read again (the
 * gradient pass recomputes the edge posteriors from the saved states and the emissions; nothing like the reference's
 * path_contrib is stored), so both tensors must still hold the values the forward call saw. */
size_t asg_state_bytes(const asg_problem *p);
size_t asg_scratch_bytes(const asg_problem *p);

/* ---- granular entry points: the reference's "serial" route (asg.py:124-128) ------------------- */

/* replaces torch_asg_native.fully_connected_forward (extension.cpp:16, fully_connected_lattice.cpp:65-91):
 * alpha+beta recursions of the fully-connected lattice; scores[B] = S_full. */
int asg_full_forward(const asg_problem *p, void *state, size_t state_bytes, void *scores, int flags, void *stream);

/* replaces torch_asg_native.fully_connected_backward (extension.cpp:17, fully_connected_lattice.cpp:93-105):
 * grad_transition[N,N], grad_inputs[T,B,N] (both contiguous, fully overwritten). */
int asg_full_backward(const asg_problem *p, const void *state, size_t state_bytes, const void *grad_out,
                      void *scratch, size_t scratch_bytes, void *grad_transition, void *grad_inputs, void *stream);

/* replaces torch_asg_native.force_aligned_forward (extension.cpp:18, force_aligned_lattice.cpp:266-319). */
int asg_aligned_forward(const asg_problem *p, void *state, size_t state_bytes, void *scores, int flags, void *stream);

/* replaces torch_asg_native.force_aligned_backward (extension.cpp:19, force_aligned_lattice.cpp:321-356). */
int asg_aligned_backward(const asg_problem *p, const void *state, size_t state_bytes, const void *grad_out,
                         void *scratch, size_t scratch_bytes, void *grad_transition, void *grad_inputs, void *stream);

/* ---- fused entry points: the reference's GPU fast route (asg.py:129-136) ---------------------- */

/* replaces torch_asg_native.fast_asg_gpu_forward (extension.cpp:25, streamlined_fast_gpu.cpp:104-230):
 * all four recursions; full_scores[B], aligned_scores[B] ([2B] each with ASG_FLAG_ALPHA_SCORES). */
int asg_forward(asg_ctx *ctx, const asg_problem *p, void *state, size_t state_bytes,
                void *full_scores, void *aligned_scores, int flags, void *stream);

/* replaces torch_asg_native.fast_asg_gpu_forward_only (extension.cpp:23, streamlined_fast_gpu.cpp:24-94):
 * beta recursions only, nothing saved.  `state` is only used as scratch by the large-alphabet path
 * (N > 64: the normalised transition matrices live there); it may be NULL when N <= 64 and S <= 64. */
int asg_forward_only(asg_ctx *ctx, const asg_problem *p, void *state, size_t state_bytes,
                     void *full_scores, void *aligned_scores, int flags, void *stream);

/* replaces torch_asg_native.fast_asg_gpu_backward (extension.cpp:27, streamlined_fast_gpu.cpp:236-297):
 * non-recursive gradient assembly for loss-side gradients grad_full[B], grad_aligned[B]. */
int asg_backward(asg_ctx *ctx, const asg_problem *p, const void *state, size_t state_bytes,
                 const void *grad_full, const void *grad_aligned, void *scratch, size_t scratch_bytes,
                 void *grad_transition, void *grad_inputs, int flags, void *stream);

/* ---- best-path (Viterbi) force alignment -- SURVEY.md 8(f)3.  No counterpart in the reference (README.md:33 lists
 * it as TODO; the lattice is force_aligned_lattice.cpp:84-111 with max instead of logsumexp,
 * doc/tech_report.tex:84-88).  scores[B] (dtype of inputs) = score of the best alignment, path[B][T] int64 = the
 * target POSITION occupied at each frame (-1 for frames >= input_lengths[b], and everywhere when the utterance has
 * no finite alignment: score -inf).  Tied comparisons keep "stay" (so among tied paths the one that advances
 * earliest is returned).  S <= 8192 like the other aligned-lattice entry points (beyond 1024 positions: N <= 38 400 in float32, 19 200 in float64).
 * `work` holds B*T*ceil(S/64) 64-bit back-pointer masks (asg_viterbi_work_bytes). */
size_t asg_viterbi_work_bytes(const asg_problem *p);
int asg_viterbi(asg_ctx *ctx, const asg_problem *p, void *work, size_t work_bytes, void *scores, int64_t *path,
                int flags, void *stream);

/* ---- Viterbi DECODING over the fully-connected lattice: the best label path under the transition matrix, and its tokens
 * (wav2letter's viterbiPath).  No counterpart in the reference (README.md:33 lists Viterbi decoders as TODO).  For utterance b
 * with len = clamp(input_lengths[b], 0, T):
 *   v[0][i] = I[0][b][i];   v[t][i] = (max_j (v[t-1][j] + tr[i][j])) + I[t][b][i]   (1 <= t < len)
 *   scores[b] = max_i v[len-1][i];   path[b][len-1] = argmax_i v[len-1][i];   path[b][t-1] = argmax_j (v[t-1][j] + tr[path[b][t]][j])
 * in the dtype of the problem, adds and maxes only; every argmax takes the smallest index on a tie.  path[b][t] = -1 for
 * t >= len; tokens[b] = path[b][0..len) with consecutive repeats collapsed, padded with -1; token_lengths[b] = their count.
 * len == 0 or no finite path: scores[b] = -inf, path and tokens all -1, token_lengths[b] = 0.
 * scores: [B] (dtype); path, tokens: [B][T] int64; token_lengths: [B] int64.  `targets`, `target_lengths` and `S` are ignored.
 * `work` (asg_viterbi_decode_work_bytes):
 *   resident route (N <= 256 in float32, N <= 128 in float64; one launch): B*T*N bytes of uint8 back-pointers;
 *   streaming route (larger N; one launch per frame): align256(P*P*e) + T*B*P*e bytes, P = N rounded up to 64, e = 4 or 8
 *   (the transposed transition matrix, then every frame's Viterbi vector).
 * Every output is written by kernels (no memset), so a captured call replays with new inputs.  Limits: T, B <= 2^30,
 * N <= 2^22 (ASG_ERR_UNSUPPORTED beyond); every index is 64-bit, so none of the loss's 32-bit state-offset limits apply. */
size_t asg_viterbi_decode_work_bytes(const asg_problem *p);
int asg_viterbi_decode(asg_ctx *ctx, const asg_problem *p, void *work, size_t work_bytes, void *scores, int64_t *path,
                       int64_t *tokens, int64_t *token_lengths, int flags, void *stream);

/* ---- Viterbi decoding over the ASG lattice COMPOSED with a deterministic weighted automaton over tokens (a token-level
 * language model).  The product graph is compiled by the caller (torch_asg_amd.TokenGraph.compile): Q product states
 * q = (label i, automaton state s'), one per pair for which some arc s --i--> s' exists, numbered in (s', i) order; per target q
 * a CSR row of incoming edges from every q' = (j, s) with j != i and s --i--> s', ascending by source index.  For utterance b
 * with len = clamp(input_lengths[b], 0, T), in the dtype of the problem, adds and maxes only:
 *   v[0][q] = start_w[q] + I[0][i]
 *   v[t][q] = best(stay: v[t-1][q] + tr[i][i];  edge e from q': (v[t-1][q'] + tr[i][src_label[e]]) + edge_w[e]) + I[t][i]
 *   scores[b] = max_q (v[len-1][q] + final_w[q])
 * "best" is the largest value, the smallest source index on a tie (the stay's source is q); the final max takes the smallest q.
 * path[b][t] = label of the winning q at frame t, states[b][t] = its automaton state; tokens / token_lengths collapse the path as
 * asg_viterbi_decode does.  Integer outputs are int64 [B][T] (token_lengths [B]) padded with -1; len == 0 or no finite path:
 * score -inf, all -1, no tokens.  Every output is written by kernels (no memset), so a captured call replays with new inputs.
 * `work` (asg_viterbi_decode_graph_work_bytes, the same on both routes): align256(T*B*Q*4) + 2*Q*B*e bytes (e = 4 or 8):
 * int32 back-pointers, then the streaming route's Viterbi vectors (the resident route leaves them untouched).
 *   resident route (2*(Q+N)*e <= 128 KiB, N <= 1024 and E <= 32768): one launch, one workgroup per utterance, both vectors
 *   in LDS;  streaming route (otherwise, or ASG_FLAG_DECODE_GRAPH_STREAMING): one launch per frame, then one backtrace launch.
 * Limits (ASG_ERR_UNSUPPORTED beyond): Q, E < 2^31, N <= 2^16, B <= 2^22, T <= 2^30.  The graph is read as given: src and
 * src_label must hold valid indices (nothing is validated on the device). */
#define ASG_FLAG_DECODE_GRAPH_STREAMING 16   /* asg_viterbi_decode_graph: take the streaming route even where the resident one
                                                would be chosen (both routes give bit-identical results; for tests) */
#define ASG_FLAG_DECODE_GRAPH_RESIDENT 32    /* ... and the resident route wherever the graph fits it (for tests and timings) */
typedef struct asg_token_graph {
    int64_t Q;                     /* product states                                                   */
    int64_t E;                     /* incoming edges, the stay excluded                                */
    int32_t N;                     /* alphabet size (= the problem's N)                                */
    int32_t dtype;                 /* ASG_DTYPE_F32 / ASG_DTYPE_F64 of the weights (= the problem's)   */
    const int32_t *label;          /* [Q] label i of q                                                 */
    const int32_t *state;          /* [Q] automaton state s' of q                                      */
    const int32_t *row;            /* [Q+1] CSR offsets of the incoming edges of q                     */
    const int32_t *src;            /* [E] source product state of each edge, ascending within a row    */
    const int32_t *src_label;      /* [E] label of that source                                         */
    const void *start_w;           /* [Q] folded weight of the start arc into q, -inf if none          */
    const void *final_w;           /* [Q] folded final weight of q's automaton state, -inf if none     */
    const void *edge_w;            /* [E] folded arc weight of each edge                               */
} asg_token_graph;
size_t asg_viterbi_decode_graph_work_bytes(const asg_problem *p, const asg_token_graph *g);
int asg_viterbi_decode_graph(asg_ctx *ctx, const asg_problem *p, const asg_token_graph *g, void *work, size_t work_bytes,
                             void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                             int flags, void *stream);

/* ---- BEAM-PRUNED Viterbi decoding over the same composed lattice: asg_viterbi_decode_graph with at most beam_size product
 * states kept per frame.  Work per frame is proportional to the kept states and their outgoing edges, never to Q or E, and the
 * back-pointers are T*B*K instead of T*B*Q.  No counterpart in the reference.  The search is specified, not approximate.
 * Product states, start_w, final_w, edge weights and the clamping of input_lengths are those of asg_viterbi_decode_graph; all
 * arithmetic is in the dtype of the problem (beam_threshold rounded to it): adds, one subtraction and comparisons.  For utterance
 * b with len = clamp(input_lengths[b], 0, T), an active set A_t of product states with values v_t:
 *   t = 0:  c[q] = start_w[q] + I[0][i(q)] for every q.
 *   t >= 1: candidates come only from sources in A_{t-1}: the stay v_{t-1}[q] + tr[i][i] when q is active (its source is q), and
 *           (v_{t-1}[q'] + tr[i][j]) + edge_w for every edge q' -> q with q' active; best[q] = the largest candidate, the smallest
 *           source index on a tie; c[q] = best[q] + I[t][i].  A q without a candidate, or with c[q] = -inf, is no candidate state.
 *   prune (every frame, t = 0 included): m = max_q c[q], lo = fl(m - beam_threshold) (-inf for +inf).  With the candidate states
 *           ordered by (c descending, q ascending), A_t = the first beam_size of them that also have c[q] >= lo; v_t = c there.
 *           No candidate state: A_t is empty and stays empty.
 *   end:    scores[b] = max over q in A_{len-1} of (v[q] + final_w[q]), the smallest q on a tie; path, states, tokens and
 *           token_lengths follow the back-pointers as in asg_viterbi_decode_graph.  len == 0, an empty last set, or no active
 *           state with a finite final_w: score -inf, integer outputs -1, no tokens.
 * NaN anywhere and +inf emissions are unspecified.  -0 and +0 compare equal in every rule above.  With beam_size >= Q and
 * beam_threshold = +inf every output equals asg_viterbi_decode_graph's; for any beam the score is <= the exact one and, when
 * finite, is exactly the score of the returned path.  Results are bit-identical run to run (integer atomics only).
 * The graph from the SOURCE side (torch_asg_amd.TokenGraph.compile_beam): per product state q' a CSR row of its outgoing edges,
 * ascending by target, each with {target q, label of q} as one pair of int32 and the folded arc weight beside it (the same edges
 * as asg_token_graph's, regrouped); start_q lists the q with start_w[q] > -inf, ascending, so that frame 0 does not scan Q;
 * max_out is the largest out-degree (it sizes the list of targets a frame can touch).
 * K = min(beam_size, max(Q, 1)).  `work` (asg_beam_decode_graph_work_bytes), per utterance and every part rounded up to 256 bytes:
 *   2 * T*K*4 (product state and source slot of every kept state) + Q*8 + Q*e (one best-candidate slot per product state, emptied
 *   by the kernel as it goes) + cap*(e + 4) (the targets touched in a frame), cap = max(min(Q, K*(max_out+1)), num_start), e = 4 / 8.
 * One launch, one workgroup per utterance; every output and all scratch is written by the kernel (no memset), so a captured call
 * replays with new inputs.  Limits (ASG_ERR_UNSUPPORTED beyond): those of asg_viterbi_decode_graph, and K <= 8192 (a beam_size
 * above Q is treated as Q).  beam_size < 1, a negative or NaN beam_threshold: ASG_ERR_INVALID.  `flags` is reserved (pass 0). */
typedef struct asg_token_graph_beam {
    const asg_token_graph *graph;  /* the product graph (label, state, start_w, final_w are read; Q, E, N, dtype)  */
    int64_t num_start;             /* entries of start_q                                                         */
    int32_t max_out;               /* largest out-degree of a product state, the stay excluded                   */
    int32_t reserved;
    const int32_t *orow;           /* [Q+1] CSR offsets of the outgoing edges of q'                              */
    const int32_t *oarc;           /* [E][2] {target q, label of q} of each outgoing edge, targets ascending within a row */
    const void *ow;                /* [E] folded arc weight of each outgoing edge                                */
    const int32_t *start_q;        /* [num_start] product states with start_w > -inf, ascending                  */
} asg_token_graph_beam;
size_t asg_beam_decode_graph_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, int beam_size);
int asg_beam_decode_graph(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, int beam_size, double beam_threshold,
                          void *work, size_t work_bytes, void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                          int64_t *states, int flags, void *stream);

/* ---- The N BEST final hypotheses of that beam search, each with its score split into an acoustic and a graph part: what an
 * n-best rescoring pass and the tuning of lm_weight / token_score need.  No counterpart in the reference.  The token automaton
 * is deterministic, so a token sequence determines its product state and two survivors of the last frame always carry different
 * transcripts: the n best final states are n distinct hypotheses, each the best path the pruned search found for its state.
 * For utterance b with len = clamp(input_lengths[b], 0, T), the search of asg_beam_decode_graph runs unchanged (the same
 * beam_size, beam_threshold, folding and dtype; the same device code).  A = A_{len-1} with values v; end[q] = v[q] + final_w[q].
 * The candidates are the q in A with end[q] > -inf, ordered by end descending, then q ascending (-0 and +0 are equal).
 *   num_hyps[b] = min(nbest, number of candidates): 0 for len == 0, an empty last set, or no finite end.
 *   For r < num_hyps[b], with q_0 .. q_{len-1} the back-pointer path of the r-th candidate, i_t and s_t the label and the
 *   automaton state of q_t:
 *     scores[b][r] = end of that candidate;  path[b][r][t] = i_t;  states[b][r][t] = s_t;  tokens[b][r] and token_lengths[b][r]
 *     the collapse of the path as in asg_viterbi_decode.
 *     emission_scores[b][r], adds only, in frame order: a = I[0][i_0]; for t >= 1: a = (a + tr[i_t][i_{t-1}]) + I[t][i_t] (the
 *     stay uses tr[i][i]).
 *     graph_scores[b][r] likewise: g = start_w[q_0]; for every t >= 1 with q_t != q_{t-1}, in order, g = g + edge_w(q_{t-1} ->
 *     q_t), the folded arc weight (an edge never joins a state to itself -- its labels differ -- so q_t == q_{t-1} is always the
 *     stay); last g = g + final_w[q_{len-1}].
 *   Rows r >= num_hyps[b] are padding: the three scores -inf, every integer output -1, token_lengths 0.  Frames t >= len: -1.
 *   scores, emission_scores, graph_scores [B][nbest] in the dtype of the problem; path, tokens, states [B][nbest][T] int64;
 *   token_lengths [B][nbest] int64; num_hyps [B] int64.  path and states may be NULL: they are then not written.
 * Row 0 equals asg_beam_decode_graph's five outputs bit for bit (the same ordering rule).  scores is the search's own sum and
 * not fl(emission_scores + graph_scores) -- the additions happen in another order -- but the two differ by no more than
 * (3*len + 2) * eps * (the sum of the magnitudes of the terms on the path).
 * K = min(beam_size, max(Q, 1)), nb = min(nbest, K).  `work` (asg_beam_decode_graph_nbest_work_bytes), every part rounded up to 256 bytes:
 *   B * (asg_beam_decode_graph's bytes per utterance + (8 + K*e) (the size and the values of the last set) + T*nb*4 (the
 *   product states of every hypothesis)) + 2*B*8 + 3*B*T*8 (what the search itself returns), e = 4 / 8.
 * Two launches on one stream, one workgroup per utterance each; every output, padding row and scratch word that is read is
 * written by a kernel (no memset, no copy, no synchronisation), so a captured call replays with new emissions and lengths.
 * Results are bit-identical run to run (no float atomics).  nbest < 1: ASG_ERR_INVALID; nbest > 8192: ASG_ERR_UNSUPPORTED;
 * everything else as for asg_beam_decode_graph.  `flags` is reserved (pass 0). */
size_t asg_beam_decode_graph_nbest_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, int beam_size, int nbest);
int asg_beam_decode_graph_nbest(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, int beam_size,
                                double beam_threshold, int nbest, void *work, size_t work_bytes, void *scores,
                                void *emission_scores, void *graph_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                                int64_t *states, int64_t *num_hyps, int flags, void *stream);

/* ---- STREAMING beam decoding: the search of asg_beam_decode_graph carried across chunks of frames, for a service that receives
 * an utterance a few frames at a time, shows a transcript while it is still arriving and needs the final one a chunk after the
 * last frame, without a second search over everything.  No counterpart in the reference.
 * A STREAM STATE is one device buffer that serves B utterance slots, for a fixed graph, dtype, K = min(beam_size, max(Q, 1)) and
 * max_frames (every call on a state passes the same gb, B, beam_size and max_frames).  Per slot it holds: pos, the frames
 * consumed so far; the active set A_{pos-1} with its values; the back-pointers (product state, source slot) of the frames
 * 0 .. pos-1; a sticky overflow word; and the slot arrays of the search (best-candidate slot per product state, touched list,
 * keys).  The contents are opaque; a state must be reset before its first use.
 *   asg_beam_stream_reset: for every slot b with mask[b] != 0 (one byte per slot on the device; NULL: every slot): pos = 0, the
 *     set empty, overflow = 0, and the best-candidate slots of all Q product states emptied (the only place where those Q
 *     entries are written: a frame empties what it touched).  Written by a kernel.
 *   asg_beam_stream_advance: p->inputs is a chunk [Tc = p->T, B, N] (any strides) and p->input_lengths the chunk's lengths (NULL:
 *     Tc for every slot); p->transition and beam_threshold are used for the frames of this call (they may differ between calls).
 *     For slot b: n = min(clamp(input_lengths[b], 0, Tc), max_frames - pos).  If the bound by max_frames cut anything, overflow = 1;
 *     the frames beyond it are not consumed and nothing is written out of bounds.  The chunk's frames 0 .. n-1 are the frames
 *     pos .. pos+n-1 of the utterance and run exactly the rules of asg_beam_decode_graph -- the same adds in the same order,
 *     the same tie rules, the same prune; the same device code: frame 0 of the utterance takes its candidates from start_w, every
 *     other frame -- the first frame of a chunk included -- from the stored set; an empty set stays empty.  Then pos += n.
 *     Nothing is written besides the state.  Tc = 0 is allowed and changes nothing.
 *   asg_beam_stream_result: reads the state and does not modify it; it may be called after any chunk, and the stream continues.
 *     With L = pos and A = A_{L-1} with values v:  final != 0: end[q] = v[q] + final_w[q];  final == 0: end[q] = v[q], the best
 *     PREFIX hypothesis, without a final weight.  The winner is the q in A with the largest end > -inf, the smallest q on a tie
 *     (-0 and +0 are equal).  scores [B] (dtype) = its end; path, tokens, states [B][max_frames] int64 follow its back-pointers
 *     as in asg_beam_decode_graph, -1 behind the data; token_lengths [B]; frames [B] = L; status [B] = the overflow word (0 / 1).
 *     L == 0, an empty set or no finite end: score -inf, path / tokens / states all -1, token_lengths 0.
 * REQUIRED PROPERTY.  Take a slot that was reset and then advanced by any sequence of chunks that concatenate to x[0:L],
 * L <= max_frames (chunks of no frames included).  asg_beam_stream_result(final = 1) then equals asg_beam_decode_graph on x with
 * T >= L frames, input_length = L, the same transition, beam_size, beam_threshold, folding and dtype: scores and token_lengths bit
 * for bit; path, tokens and states equal on the columns < T and -1 elsewhere.  No tolerance: the search never looks ahead.
 * State (asg_beam_stream_state_bytes; 0 for arguments that the calls refuse), every part rounded up to 256 bytes:
 *   B * (asg_beam_decode_graph's bytes per utterance with T = max_frames + 256 (pos, set size, overflow) + K*(e + 4) (the stored
 *   set: values, then product states)), e = 4 / 8.  The back-pointers keep asg_beam_decode_graph's [frame][K] layout.
 * Each call is ONE launch on `stream`, one workgroup per slot for advance and result: no host synchronisation, no copy, no
 * memset, so a captured call replays with new chunk contents and lengths, and a capture is one linear chain.  Integer atomics
 * only: bit-identical run to run.  Limits: those of asg_beam_decode_graph with T = max_frames (K <= 8192, ...; ASG_ERR_UNSUPPORTED
 * beyond); max_frames < 1, Tc < 0, B < 1, beam_size < 1, a negative or NaN beam_threshold, dtype not the graph's:
 * ASG_ERR_INVALID; a state buffer smaller than asg_beam_stream_state_bytes: ASG_ERR_WORKSPACE.  `flags` is reserved (pass 0). */
size_t asg_beam_stream_state_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t max_frames);
int asg_beam_stream_reset(asg_ctx *ctx, const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t max_frames, void *state,
                          size_t state_bytes, const uint8_t *mask, int flags, void *stream);
int asg_beam_stream_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, int beam_size,
                            double beam_threshold, int64_t max_frames, void *state, size_t state_bytes, int flags, void *stream);
int asg_beam_stream_result(asg_ctx *ctx, const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t max_frames,
                           const void *state, size_t state_bytes, int final, void *scores, int64_t *path, int64_t *tokens,
                           int64_t *token_lengths, int64_t *states, int64_t *frames, int64_t *status, int flags, void *stream);

/* ---- WINDOWED streaming beam decoding: the stream above in BOUNDED memory, for an open microphone, a meeting, a broadcast --
 * utterances without a max_frames.  The search is asg_beam_stream_advance's (the same device code, the same sets and scores bit
 * for bit); the back-pointers are kept only for a window of W frames, in a ring, and the prefix of the transcript on which all
 * surviving hypotheses agree is COMMITTED: returned by the advance that finds it, never to change.  No counterpart in the reference.
 * A WINDOW STREAM STATE serves B slots, for a fixed graph, dtype, K = min(beam_size, max(Q, 1)), window W >= 1 and commit period P,
 * 1 <= P <= W (every call on a state passes the same gb, B, beam_size, W and P).  Per slot it holds: pos (int64), the frames
 * consumed so far -- unbounded; base (int64), the frames committed so far, base <= pos; the stored set A_{pos-1} with its values;
 * bq / bs int32 [W][K], the back-pointers (product state, source slot) of frame u in row u mod W (computed in 64 bits); carry
 * (int32), the label of the last committed frame or -1; a sticky status word; and the slot arrays of the search as in
 * asg_beam_stream_*.  The contents are opaque; a state must be reset before its first use.
 *   asg_beam_window_reset: as asg_beam_stream_reset, and base = 0, carry = -1, status = 0 for the chosen slots.
 *   asg_beam_window_advance: p->inputs is a chunk [Tc = p->T, B, N], p->input_lengths the chunk's lengths, p->transition and
 *     beam_threshold those of this call, as for asg_beam_stream_advance.  For slot b, n = clamp(input_lengths[b], 0, Tc) -- there
 *     is no other bound.  The chunk's frames are the frames pos .. pos+n-1 of the utterance and run exactly as in
 *     asg_beam_stream_advance (frame 0 from start_w, the first frame of a chunk from the stored set, an empty set stays empty);
 *     the back-pointers of frame u go to row u mod W.  After each frame, with pos now counting it, a COMMIT ATTEMPT runs if
 *     pos mod P == 0 and the set is not empty:
 *       1. Convergence.  R = all slots of A_{pos-1}.  If |R| == 1: c = pos-1.  Otherwise for u = pos-1 down to base+1:
 *          R <- { bs[u][k] : k in R }; the first u at which |R| == 1 gives c = u-1; no such u: no c.  If c exists, the path from
 *          that one slot of frame c back to frame base is committed: the frames base .. c in ascending order, and base = c+1.
 *       2. Forced commit, if afterwards pos - base > W - P (the next P frames could overwrite live rows): F = (pos - base) -
 *          (W - P).  The best prefix state of A_{pos-1} -- largest v, smallest q on a tie, -0 equal to +0: the rule of
 *          asg_beam_stream_result(final = 0) -- is followed back to frame base+F-1; the frames base .. base+F-1 on that path are
 *          committed, base += F and status |= 1.
 *     Committing a frame with product state q appends label[q] to new_path and state[q] to new_states at the next free column of
 *     this call's output row; if label[q] != carry it appends the label to new_tokens; then carry = label[q] (the collapse of
 *     asg_viterbi_decode, carried across calls).  After an attempt pos - base <= W - P, between attempts pos - base <= W: no live
 *     row is ever overwritten.  Then pos += n.
 *     Outputs: new_path, new_states, new_tokens int64 [B][W + Tc] (committed <= (pos - base before the call) + n <= W + Tc), -1
 *     behind the data; new_frames [B], the frames this call committed; new_token_lengths [B].  Every element is written by the
 *     kernel.  Tc = 0 is allowed and writes the empty outputs.
 *   asg_beam_window_result: reads the state only; the stream goes on.  The winner is chosen as in asg_beam_stream_result (final
 *     != 0: v + final_w; final == 0: v; the smallest q on a tie).  scores [B]; path, states, tokens int64 [B][W], -1 behind the
 *     data: path and states hold the winner's frames base .. pos-1 (the uncommitted TAIL), tokens their collapse started from
 *     carry -- a first tail label equal to carry is no token; token_lengths [B]; frames [B] = pos; committed [B] = base;
 *     status [B]: bit 0 = a forced commit has happened (sticky until the reset), bit 1 = pos >= 1 and the set is empty.  An empty
 *     set or no finite end: score -inf, the tail all -1, token_lengths 0; what was committed stays committed.  The backtrace is at
 *     most W steps, whatever pos.
 * REQUIRED PROPERTIES (no tolerance in any).  1. Search identity: for any chunking of x[0:L], any W and P, result(final = 1).scores
 * equals asg_beam_decode_graph's score on x bit for bit and result(final = 0).scores equals asg_beam_stream_result's: the window
 * never touches the search.  2. Chunk invariance: at equal pos, base, carry, status and the concatenation of everything advance
 * has returned are the same for every chunking, forced commits included -- attempts happen at frame indices, not at call
 * boundaries.  3. Exactness: while status bit 0 is clear and the one-shot score is finite, concat(new_path of all calls) followed
 * by the tail path equals the one-shot path[:L], the same for states, and concat(new_tokens) followed by the tail tokens equals
 * the one-shot tokens[:token_length]; with W - P >= L a forced commit is impossible.  4. With status bit 0 set the outputs are
 * still exactly those specified above: deterministic, the same for every chunking.
 * State (asg_beam_window_state_bytes; 0 for arguments that the calls refuse), every part rounded up to 256 bytes:
 *   B * (asg_beam_decode_graph's bytes per utterance with T = W + 256 (pos, base, set size, carry, status) + K*(e + 4) (the stored
 *   set: values, then product states)), e = 4 / 8: the back-pointers take 2 * W*K*4 bytes, whatever the length of the utterance.
 * Each call is ONE launch on `stream`, one 1024-thread workgroup per slot for advance and result: no host synchronisation, no
 * copy, no memset, so a captured advance is one kernel node and replays with new chunk contents and lengths whatever the number
 * of hardware queues.  Integer atomics only: bit-identical run to run.  Limits: those of asg_beam_decode_graph with T = W (K <=
 * 8192, ...; ASG_ERR_UNSUPPORTED beyond); W < 1, P < 1, P > W, Tc < 0, B < 1, beam_size < 1, a negative or NaN beam_threshold,
 * dtype not the graph's, a NULL output: ASG_ERR_INVALID; a state buffer smaller than asg_beam_window_state_bytes:
 * ASG_ERR_WORKSPACE.  `flags` is reserved (pass 0). */
size_t asg_beam_window_state_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t W, int64_t P);
int asg_beam_window_reset(asg_ctx *ctx, const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t W, int64_t P, void *state,
                          size_t state_bytes, const uint8_t *mask, int flags, void *stream);
int asg_beam_window_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, int beam_size,
                            double beam_threshold, int64_t W, int64_t P, void *state, size_t state_bytes, int64_t *new_path,
                            int64_t *new_states, int64_t *new_tokens, int64_t *new_frames, int64_t *new_token_lengths, int flags,
                            void *stream);
int asg_beam_window_result(asg_ctx *ctx, const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t W, int64_t P,
                           const void *state, size_t state_bytes, int final, void *scores, int64_t *path, int64_t *tokens,
                           int64_t *token_lengths, int64_t *states, int64_t *frames, int64_t *committed, int64_t *status, int flags,
                           void *stream);

/* ---- The N BEST hypotheses of the two streams above: asg_beam_decode_graph_nbest's list from a stream state or a window stream
 * state, which the call only reads -- the same kernel, pointed at the stored set and at the rows the state keeps -- so that a
 * service that rescores the final list needs neither the emissions nor a second search.  Throughout K = min(beam_size, max(Q, 1))
 * and nb = min(nbest, K).  No counterpart in the reference.
 * asg_beam_stream_nbest.  With L = pos and A = A_{L-1} with values v: the candidates and their order are those of
 *   asg_beam_stream_result -- end[q] = v[q] + final_w[q] (final != 0) or v[q] (final == 0, the n best PREFIXES), end > -inf,
 *   descending, q ascending on a tie, -0 equal to +0.  num_hyps [B] = min(nbest, candidates).  Row r < num_hyps: scores [B][nbest]
 *   (dtype) = the candidate's end; path / states int64 [B][nbest][max_frames] follow its back-pointers (either may be NULL: not
 *   written); tokens [B][nbest][max_frames] and token_lengths [B][nbest] the collapse of its path; graph_scores [B][nbest] by
 *   asg_beam_decode_graph_nbest's rule -- start_w of the first state, plus the weight of every edge taken, in frame order, plus
 *   final_w of the last state, WITHOUT that final weight when final == 0.  Padding as there: rows >= num_hyps have scores and
 *   graph_scores -inf, token_lengths 0 and every wide column -1; columns behind the data are -1.  frames [B] = L and status [B] =
 *   the overflow word, as asg_beam_stream_result writes them.  Row 0 equals asg_beam_stream_result(final) bit for bit.
 *   REQUIRED PROPERTY: for any chunking of x[0:L], L <= max_frames, the final != 0 outputs equal asg_beam_decode_graph_nbest's on
 *   x (T >= L frames, input_length = L, the same arguments) bit for bit -- scores, graph_scores, token_lengths, num_hyps; path,
 *   tokens and states on that call's columns and -1 beyond.  The same adds in the same order: no tolerance.
 *   There is no emission_scores: the state keeps no emissions.  A caller who kept the frames has the one-shot call; the others
 *   have scores - graph_scores, which is it up to rounding.
 *   `work` (asg_beam_stream_nbest_work_bytes): B * (max_frames*nb*4 rounded up to 256) bytes; its contents mean nothing between
 *   calls.
 * asg_beam_window_nbest.  The candidates, their order, num_hyps and scores are asg_beam_stream_nbest's at equal pos, bit for bit
 *   (the window's property 1, for every row).  Row r holds the candidate's TAIL: path / states int64 [B][nbest][W] (either may be
 *   NULL) are the frames base .. pos-1 on ITS OWN chain of back-pointers, column t = frame base + t, walked through the ring in at
 *   most W steps; tokens [B][nbest][W] is the collapse of the tail started from carry -- a first tail label equal to carry is no
 *   token -- and token_lengths its count.  The tail may be empty (base == pos, after a commit up to the last frame): the row still
 *   counts, with its score, token_lengths 0 and -1 everywhere.  frames = pos, committed = base and status (bit 0: a forced commit
 *   has happened, bit 1: pos >= 1 and the set is empty) as asg_beam_window_result writes them.  Padding as above.
 *   REQUIRED PROPERTY, while status bit 0 is clear: for EVERY row, everything advance has committed followed by the row's tail
 *   equals the row of asg_beam_stream_nbest at equal pos, for path, states and tokens.  Why: a convergence commit stops at a frame
 *   c at which every survivor of that moment has the same ancestor, so the committed chain is an ancestor chain of every survivor
 *   of that frame, and every later survivor descends from one of those -- each row's full chain begins with exactly what was
 *   committed.  With bit 0 set some frames were committed along the best hypothesis of the moment only; the rows are then still
 *   exactly the chains specified above (deterministic, the same for every chunking), but need not continue the committed prefix.
 *   There is no graph_scores: the edge into frame `base` needs the product state of frame base-1, whose row the ring may
 *   already have overwritten, and the header keeps only its label (carry).  The window state is not widened for it.
 *   `work` (asg_beam_window_nbest_work_bytes): B * (W*nb*4 rounded up to 256) bytes.
 * Each call is ONE launch on `stream`, one 1024-thread workgroup per slot: no host synchronisation, no copy, no memset -- every
 * output element and every scratch word that is read is written by the kernel -- so a captured call replays.  One integer LDS
 * counter, no atomics on values: bit-identical run to run.  LDS: P2(K) * (8 + e) bytes, P2 the power of two >= K.  Errors: those
 * of asg_beam_stream_result / asg_beam_window_result; nbest < 1: ASG_ERR_INVALID; nbest > 8192: ASG_ERR_UNSUPPORTED; a `work`
 * smaller than *_work_bytes: ASG_ERR_WORKSPACE; NULL state, work, scores, graph_scores, tokens, token_lengths, num_hyps, frames,
 * committed or status: ASG_ERR_INVALID.  *_work_bytes returns 0 for arguments the call refuses.  `flags` is reserved (pass 0).
 * Not here: emission_scores from a stream, graph_scores from the window, confidences from any stream.  (The word family's window:
 * asg_beam_word_window_nbest.) */
size_t asg_beam_stream_nbest_work_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t max_frames,
                                        int nbest);
int asg_beam_stream_nbest(asg_ctx *ctx, const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t max_frames,
                          const void *state, size_t state_bytes, int final, int nbest, void *work, size_t work_bytes, void *scores,
                          void *graph_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                          int64_t *num_hyps, int64_t *frames, int64_t *status, int flags, void *stream);
size_t asg_beam_window_nbest_work_bytes(const asg_token_graph_beam *gb, int64_t B, int dtype, int beam_size, int64_t W, int64_t P,
                                        int nbest);
int asg_beam_window_nbest(asg_ctx *ctx, const asg_token_graph_beam *gb, int64_t B, int beam_size, int64_t W, int64_t P,
                          const void *state, size_t state_bytes, int final, int nbest, void *work, size_t work_bytes, void *scores,
                          int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *num_hyps,
                          int64_t *frames, int64_t *committed, int64_t *status, int flags, void *stream);

/* ---- Beam decoding with a LEXICON and a WORD n-gram LM, the LM composed ON THE FLY: the search of asg_beam_decode_graph over
 * pairs (h, q) -- h a history state of a backoff word LM, q a product state of the lexicon automaton -- that exist only while the
 * search holds them.  A static composition would need one slot per (history, product state); this needs none.  No counterpart in
 * the reference.  The search is specified, not approximate.
 * The lexicon: gb is torch_asg_amd.TokenGraph.from_lexicon compiled as for asg_beam_decode_graph with lm_weight 1 (automaton state
 * 0 is the root; a word-end node has its one arc on `separator` to the root); word_of_state[s] is the id of the word that ends at
 * automaton state s, -1 elsewhere.  The LM: H states, state 0 the empty history; row / word / next and lw describe the explicit
 * arcs of each state (word ascending within a row), backoff / bw the backoff (backoff[0] = -1), ew the end of the sentence with the
 * backoff resolved; every weight folded by the caller in the dtype of the problem (lw = fl(fl(lm_weight * logp) + word_score),
 * bw = fl(lm_weight * bow), ew = fl(lm_weight * eos), -inf staying -inf): the device only adds.
 *   step(h, w): a = 0; while w is not in row h: backoff[h] < 0 (or w < 0, or more than 64 backoff steps): rejected; else
 *               a = a + bw[h], h = backoff[h].  Then a = a + lw[arc]: -> (next[arc], a).
 * PAIR ORDER is h ascending, then q ascending; it takes the place of "q ascending" and "the smallest source index" in every
 * rule of asg_beam_decode_graph.  All arithmetic is adds, one subtraction and comparisons in the dtype of the problem; -0 and +0
 * are one value.  For utterance b with len = clamp(input_lengths[b], 0, T), a kept set A_t of pairs with values v_t:
 *   t = 0:  for every q of start_q the pair (start, q) with c = start_w[q] + I[0][i(q)].
 *   t >= 1: from every kept (h, q') with value v and label j: the stay gives (h, q') with v + tr[j][j]; an outgoing edge e to q
 *           with label i != separator gives (h, q) with (v + tr[i][j]) + ow[e]; one with i == separator takes w =
 *           word_of_state[state(q')], (h', a) = step(h, w), and gives (h', q) with ((v + tr[i][j]) + ow[e]) + a.  A rejected step
 *           or a -inf value is no candidate.  Per target pair the largest candidate wins, the smallest source pair on a tie;
 *           c = best + I[t][i].
 *   prune:  asg_beam_decode_graph's rule: m = max c, lo = fl(m - beam_threshold); with the candidate pairs ordered by (c
 *           descending, pair order), A_t = the first beam_size of them that also have c >= lo.
 *   end:    end(h, q) = (v + final_w[q]) + endw, with endw = ew[h] when state(q) is the root, and, when state(q) ends a word w,
 *           endw = a + ew[h'] for (h', a) = step(h, w) (rejected: no end); mid-word there is none.  scores[b] = the largest end
 *           over A_{len-1}, the smallest pair on a tie.  len == 0, an empty last set, or no finite end: score -inf, every integer
 *           output -1, no tokens, no words.
 *   outputs: scores [B] (dtype); path, tokens, states, lm_states, words [B][T] int64, token_lengths, word_lengths [B] int64.
 *           path / tokens / token_lengths / states as asg_beam_decode_graph; lm_states[b][t] = h of the winning path's pair at frame
 *           t; words[b] = the word of every separator edge on the path, in order, then the word of the final step if the path
 *           ends in a word-end node, -1 behind them; word_lengths[b] their count.
 * K = beam_size (no clamp to Q: pairs are not bounded by Q).  `work` (asg_beam_decode_words_work_bytes), per utterance and every
 * part rounded up to 256 bytes:
 *   3 * T*K*4 (product state, LM state and source slot of every kept pair) + C*(16 + e) (an open-addressed table of C slots: key,
 *   best candidate, its source; emptied by the kernel as it goes) + cap*(e + 12) (the pairs touched in a frame),
 *   cap = max(K*(max_out+1), num_start), C = the power of two >= 2*cap, e = 4 / 8.  No term in H, V, A or Q.
 * One launch, one workgroup per utterance; every output and all scratch is written by the kernel (no memset), so a captured call
 * replays with new inputs.  Integer atomics only: bit-identical run to run, whatever the order in which pairs enter the table.
 * Limits (ASG_ERR_UNSUPPORTED beyond): those of asg_viterbi_decode_graph, beam_size <= 8192, and H, Q <= 2^25 (a source pair and
 * its slot are one 64-bit word), A < 2^31.  beam_size < 1, a negative or NaN beam_threshold, an LM of another dtype, start or
 * separator out of range, a NULL array or output: ASG_ERR_INVALID.  Nothing of the graph or the LM is validated on the device.
 * `flags` is reserved (pass 0). */
typedef struct asg_word_lm {
    int64_t H;                     /* history states                                                    */
    int64_t A;                     /* explicit arcs                                                     */
    int64_t V;                     /* words                                                             */
    int64_t S;                     /* automaton states of the lexicon (entries of word_of_state)        */
    int32_t start;                 /* the state after <s>                                               */
    int32_t separator;             /* the token that ends a word                                        */
    int32_t dtype;                 /* ASG_DTYPE_F32 / ASG_DTYPE_F64 of lw, bw, ew (= the problem's)     */
    int32_t reserved;
    const int32_t *row;            /* [H+1] offsets of the arcs of each state                           */
    const int32_t *word;           /* [A] word of each arc, ascending within a row                      */
    const int32_t *next;           /* [A] next state of each arc                                        */
    const int32_t *backoff;        /* [H] backoff state, -1: none                                       */
    const void *lw;                /* [A] folded arc weights                                            */
    const void *bw;                /* [H] folded backoff weights                                        */
    const void *ew;                /* [H] folded end-of-sentence weights, -inf: none                    */
    const int32_t *word_of_state;  /* [S] word that ends at a lexicon state, -1: none                   */
} asg_word_lm;
size_t asg_beam_decode_words_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size);
int asg_beam_decode_words(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size,
                          double beam_threshold, void *work, size_t work_bytes, void *scores, int64_t *path, int64_t *tokens,
                          int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths,
                          int flags, void *stream);

/* ---- BEAM-PRUNED full score over the PAIRS of asg_beam_decode_words, and its gradients: asg_beam_graph_full_forward / _backward
 * with the lattice state widened from a product state to a pair (h, q) -- a normaliser Z_K whose work per frame follows the beam
 * and never H * Q, so a criterion can be trained against what the word decoder searches.  No counterpart in the reference.  Per
 * utterance b, len = clamp(input_lengths[b], 0, T); lexicon graph, folding, start_w, final_w, ow, the LM's folded lw / bw / ew,
 * step(h, w) and PAIR ORDER exactly as in asg_beam_decode_words:
 *   1. Kept sets.  A_t, t = 0 .. len-1, are exactly the sets of pairs asg_beam_decode_words keeps for the same emissions,
 *      transition, lexicon, LM, beam_size, beam_threshold, computed in the dtype of the problem (the same device code runs).  They
 *      are a discrete function of the inputs and constants to the gradient.  No look-ahead (asg_beam_words_full_forward_la, below,
 *      takes the sets of the look-ahead search).
 *   2. Forced pairs (only when p->targets is given).  y = targets[b][:clamp(target_lengths[b], 0, S)] with consecutive equal
 *      labels merged, n = |y|.  The lexicon automaton is walked along y from the start with h = start; on a separator out of a
 *      word-end node (h, a) = step(h, word of the node).  This gives p_k = (h_k, q_k), k = 1 .. n, and
 *      F_t = { p_k : k-1 <= t and n-k <= len-1-t }.  Every F_t is empty when the target has no alignment (target length 0 or
 *      > len), holds a label outside [0, N), a lexicon arc is missing, an LM step is rejected, the path ends mid-word, or the end
 *      final_w[q_n] + endw(p_n) is -inf.  The forced pairs do NOT feed back into the search of step 1.
 *   3. Lattice.  U_t = A_t united with F_t, ascending in pair order, no duplicates.  For p' = (h', q') with label i':
 *        alpha[0][p'] = start_w[q'] + I[0][i']                                         for the start pairs (start, q') in U_0
 *        alpha[t][p'] = lse over p = (h, q) in U_{t-1} with an edge p -> p' of
 *                          ((alpha[t-1][p] + tr[i'][i]) + w(p -> p')) + I[t][i']                                for p' in U_t
 *      The edges are the search's own candidates: the stay (w = 0, the same pair); a lexicon edge e with a label other than the
 *      separator (h' = h, w = ow[e]); a separator edge out of a word-end node ((h', a) = step(h, word of the node), w = ow[e] + a;
 *      a rejected step is no edge).
 *        scores[b] = Z_K = lse over p in U_{len-1} of (alpha[len-1][p] + final_w[q]) + endw(p)
 *      with endw as in asg_beam_decode_words: ew[h] at the root, a + ew[h'] after one more step in a word-end node, no end
 *      mid-word.  Every lse is max-then-sum; the maximum and the sum of a target are integer reductions (the order-preserving key
 *      of a value; exp(c - max) as a 64-bit fixed-point number with 48 fractional bits), so no order of arrival changes a bit.
 *      All candidates -inf gives -inf, never NaN; len == 0 or an empty lattice: -inf.  beta, the label posteriors and the
 *      expected (i, j) counts are the mirror image over the same U_t; grad_inputs [T,B,N] (contiguous, every element written, zero
 *      rows at t >= len) and grad_transition [N,N] as asg_beam_graph_full_backward.  Lexicon, LM and their weights are constants.
 *   4. Z_K >= asg_beam_decode_words' score without targets.  With targets every alignment of the target runs through the F_t, so
 *      Z_K - (aligned score + asg_words_target_scores) >= 0 for ANY beam.  With weights and emissions such that the search's sums
 *      do not round, beam_size at least the number of reachable pairs and beam_threshold = +inf, Z_K equals
 *      asg_graph_full_forward's score on the static composition of the lexicon with the LM.
 * No float atomics (label posteriors and (i, j) counts as in asg_beam_graph_full_backward; utterances added in ascending order):
 * bit-identical run to run.  ASG_FLAG_BEAM_LOSS_ACCUMULATE (backward) continues grad_transition from what it holds, so a batch
 * processed in consecutive groups gives the bits of one call.  Every output and all scratch that is read is written by kernels (no
 * memset, no host synchronisation): both calls can be captured.
 * K = beam_size; nf = min(S, T) when p->targets is given, else 0; M = K + nf; e = 4 / 8.  Every part rounded up to 256 bytes:
 *   work:    asg_beam_words_full_work_bytes(p, gb, lm, beam_size, store) =
 *            B * (asg_beam_decode_words' bytes per utterance + 2*T*4 + 256 + nf*8 + T*M*8 + (store ? T : 2)*M*e)
 *   scratch: asg_beam_words_full_scratch_bytes(p, gb, lm, beam_size) = B * (2*M*e + N*N*8)
 * No term in H, V, A or Q (the search has none either).
 * The forward keeps alpha for the backward with ASG_FLAG_GRAPH_LOSS_KEEP_ALPHA; the backward takes the same problem (targets
 * included: they size the layout), the same beam_size, that work buffer and the scores of that forward.
 * Limits (ASG_ERR_UNSUPPORTED beyond): those of asg_beam_decode_words (beam_size <= 8192, ...), N <= 1024, min(S, T) <= 2048 with
 * targets, T <= 2^20, and M <= (160 KiB - 256) / (16 + e) = 8179 (float32) / 6816 (float64): a frame's lattice set stays in LDS
 * with a 64-bit pair, a 64-bit sum and a maximum per member.  beam_size < 1, a negative or NaN beam_threshold, and everything
 * asg_beam_decode_words refuses: ASG_ERR_INVALID.  float32 and float64.
 * asg_words_target_scores: out[b] = the lexicon + LM score of targets[b] with consecutive equal labels merged -- start_w, then
 * w(p -> p') of every edge of the walk of step 2, then final_w[q_n] + endw(p_n) -- or -inf where step 2 rejects it (input
 * lengths are not looked at; an empty target is -inf).  The pair twin of asg_graph_target_scores. */
size_t asg_beam_words_full_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size,
                                      int store);
size_t asg_beam_words_full_scratch_bytes(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, int beam_size);
int asg_beam_words_full_forward(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                int beam_size, double beam_threshold, void *work, size_t work_bytes, void *scores, int flags,
                                void *stream);
int asg_beam_words_full_backward(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                 int beam_size, const void *work, size_t work_bytes, const void *scores, const void *grad_scores,
                                 void *grad_inputs, void *grad_transition, void *scratch, size_t scratch_bytes, int flags,
                                 void *stream);
int asg_words_target_scores(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm, void *out,
                            void *stream);

/* ---- asg_beam_words_full_forward with the sets of a LOOK-AHEAD search: the normaliser over what asg_beam_decode_words_la (below)
 * keeps, so a criterion can be trained against the lattice a look-ahead decoder searches at test time.  `la` is that call's
 * look-ahead (asg_word_lookahead, below), built for the same lexicon, LM and folding.  No counterpart in the reference.
 *   1. Kept sets.  A_t, t = 0 .. len-1, are exactly the sets of pairs asg_beam_decode_words_la keeps for the same emissions,
 *      transition, lexicon, LM, look-ahead, beam_size and beam_threshold, bit for bit: the same device code runs -- the dead-end
 *      prune on entry (an edge into a node n with L(h, n) = -inf is no candidate), and the candidates ranked and pruned by their
 *      values WITH L(h, state(q)) included.  The sets are constants of the gradient.
 *   2. Forced pairs.  F_t exactly as in asg_beam_words_full_forward.  The look-ahead does not enter the walk of the target (a
 *      target through a dead-end node is forced in like any other, and its end then rejects it: every F_t empty), and the forced
 *      pairs do not feed back into the search.
 *   3. Lattice.  Step 3 of asg_beam_words_full_forward verbatim over U_t = A_t united with F_t, with the PLAIN weights: no
 *      look-ahead term in alpha, beta, the end or the gradients.  Why: the look-ahead changes a pair's value by L(h, state(q)),
 *      which is 0 at the root and taken back on the separator edge or at the end, so along every complete path the terms
 *      telescope to zero and the sum over the complete paths of a lattice is the same real number with or without them.
 *      Carrying them would only add the rounding of terms that cancel, and would make the forward and backward kernels read the
 *      tables.  The look-ahead decides WHICH pairs are in the lattice and nothing else.
 *   4. With targets a finite scores[b] - (aligned score + asg_words_target_scores) is >= 0 for any beam, as before: the target is
 *      forced in.  Without targets Z_K >= the plain path score (asg_beam_decode_words' sums, no cancelling terms) of the path
 *      asg_beam_decode_words_la returns, since that path runs through the A_t; this is >= that call's `scores` exactly when no
 *      sum rounds (weights and emissions in eighths, say), otherwise up to the rounding of the cancelling terms.  With a beam
 *      that prunes nothing (beam_size >= the pairs of any frame, beam_threshold = +inf) and no dead-end node, U_t is
 *      asg_beam_words_full_forward's: scores and both gradients have that call's bits.  A dead-end node (no word below it that
 *      the LM accepts after h) never lies on a complete path and leads only to other dead ends, so leaving its pairs out removes
 *      members whose beta and end are -inf and changes no other member's alpha: Z_K and both gradients are the same real
 *      numbers as with those pairs in.  Not a promise of the same bits: alpha is (integer reductions), but the members that
 *      remain change place in the floating-point sums of Z_K and of beta, so there the two agree up to that rounding.
 * asg_beam_words_full_backward, asg_beam_words_full_work_bytes and asg_beam_words_full_scratch_bytes serve both forms unchanged:
 * the backward reads the stored U and alpha only, and the look-ahead has no workspace of its own.  Launches, determinism and
 * capture as asg_beam_words_full_forward.  Limits and errors: that call's, then asg_beam_decode_words_la's for `la` (a NULL
 * look-ahead or array, another dtype, a bad A' or levels, S or H other than the LM's: ASG_ERR_INVALID). */
struct asg_word_lookahead;
int asg_beam_words_full_forward_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                   const struct asg_word_lookahead *la, int beam_size, double beam_threshold, void *work,
                                   size_t work_bytes, void *scores, int flags, void *stream);

/* ---- WORD CONFIDENCES and END FRAMES of asg_beam_decode_words' hypothesis, from the lattice its search kept: for every word of
 * the winning path, the frame it ends at and how much of the probability mass inside the kept sets agrees that this word ends
 * there -- what captions, keyword hits and pseudo-labels need beside the words.  No counterpart in the reference.  Per utterance b,
 * len = clamp(input_lengths[b], 0, T); lexicon graph, folded LM, step(h, w), PAIR ORDER, the kept sets A_t and the edges exactly
 * as in asg_beam_decode_words / asg_beam_words_full_forward, WITHOUT targets (p->targets is not looked at): U_t = A_t.
 *   1. Lattice paths.  A path is p_0 .. p_{len-1} with p_t in A_t, p_0 a start pair, consecutive pairs joined by one of the
 *      search's edges (stay, lexicon edge, separator edge with its LM step), and a finite end.  Its weight is what step 3 of
 *      asg_beam_words_full_forward sums: start, edges, transitions, emissions, end.  Z_K = lse over all of them = that call's
 *      score without targets, bit for bit (the same kernels run).  The decoder's winning path is one of these paths.
 *   2. Word events.  A path COMPLETES word w AT FRAME t, 1 <= t <= len-1, when its edge p_{t-1} -> p_t is a separator edge out of
 *      a word-end node with word_of_state = w; it completes w AT FRAME len when it ends in a word-end node of w (the final step
 *      of the end rule).  P(w, t) = sum over the paths with that event of exp(weight - Z_K): histories and source pairs are
 *      summed over, only the word and the frame identify the event.
 *   3. Hypothesis.  The k-th word of the winning path, k < word_lengths[b], is w_k = words[b][k]; its end frame t_k is the frame
 *      of its separator edge (the frame whose label is the separator behind another label), or len for the word of the final
 *      step.  t_k ascends strictly.
 *   4. Outputs.  scores, path, tokens, token_lengths, states, lm_states, words, word_lengths: asg_beam_decode_words' own, bit for
 *      bit (the same device text searches, ends and backtraces).  Beyond them:
 *        word_frames      [B][T] int64: t_k, then -1 behind the words;
 *        word_confidences [B][T] dtype: conf_k = sum over t in [t_k - tol, t_k + tol] meet [1, len] of P(w_k, t), then 0;
 *        normalisers      [B]    dtype: Z_K.
 *      tol = frame_tolerance.  At tol = 0, conf_k is a probability: exp(scores[b] - Z_K) <= conf_k <= 1 up to rounding (the
 *      winning path has the event).  At tol > 0 it is the EXPECTED NUMBER of completions of w_k inside the window: it passes 1
 *      only where a path completes a short word twice inside it, and is returned unclipped.
 *   5. Degenerate utterances.  len == 0, an empty last set or no finite end: score -inf, normaliser -inf, integer outputs -1,
 *      lengths 0, confidences 0.  Never a NaN.
 * An arc posterior is exp((alpha[t-1][p] + c) - Z_K), c = beta[t][p'] + the edge's terms, with alpha of asg_beam_words_full_forward
 * and beta its mirror image (max-then-sum per pair, the sums of asg_beam_words_full_backward); a final-step posterior is
 * exp((alpha[len-1][p] + (final_w[q] + endw(p))) - Z_K).  Each is added to the words it counts for as a 64-bit fixed-point integer
 * with 54 fractional bits: integer adds only, NO FLOAT ATOMICS, bit-identical run to run and for any grouping of the batch.
 * Every output and every workspace word that is read is written by kernels (no memset, no host synchronisation): the call can be
 * captured and replayed.  The frame loop of the search runs ONCE per utterance.
 * K = beam_size, M = K, e = 4 / 8.  Every part rounded up to 256 bytes:
 *   work: asg_beam_words_confidence_work_bytes(p, gb, lm, beam_size) =
 *         B * (asg_beam_words_full_work_bytes' bytes per utterance without targets at store = 1, i.e.
 *              asg_beam_decode_words' bytes per utterance + 2*T*4 + 256 + T*M*8 + T*M*e,     + 2*M*e (two rows of beta))
 * The word accumulators live in LDS and need no workspace.  No term in H, V, A or Q.
 * Limits (ASG_ERR_UNSUPPORTED beyond): those of asg_beam_words_full_forward without targets (beam_size <= 8192, N <= 1024,
 * T <= 2^20, M <= 8179 float32 / 6816 float64), and frame_tolerance <= 64; frame_tolerance < 0: ASG_ERR_INVALID.  Argument
 * errors: those of asg_beam_decode_words (a NULL output among them), then asg_beam_decode_words_la's for `la`.  float32 and
 * float64.
 * asg_beam_words_confidence_la: sets, hypothesis and the eight decoder outputs are asg_beam_decode_words_la's, bit for bit; the
 * lattice keeps the PLAIN weights, exactly as asg_beam_words_full_forward_la does (look-ahead terms cancel along complete
 * paths), so normalisers has that call's bits and scores[b] - Z_K <= 0 holds up to the rounding of the cancelling terms. */
size_t asg_beam_words_confidence_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                            int beam_size);
int asg_beam_words_confidence(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                              int beam_size, double beam_threshold, int frame_tolerance, void *work, size_t work_bytes,
                              void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                              int64_t *lm_states, int64_t *words, int64_t *word_lengths, int64_t *word_frames,
                              void *word_confidences, void *normalisers, int flags, void *stream);
int asg_beam_words_confidence_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                 const struct asg_word_lookahead *la, int beam_size, double beam_threshold, int frame_tolerance,
                                 void *work, size_t work_bytes, void *scores, int64_t *path, int64_t *tokens,
                                 int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                 int64_t *word_lengths, int64_t *word_frames, void *word_confidences, void *normalisers,
                                 int flags, void *stream);

/* ---- WORD CONFIDENCES and END FRAMES for EVERY ROW of asg_beam_decode_words_nbest's list: what rescoring with a stronger LM,
 * confusion-network / ROVER combination of the rows and pseudo-labelling on their agreement need.  The quantity is not new:
 * P(w, t) of asg_beam_words_confidence does not depend on the hypothesis; a row only selects which (word, frame) cells are read.
 * Per utterance b everything is asg_beam_decode_words_nbest's (or _nbest_la's) and asg_beam_words_confidence's (or _la's) on the
 * same arguments: the same search, run ONCE; the same kept sets A_t; the lattice with U_t = A_t and the plain weights; the same
 * Z_K; the same word events P(w, t).  The argument order is asg_beam_decode_words_nbest's with frame_tolerance behind nbest and
 * word_frames, word_confidences, normalisers behind num_hyps; the _la form takes the look-ahead behind the LM.
 *   1. The twelve n-best outputs of asg_beam_decode_words_nbest / _la, bit for bit (the same device text ranks, walks and
 *      writes).  path, states and lm_states may be NULL.
 *   2. word_frames [B][nbest][T] int64.  For row r < num_hyps[b] and k < word_lengths[b][r], t_{r,k} is the frame of the k-th
 *      separator edge of the row's path (step 3 of asg_beam_words_confidence, applied to the row's path), or len for the word
 *      closed by the final step.  It ascends strictly within a row.  -1 behind the words and in padding rows.
 *   3. word_confidences [B][nbest][T] dtype.  conf_{r,k} = sum of P(words[b][r][k], t) over t in [t_{r,k} - tol, t_{r,k} + tol]
 *      meet [1, len]; 0 behind the words and in padding rows; unclipped.  tol = frame_tolerance.
 *   4. normalisers [B] dtype: Z_K.
 * Properties.  Row 0's frames and confidences are asg_beam_words_confidence's on the same arguments, bit for bit: an event is
 * added as the same 54-bit fixed-point integer, and an integer sum does not depend on its order.  At tol = 0,
 * exp(scores[b][r] - Z_K) <= conf_{r,k} <= 1 up to rounding for every row: a row's path is a lattice path that has the event.
 * Rows that hold the same word ending at the same frame get the same bits (they read one cell).  Degenerate utterances (len == 0,
 * an empty last set, no finite end): num_hyps 0, normaliser -inf, frames -1, confidences 0; never a NaN.  NO FLOAT ATOMICS, no
 * memset, no host synchronisation: bit-identical run to run and for any grouping of the batch, and the call can be captured and
 * replayed.  The frame loop of the search runs ONCE per utterance.
 * K = beam_size, M = K, e = 4 / 8, nb = min(nbest, K), P2(x) = the power of two >= max(x, 2).  Every part rounded up to 256 bytes:
 *   work: asg_beam_words_nbest_confidence_work_bytes(p, gb, lm, beam_size, nbest) =
 *         B * (asg_beam_words_confidence_work_bytes' bytes per utterance
 *              + 8 + K*(e+8) (the last set) + T*nb*4 (the rows' product states) + 256 + (T+2)*4 (the first cell of every frame)
 *              + P2(nb*T)*8 (the rows' queries) + nb*T*8 (the cells) + nb*T*8 (their sums))
 *         + 3 * (B*8) + 6*B*T*8 (the one-best outputs of the search).
 * No term in H, V, A or Q.
 * Limits: the union of the two parent calls': nbest < 1 or frame_tolerance < 0: ASG_ERR_INVALID; nbest > 8192 or
 * frame_tolerance > 64: ASG_ERR_UNSUPPORTED; the limits of asg_beam_words_confidence.  ONE new limit (ASG_ERR_UNSUPPORTED
 * beyond): the accumulators of the open cells live in LDS beside a frame's lattice set,
 *         16 * ceil(M*(e+8) / 16) + 1024 + 12 * P2(min(nbest, K) * (2*frame_tolerance + 2)) <= 163840   and   nb*T <= 2^30.
 * Argument errors, in this order: asg_beam_words_confidence's for p, gb, lm and beam_size; nbest; frame_tolerance and the new
 * limit; `la` as asg_beam_decode_words_la checks it; the threshold; a NULL among work and the outputs other than path, states,
 * lm_states; the workspace.  float32 and float64. */
size_t asg_beam_words_nbest_confidence_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                                  int beam_size, int nbest);
int asg_beam_words_nbest_confidence(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                    int beam_size, double beam_threshold, int nbest, int frame_tolerance, void *work,
                                    size_t work_bytes, void *scores, void *emission_scores, void *graph_scores, void *lm_scores,
                                    int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states,
                                    int64_t *words, int64_t *word_lengths, int64_t *num_hyps, int64_t *word_frames,
                                    void *word_confidences, void *normalisers, int flags, void *stream);
int asg_beam_words_nbest_confidence_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                       const struct asg_word_lookahead *la, int beam_size, double beam_threshold, int nbest,
                                       int frame_tolerance, void *work, size_t work_bytes, void *scores, void *emission_scores,
                                       void *graph_scores, void *lm_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                                       int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths,
                                       int64_t *num_hyps, int64_t *word_frames, void *word_confidences, void *normalisers,
                                       int flags, void *stream);

/* ---- asg_beam_decode_words with LM LOOK-AHEAD: inside a word, a pair's value also carries the best LM score that any word below
 * its trie node can still get after the pair's history, so that a narrow beam ranks partial words by more than acoustics.  The
 * term telescopes: every edge adds the difference between the look-ahead of its two ends, the separator edge takes back what the
 * word entered with, and a complete hypothesis sums the terms of asg_beam_decode_words plus terms that cancel.  One value per
 * pair stays the only search state; table, select, prune, pair order, back-pointers, the eight outputs and the workspace
 * (asg_beam_decode_words_work_bytes serves both calls) are asg_beam_decode_words'.  No counterpart in the reference.
 * The arrays (torch_asg_amd.WordLookahead builds them):
 *   ranks:  the trie (automaton states of the lexicon, root 0, the separator arcs left out) in pre-order, children by ascending
 *           token; the word of a word-end node takes the next rank when the node is entered.  rlo[n] / rhi[n] are the counter on
 *           entry and on exit, so the words below n, its own included, have the ranks [rlo[n], rhi[n]).  LM words the lexicon does
 *           not spell have no rank; a lexicon word without an LM arc has a rank and no arcs.
 *   rows:   for every LM state s its arcs whose word has a rank, sorted by rank: krow [H+1] offsets, krank [A'] ascending within
 *           a row.  E(s, n) = the largest lw over the arcs of row s with rank in [rlo[n], rhi[n]), -inf if there is none.
 *           tab [levels][A']: tab[k][i] = the largest lw over the arcs i .. i + 2^k - 1 that lie in the row of i (tab[0] is lw in
 *           rank order), 2^(levels-1) <= the longest row; E is two binary searches in krank and two reads.  -0 is stored as +0,
 *           so a maximum is one bit pattern and the values, not the layout, are what is specified.  dense0 [S] holds E(0, n)
 *           for every node: state 0, the empty history, ends the backoff chains and has the longest row, so its answer is
 *           one read (the same value, another layout).
 *   la_state [H]: the history whose rows the look-ahead of h reads: h backed off until at most order - 1 backoff steps remain
 *           to a state without a backoff (order 1: one state for all h, unigram smearing; order >= the LM's: h itself).
 *   The caller guarantees: every ranked word with an arc in any row has an arc in every state without a backoff (an ARPA LM: all
 *   unigrams in state 0).  Then LA = -inf says that no word below the node is accepted, whatever the truncation.
 * All sums in the dtype of the problem, in the order written ("max(r, x)" is x if x > r, else r):
 *   LA(s, n):  r = -inf; a = 0
 *              loop: r = max(r, a + E(s, n));  if backoff[s] < 0: return r;  a = a + bw[s];  s = backoff[s]
 *   L(h, n) = 0 if n is the root, else LA(la_state[h], n)
 *   t = 0:  for a start state q, c = (start_w[q] + L(start, state(q))) + I[0][i(q)].
 *   stay:   unchanged: the same node, nothing added.
 *   edge from a kept (h, q') to q with label i != separator: L(h, state(q)) == -inf is no candidate (a dead end is pruned here);
 *           else c = ((v + tr[i][j]) + ow[e]) + (L(h, state(q)) - L(h, state(q'))).
 *   separator edge out of a word-end node, (h', a) = step(h, w): c = ((v + tr[i][j]) + ow[e]) + (a - L(h, state(q'))); the
 *           target is the root, whose L is 0.
 *   end:    at the root (v + final_w[q]) + ew[h]; in a word-end node (v + final_w[q]) + ((a - L(h, state(q))) + ew[h']); mid-word
 *           none.
 * L(h, state(q')) of a kept pair is finite by construction (it entered its node through a finite L, start pairs included), so no
 * -inf - -inf is formed.  Every other rule is asg_beam_decode_words', verbatim.
 * Consequences: with beam_size >= all pairs and an infinite threshold the kept paths are those of asg_beam_decode_words, and
 * `scores` differs from that call's only by the rounding of the cancelling terms (bit-equal when no sum rounds).  With a beam
 * that prunes, the two searches keep different sets: that is the point.
 * Cost: per expanded edge and backoff level of la_state[h] two binary searches in a row of krank and two reads; L of the source
 * pair once per pair and candidate phase; at state 0 one read.  No workspace of its own, no atomics, nothing to clear;
 * (A' * levels + S) * e bytes of table.
 * Limits and errors: those of asg_beam_decode_words; a NULL look-ahead, one of another dtype, a NULL or mis-sized array (A' < 0,
 * A' > A, levels outside 1 .. 31 or beyond what A' arcs can fill) or one built for another lexicon / LM shape (S, H):
 * ASG_ERR_INVALID.  Nothing of it is validated on the device.
 * The two word streams take the look-ahead through asg_beam_word_stream_*_la and asg_beam_word_window_*_la (below, with the rule
 * for the prefix result), the two n-best calls through asg_beam_decode_words_nbest_la and asg_beam_word_stream_nbest_la (further
 * below, with the rule for the score split: the three parts take no look-ahead term). */
typedef struct asg_word_lookahead {
    int64_t S;                     /* automaton states of the lexicon (entries of rlo, rhi) = asg_word_lm.S */
    int64_t H;                     /* history states (entries of la_state) = asg_word_lm.H                  */
    int64_t A;                     /* ranked arcs A'                                                        */
    int32_t levels;                /* levels of tab                                                         */
    int32_t dtype;                 /* ASG_DTYPE_F32 / ASG_DTYPE_F64 of tab (= the problem's)               */
    const int32_t *rlo;            /* [S]                                                                   */
    const int32_t *rhi;            /* [S]                                                                   */
    const int32_t *la_state;       /* [H]                                                                   */
    const int32_t *krow;           /* [H+1]                                                                 */
    const int32_t *krank;          /* [A']                                                                  */
    const void *tab;               /* [levels][A']                                                          */
    const void *dense0;            /* [S] E(0, n) of every node n                                           */
} asg_word_lookahead;
int asg_beam_decode_words_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                             const asg_word_lookahead *la, int beam_size, double beam_threshold, void *work, size_t work_bytes,
                             void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                             int64_t *lm_states, int64_t *words, int64_t *word_lengths, int flags, void *stream);

/* ---- STREAMING beam decoding with a lexicon and a word n-gram LM: the search of asg_beam_decode_words over pairs (h, q) carried
 * across chunks of frames, as asg_beam_stream_* carries the search of asg_beam_decode_graph -- the growing stream, bounded by
 * max_frames.  A live transcription service gets a word LM and a transcript while the utterance is still arriving.  No counterpart
 * in the reference.  gb and lm are those of asg_beam_decode_words (the weights folded by the caller).
 * A WORD STREAM STATE is one device buffer that serves B utterance slots, for a fixed lexicon, LM shape, dtype, K = beam_size (no
 * clamp to Q) and max_frames (every call on a state passes the same gb, lm, B, beam_size and max_frames).  Per slot it holds:
 * pos, the frames consumed so far; the kept set A_{pos-1} of pairs with its values; the back-pointers (product state, LM state,
 * source slot) of the frames 0 .. pos-1; a sticky overflow word; and the table and lists of the search.  The contents are opaque;
 * a state must be reset before its first use.
 *   asg_beam_word_stream_reset: for every slot b with mask[b] != 0 (one byte per slot on the device; NULL: every slot): pos = 0,
 *     the set empty, overflow = 0, and all C slots of the table emptied (the only place where all of them are written: a frame
 *     empties what it touched).  Written by a kernel.
 *   asg_beam_word_stream_advance: p->inputs is a chunk [Tc = p->T, B, N] (any strides) and p->input_lengths the chunk's lengths
 *     (NULL: Tc for every slot); p->transition and beam_threshold are used for the frames of this call (they may differ between
 *     calls).  For slot b: n = min(clamp(input_lengths[b], 0, Tc), max_frames - pos).  If the bound by max_frames cut anything,
 *     overflow = 1; the frames beyond it are not consumed and nothing is written out of bounds.  The chunk's frames 0 .. n-1 are
 *     the frames pos .. pos+n-1 of the utterance and run exactly the rules of asg_beam_decode_words -- the same adds in the same
 *     order, the same LM walk, the same pair order in every tie, the same prune; the same device code: frame 0 of the utterance
 *     takes the pairs (start, q) of start_q, every other frame -- the first frame of a chunk included, LM walk and all -- its
 *     candidates from the stored set; an empty set stays empty.  Then pos += n (also for an empty set).  Nothing is written
 *     besides the state.  Tc = 0 is allowed and changes nothing.
 *   asg_beam_word_stream_result: reads the state and does not modify it; it may be called after any chunk, and the stream
 *     continues.  With L = pos and A = A_{L-1} with values v:
 *       final != 0: the end of asg_beam_decode_words: end(h, q) = (v + final_w[q]) + endw, endw = ew[h] at the root, a + ew[h'] after
 *                   one more LM step in a word-end node (rejected: no end), no end mid-word; the word of that step is appended to
 *                   words.
 *       final == 0: end(h, q) = v, the best PREFIX hypothesis: no final weight, no LM end, no final word.  A prefix that ends
 *                   mid-word is a valid prefix; words holds the words of the separator edges on the path only.
 *     The winner is the pair of A with the largest end > -inf, the smallest pair on a tie (-0 and +0 are equal).  scores [B]
 *     (dtype) = its end; path, tokens, states, lm_states, words [B][max_frames] int64 follow its back-pointers as in
 *     asg_beam_decode_words, -1 behind the data; token_lengths, word_lengths [B]; frames [B] = L; status [B] = the overflow word
 *     (0 / 1).  L == 0, an empty set or no finite end: score -inf, every integer array -1, both lengths 0.
 * REQUIRED PROPERTY.  Take a slot that was reset and then advanced by any sequence of chunks that concatenate to x[0:L],
 * L <= max_frames (chunks of no frames included).  asg_beam_word_stream_result(final = 1) then equals asg_beam_decode_words on x
 * with T >= L frames, input_length = L, the same transition, beam_size, beam_threshold, folding and dtype: scores, token_lengths
 * and word_lengths bit for bit; path, tokens, states, lm_states and words equal on the columns < T and -1 elsewhere.  No
 * tolerance: the search over pairs never looks ahead, and the LM walk depends on the source pair alone.
 * State (asg_beam_word_stream_state_bytes; 0 for arguments that the calls refuse), every part rounded up to 256 bytes:
 *   B * (asg_beam_decode_words' bytes per utterance with T = max_frames + 256 (pos, set size, overflow) + K*(e + 8) (the stored
 *   set: values, then product states, then LM states)), e = 4 / 8.  The back-pointers keep asg_beam_decode_words' [frame][K]
 *   layout -- the source slots of all kept pairs, not only the winner's: asg_beam_word_stream_nbest walks them.  No term in H, V, A
 *   or Q.
 * Each call is ONE launch on `stream`, one 1024-thread workgroup per slot for advance and result: no host synchronisation, no
 * copy, no memset, so a captured call replays with new chunk contents and lengths, and a capture is one linear chain.  Integer
 * atomics only: bit-identical run to run.  Limits and errors: those of asg_beam_decode_words with T = max_frames (beam_size <=
 * 8192, H, Q <= 2^25, A < 2^31; ASG_ERR_UNSUPPORTED beyond) and those of asg_beam_stream_*: max_frames < 1, Tc < 0, B < 1,
 * beam_size < 1, a negative or NaN beam_threshold, a dtype that is not the graph's and the LM's, a NULL array or output:
 * ASG_ERR_INVALID; a state buffer smaller than asg_beam_word_stream_state_bytes: ASG_ERR_WORKSPACE.  Not here: a loss over a
 * stream (the one-shot loss over pairs: asg_beam_words_full_forward above; n-best over pairs: asg_beam_word_stream_nbest
 * below; the windowed form with a committed prefix: asg_beam_word_window_* further below; LM look-ahead:
 * asg_beam_word_stream_advance_la behind those).  `flags` is reserved (pass 0). */
size_t asg_beam_word_stream_state_bytes(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype, int beam_size,
                                        int64_t max_frames);
int asg_beam_word_stream_reset(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                               int64_t max_frames, void *state, size_t state_bytes, const uint8_t *mask, int flags, void *stream);
int asg_beam_word_stream_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                 int beam_size, double beam_threshold, int64_t max_frames, void *state, size_t state_bytes,
                                 int flags, void *stream);
int asg_beam_word_stream_result(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                                int64_t max_frames, const void *state, size_t state_bytes, int final, void *scores, int64_t *path,
                                int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                int64_t *word_lengths, int64_t *frames, int64_t *status, int flags, void *stream);

/* ---- The N BEST hypotheses of the search over pairs, each with its score split THREE ways -- acoustic, lexicon, LM -- and its
 * words: what an n-best rescoring pass with a stronger LM and the tuning of lm_weight / word_score need.  No counterpart in the
 * reference.  The search of asg_beam_decode_words runs unchanged: the same sets, the same back-pointers, the same bits (the same
 * device code).  For utterance b with len = clamp(input_lengths[b], 0, T), A = A_{len-1} with values v:
 *   candidates: every pair (h, q) of A whose end(h, q) = (v + final_w[q]) + endw is > -inf, endw exactly as in
 *     asg_beam_decode_words: ew[h] when state(q) is the root; in a word-end node one more step(h, w), endw = a + ew[h'], no
 *     candidate if the LM rejects; mid-word there is none.  Ordered by end descending (-0 and +0 are equal), then PAIR ORDER
 *     (h ascending, then q ascending).  num_hyps[b] = min(nbest, number of candidates).
 *   For r < num_hyps[b], with (h_t, q_t), t < len, the back-pointer path of the r-th candidate, i_t and s_t label and automaton
 *   state of q_t:
 *     scores[b][r] = the search's own end sum of that pair.  path[b][r][t] = i_t, states[b][r][t] = s_t, lm_states[b][r][t] =
 *     h_t: optional, each may be NULL and is then not written.  tokens / token_lengths: the collapse of the path.  words /
 *     word_lengths: the word of every separator edge on the path, in order, then the word of the final step if the path ends in
 *     a word-end node (asg_beam_decode_words' rule).
 *     Three sums over the path, in frame order, adds only, in the dtype of the problem:
 *       emission_scores: a = I[0][i_0]; for t >= 1: a = (a + tr[i_t][i_{t-1}]) + I[t][i_t].
 *       graph_scores (the lexicon automaton): g = start_w[q_0]; for every t >= 1 with q_t != q_{t-1}: g = g + ow[e] of the edge
 *         q_{t-1} -> q_t; last g = g + final_w[q_{len-1}].
 *       lm_scores: l = 0; for every separator edge (q_t != q_{t-1}, i_t == separator), in order: l = l + a, a the sum of
 *         step(h_{t-1}, word) as step itself forms it (0, + bw per backoff step, + lw of the arc); last l = l + endw.
 *   scores is the search's sum and NOT the rounded sum of the three parts: they agree within 2 * n * eps * (the sum of the
 *   magnitudes of the terms), n the number of terms the three sums add, the inner terms of every LM walk included (two
 *   summation orders of the same n terms).  With word_lengths the caller can re-weight: lm_scores = lm_weight * (raw LM) +
 *   word_score * word_lengths up to rounding.
 *   Rows r >= num_hyps[b] are padding: the four scores -inf, every integer output -1, both lengths 0.  Frames t >= len: -1.
 *   Row 0 equals asg_beam_decode_words' eight outputs bit for bit.
 *   DISTINCTNESS.  Lexicon and LM are deterministic, so a token sequence determines its pair: the rows are distinct token
 *   sequences.  (Not every token sequence has a row: those whose histories the LM no longer tells apart -- after a backoff, or
 *   beyond the order of the n-gram -- end in one pair, and the search keeps the best of them, as it does for the one best.)
 *   Word sequences can repeat: the same words with and without a closing separator end at the root and in the
 *   word-end node.  Rows are not merged; the better of the two comes first, and a caller who wants distinct word sequences drops
 *   the later one.
 *   scores, emission_scores, graph_scores, lm_scores [B][nbest] (dtype); path, tokens, states, lm_states, words [B][nbest][T]
 *   int64; token_lengths, word_lengths [B][nbest] int64; num_hyps [B] int64.
 * `work` (asg_beam_decode_words_nbest_work_bytes), every part rounded up to 256 bytes, nb = min(nbest, beam_size), e = 4 / 8:
 *   B * (asg_beam_decode_words' bytes per utterance + (8 + K*(e + 8)) (size, values, product states and LM states of the last
 *   set) + T*nb*4 (the product states of every hypothesis)) + 3*B*8 + 5*B*T*8 (what the one-best search itself returns).  No term
 *   in H, V, A or Q.
 * Two launches on one stream, one workgroup per utterance each; no memset, no copy, no synchronisation: a captured call replays
 * with new emissions and lengths.  No float atomics: bit-identical run to run.  nbest < 1: ASG_ERR_INVALID; nbest > 8192:
 * ASG_ERR_UNSUPPORTED (nbest > beam_size only adds padding rows); everything else as for asg_beam_decode_words.
 *
 * asg_beam_word_stream_nbest: the same over a word stream state, which it only reads (the same kernel, pointed at the stored set
 * and at rows 0 .. pos-1).  final != 0: the rules above with len = pos.  final == 0: the n best PREFIXES: the candidates are the
 * kept pairs with v > -inf, mid-word pairs included, ordered by v descending, then pair order; scores = v; graph_scores has no
 * final_w, lm_scores no endw, and there is no final word.  Row 0 equals asg_beam_word_stream_result(final) bit for bit; frames and
 * status are that call's.  A stream state keeps no emissions, so there is NO emission_scores here: a caller who kept the frames
 * takes it from asg_beam_decode_words_nbest, the others have scores - (graph_scores + lm_scores) up to rounding.  For any chunking
 * of an utterance of at most max_frames frames, the outputs with final != 0 equal asg_beam_decode_words_nbest's bit for bit (on
 * that call's columns, -1 beyond): the n-best stage reads the set and the rows only, and those are the one-shot search's
 * (REQUIRED PROPERTY above).  `work` (asg_beam_word_stream_nbest_work_bytes): B * max_frames*nb*4 rounded up to 256 bytes per
 * slot; its contents mean nothing between calls.  One launch.  Errors: those of asg_beam_word_stream_result, the nbest limits
 * above, a short `work`: ASG_ERR_WORKSPACE.  `flags` is reserved (pass 0). */
size_t asg_beam_decode_words_nbest_work_bytes(const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                              int beam_size, int nbest);
int asg_beam_decode_words_nbest(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                int beam_size, double beam_threshold, int nbest, void *work, size_t work_bytes, void *scores,
                                void *emission_scores, void *graph_scores, void *lm_scores, int64_t *path, int64_t *tokens,
                                int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths,
                                int64_t *num_hyps, int flags, void *stream);
size_t asg_beam_word_stream_nbest_work_bytes(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype,
                                             int beam_size, int64_t max_frames, int nbest);
int asg_beam_word_stream_nbest(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                               int64_t max_frames, const void *state, size_t state_bytes, int final, int nbest, void *work,
                               size_t work_bytes, void *scores, void *graph_scores, void *lm_scores, int64_t *path, int64_t *tokens,
                               int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths,
                               int64_t *num_hyps, int64_t *frames, int64_t *status, int flags, void *stream);

/* ---- WINDOWED streaming beam decoding with a lexicon and a word n-gram LM: asg_beam_word_stream_* in BOUNDED memory, as
 * asg_beam_window_* is asg_beam_stream_* in bounded memory -- an open microphone, a meeting, a broadcast, with a word LM and a
 * transcript in WORDS.  The search is asg_beam_word_stream_advance's (the same device code, the same sets and scores bit for bit);
 * the back-pointers are kept only for a window of W frames, in rings, and the prefix of the transcript on which all surviving
 * hypotheses agree is COMMITTED: returned by the advance that finds it, never to change.  No counterpart in the reference.
 * A WORD WINDOW STREAM STATE serves B slots, for a fixed lexicon, LM shape, dtype, K = beam_size (no clamp to Q), window W >= 1 and
 * commit period P, 1 <= P <= W (every call on a state passes the same gb, lm, B, beam_size, W and P).  Per slot it holds: pos
 * (int64), the frames consumed so far -- unbounded; base (int64), the frames committed so far, base <= pos; the stored set
 * A_{pos-1} of pairs: values, then product states q, then LM states h, exactly asg_beam_word_stream_*'s; three rings bq / bh / bs
 * int32 [W][K], the back-pointers (product state, LM state, source slot) of frame u in row u mod W (computed in 64 bits); carry
 * (int32), the label of the last committed frame or -1; carry_state (int32), the automaton state of the last committed frame or
 * -1; a sticky status word; and the table and lists of the search.  The contents are opaque; a state must be reset before its
 * first use.
 *   asg_beam_word_window_reset: as asg_beam_word_stream_reset (all C slots of the table emptied), and pos = base = 0, carry =
 *     carry_state = -1, status = 0 for the chosen slots.
 *   asg_beam_word_window_advance: p->inputs is a chunk [Tc = p->T, B, N], p->input_lengths the chunk's lengths, p->transition and
 *     beam_threshold those of this call.  For slot b, n = clamp(input_lengths[b], 0, Tc) -- there is no max_frames and no overflow
 *     word.  The chunk's frames are the frames pos .. pos+n-1 of the utterance and run exactly as in asg_beam_word_stream_advance
 *     (frame 0 -- and only pos == 0 -- from start_q, the first frame of a chunk from the stored set, an empty set stays empty); the
 *     back-pointers of frame u go to row u mod W.  After each frame, with pos now counting it, a COMMIT ATTEMPT runs if
 *     pos mod P == 0 and the set is not empty.  It is asg_beam_window_advance's, over the slots of pairs:
 *       1. Convergence.  R = all slots of A_{pos-1}.  If |R| == 1: c = pos-1.  Otherwise for u = pos-1 down to base+1:
 *          R <- { bs[u][k] : k in R }; the first u at which |R| == 1 gives c = u-1; no such u: no c.  If c exists, the path from
 *          that one slot of frame c back to frame base is committed: the frames base .. c in ascending order, and base = c+1.
 *          (Slots, not product states: two pairs with one q and two histories are two slots.)
 *       2. Forced commit, if afterwards pos - base > W - P: F = (pos - base) - (W - P).  The best prefix pair of A_{pos-1} --
 *          largest v, smallest pair on a tie, -0 equal to +0: the rule of asg_beam_word_stream_result(final = 0) -- is followed
 *          back to frame base+F-1; the frames base .. base+F-1 on that path are committed, base += F and status |= 1.
 *     Committing a frame with pair (h, q) appends label[q] to new_path, state[q] to new_states and h to new_lm_states at the next
 *     free column of this call's output row.  To new_tokens it appends label[q] if label[q] != carry.  To new_words it appends
 *     word_of_state[carry_state] if label[q] == separator, carry != separator and carry != -1 (the frame is not frame 0): the
 *     separator behind another label is a separator edge, and its word ends in the state before -- asg_beam_decode_words' rule
 *     for words, continued across segments: the label and the state before the first frame of a segment are those of the last
 *     frame committed before it, in this call or an earlier one, so an edge that straddles two commits or two calls yields its
 *     word exactly once.  (A forced commit may splice two paths; the state before a separator is then whatever was committed, and
 *     its word may be -1.)  Then carry = label[q], carry_state = state[q].  After an attempt pos - base <= W - P, between attempts
 *     pos - base <= W: no live row is ever overwritten.  Then pos += n.
 *     Outputs: new_path, new_states, new_lm_states, new_tokens, new_words int64 [B][W + Tc] (committed <= (pos - base before the
 *     call) + n <= W + Tc), -1 behind the data; new_frames [B], the frames this call committed; new_token_lengths,
 *     new_word_lengths [B].  Every element of all eight is written by the kernel.  Tc = 0 is allowed and writes the empty outputs.
 *   asg_beam_word_window_result: reads the state only; the stream goes on.  The winner is chosen as in
 *     asg_beam_word_stream_result: final != 0: end(h, q) = (v + final_w[q]) + endw, the end of asg_beam_decode_words; final == 0:
 *     v, the best prefix; the smallest pair on a tie.  scores [B]; path, states, lm_states, tokens, words int64 [B][W], -1 behind
 *     the data: path, states and lm_states hold the winner's frames base .. pos-1 (the uncommitted TAIL, at most W); tokens their
 *     collapse started from carry; words the words of the tail by the rule above, started from carry / carry_state, then, with
 *     final != 0, the word of the final step if the winner ends in a word-end node (also when the tail is empty).  token_lengths,
 *     word_lengths [B]; frames [B] = pos; committed [B] = base; status [B]: bit 0 = a forced commit has happened (sticky until the
 *     reset), bit 1 = pos >= 1 and the set is empty.  No frame, an empty set or no finite end: score -inf, the integer arrays -1,
 *     both lengths 0; what was committed stays committed.  The backtrace is at most W steps, whatever pos.
 * REQUIRED PROPERTIES (no tolerance in any).  1. Search identity: for any chunking of x[0:L], any W and P, result(final = 1).scores
 * equals asg_beam_decode_words' score on x bit for bit and result(final = 0).scores equals asg_beam_word_stream_result's: the
 * rings cannot alter a score, the frame reads its sources from the set.  2. Chunk invariance: at equal pos, base, carry,
 * carry_state, status and the concatenation of everything advance has returned are the same for every chunking, forced commits
 * included -- attempts happen at frame indices, not at call boundaries.  3. Exactness: while status bit 0 is clear and the
 * one-shot score is finite, concat(new_path of all calls) followed by the tail path equals the one-shot path[:L], the same for
 * states and lm_states, concat(new_tokens) followed by the tail tokens equals the one-shot tokens[:token_length], and
 * concat(new_words) followed by the tail words (final = 1) equals the one-shot words[:word_length]; with W - P >= L a forced commit
 * is impossible.  4. With status bit 0 set the outputs are still exactly those specified above.
 * State (asg_beam_word_window_state_bytes; 0 for arguments that the calls refuse), every part rounded up to 256 bytes:
 *   B * (asg_beam_decode_words' bytes per utterance with T = W, 3 * W*K*4 + C*(16 + e) + cap*(e + 12), + 256 (pos, base, set size,
 *   carry, carry_state, status) + K*(e + 8) (the stored set)), e = 4 / 8.  No term in H, V, A, Q or pos.
 * Each call is ONE launch on `stream`, one 1024-thread workgroup per slot for advance and result: no host synchronisation, no
 * copy, no memset, so a captured advance or result is one kernel node of a linear chain and replays with new chunk contents and
 * lengths.  Integer atomics only: bit-identical run to run.  Limits and errors: those of asg_beam_decode_words with T = W
 * (beam_size <= 8192 with no clamp to Q, H, Q <= 2^25, A < 2^31, W within asg_beam_window_*'s bound; ASG_ERR_UNSUPPORTED beyond);
 * W < 1, P < 1, P > W, Tc < 0, B < 1, beam_size < 1, a negative or NaN beam_threshold, a dtype that is not the graph's and the
 * LM's, a NULL array or output: ASG_ERR_INVALID; a state buffer smaller than asg_beam_word_window_state_bytes: ASG_ERR_WORKSPACE.
 * The n best of the window: asg_beam_word_window_nbest below.  Not here: a commit rule that looks at scores (LM look-ahead:
 * asg_beam_word_window_advance_la below).
 * `flags` is reserved (pass 0). */
size_t asg_beam_word_window_state_bytes(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype, int beam_size,
                                        int64_t W, int64_t P);
int asg_beam_word_window_reset(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                               int64_t W, int64_t P, void *state, size_t state_bytes, const uint8_t *mask, int flags, void *stream);
int asg_beam_word_window_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                 int beam_size, double beam_threshold, int64_t W, int64_t P, void *state, size_t state_bytes,
                                 int64_t *new_path, int64_t *new_states, int64_t *new_lm_states, int64_t *new_tokens,
                                 int64_t *new_words, int64_t *new_frames, int64_t *new_token_lengths, int64_t *new_word_lengths,
                                 int flags, void *stream);
int asg_beam_word_window_result(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                                int64_t W, int64_t P, const void *state, size_t state_bytes, int final, void *scores, int64_t *path,
                                int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                int64_t *word_lengths, int64_t *frames, int64_t *committed, int64_t *status, int flags,
                                void *stream);

/* ---- The two word streams with LM LOOK-AHEAD: asg_beam_word_stream_* and asg_beam_word_window_* over the search of
 * asg_beam_decode_words_la.  Each entry point is the plain call with `la`, the look-ahead of that call, behind `lm`; everything
 * the plain call's text says holds with the changes below.  No counterpart in the reference.
 *   Frames.  Every frame a stream consumes runs the rules of asg_beam_decode_words_la, verbatim: t = 0 (frame 0 of the utterance,
 *     and only pos == 0), stay, the edge into a node with its dead-end prune, the separator edge.  The stored set holds the values
 *     as the search ranks them, L(h, state(q)) included.  L reads static arrays and the pair's own (h, q) -- nothing of the frame,
 *     the chunk or the call -- so a pair kept a call ago expands as one kept a frame ago, separator edge on the first frame of a
 *     chunk included.
 *   result, final != 0: the end of asg_beam_decode_words_la: (v + final_w[q]) + ew[h] at the root, (v + final_w[q]) +
 *     ((a - L(h, state(q))) + ew[h']) in a word-end node, none mid-word.
 *   result, final == 0, the best PREFIX: end(h, q) = v - L(h, state(q)) -- the estimate that has not cancelled yet is taken
 *     back.  L is 0 at the root and finite for every kept pair, so the end of a kept pair is finite.  The winner is the largest
 *     end, the smallest pair on a tie, -0 equal to +0; scores = that end; path, words and tokens follow the plain call's prefix
 *     rules.  A prefix score thus means what it means without look-ahead: a beam that prunes nothing returns the prefix of the
 *     plain stream (bit for bit when no sum rounds), and where the two differ pruning is the cause, not the reporting.
 *   Window.  asg_beam_word_window_advance word for word over the frame above.  Convergence looks at slots only and does not change;
 *     the forced commit follows "the best prefix pair", which is the rule above (largest v - L); result as above for both values
 *     of `final`.
 * REQUIRED PROPERTIES (no tolerance).  asg_beam_word_stream_result_la(final = 1) after any chunking of x[0:L] equals
 * asg_beam_decode_words_la on x as the plain stream equals asg_beam_decode_words; the properties 1 - 4 of asg_beam_word_window_*
 * hold with asg_beam_decode_words_la and asg_beam_word_stream_result_la in the place of the plain calls.
 * Mixing.  A state advanced with a look-ahead must be read, and advanced further, with the same look-ahead, and a state advanced
 * without one by the plain calls: the stored values do not say which estimate they carry, and NOTHING HERE CAN CHECK IT -- the
 * caller guarantees it (torch_asg_amd's stream objects bind the look-ahead in their constructor).
 * State.  asg_beam_word_{stream,window}_state_bytes and _reset serve both forms: the look-ahead adds no byte to a state and
 * nothing to clear.  One launch per call as the plain calls, no workspace, integer atomics only, capturable.
 * Limits and errors: the plain call's, and asg_beam_decode_words_la's for `la`: a NULL look-ahead, one of another dtype, a NULL
 * or mis-sized array, or S / H other than the LM view's: ASG_ERR_INVALID.  The n best of such a stream:
 * asg_beam_word_stream_nbest_la below. */
int asg_beam_word_stream_advance_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                    const asg_word_lookahead *la, int beam_size, double beam_threshold, int64_t max_frames,
                                    void *state, size_t state_bytes, int flags, void *stream);
int asg_beam_word_stream_result_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                   const asg_word_lookahead *la, int64_t B, int beam_size, int64_t max_frames, const void *state,
                                   size_t state_bytes, int final, void *scores, int64_t *path, int64_t *tokens,
                                   int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                   int64_t *word_lengths, int64_t *frames, int64_t *status, int flags, void *stream);
int asg_beam_word_window_advance_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                    const asg_word_lookahead *la, int beam_size, double beam_threshold, int64_t W, int64_t P,
                                    void *state, size_t state_bytes, int64_t *new_path, int64_t *new_states,
                                    int64_t *new_lm_states, int64_t *new_tokens, int64_t *new_words, int64_t *new_frames,
                                    int64_t *new_token_lengths, int64_t *new_word_lengths, int flags, void *stream);
int asg_beam_word_window_result_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                   const asg_word_lookahead *la, int64_t B, int beam_size, int64_t W, int64_t P, const void *state,
                                   size_t state_bytes, int final, void *scores, int64_t *path, int64_t *tokens,
                                   int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                   int64_t *word_lengths, int64_t *frames, int64_t *committed, int64_t *status, int flags,
                                   void *stream);

/* ---- The N BEST hypotheses of the WINDOWED word stream: asg_beam_word_stream_nbest's list from a state of asg_beam_word_window_*,
 * which the call only reads -- the same kernel, pointed at the stored set and at the rings -- so that an open microphone with a
 * lexicon and a word LM can hand a list to a rescorer in bounded memory.  The arguments are asg_beam_word_window_result's
 * (asg_beam_word_window_result_la's), then nbest, work, work_bytes, then the outputs.  Throughout K = beam_size (no clamp to Q)
 * and nb = min(nbest, K).  No counterpart in the reference.
 * asg_beam_word_window_nbest.  The candidates, their order, num_hyps and scores are asg_beam_word_stream_nbest's at equal pos, bit
 *   for bit (the window's property 1, for every row): every entry (h, q) of the stored set with a valid q whose end is > -inf --
 *   final != 0: end = (v + final_w[q]) + endw, the end of asg_beam_decode_words (none mid-word, none where the LM rejects the
 *   word); final == 0: end = v, the n best PREFIXES --, end descending, then pair order ascending, -0 equal to +0.  num_hyps [B] =
 *   min(nbest, candidates): 0 for pos == 0 or an empty set.  scores [B][nbest] (dtype) = the candidate's end.
 *   Row r < num_hyps holds the candidate's TAIL, the frames base .. pos-1 on ITS OWN chain of back-pointers through the rings
 *   (frame u in row u mod W), column t = frame base + t, walked in at most W steps; all row outputs are int64 [B][nbest][W], -1
 *   behind the data.  path = label[q], states = state[q], lm_states = the ring bh of every tail frame (any of the three may be
 *   NULL: not written).  tokens is the collapse of the tail started from carry -- a first tail label equal to carry is no token.
 *   words follows asg_beam_word_window_advance's rule started from carry / carry_state: a tail frame whose label is the separator
 *   behind a label that is neither the separator nor -1 appends word_of_state[the automaton state of the frame before], and before
 *   column 0 that label and state are carry and carry_state -- a separator edge on the first uncommitted frame yields its word
 *   exactly once, here and not in any commit.  With final != 0 the word of the final step is appended if the candidate ends in a
 *   word-end node, also behind an empty tail, while fewer than W words stand in the row (asg_beam_word_window_result's bound).
 *   token_lengths, word_lengths [B][nbest].  The tail may be empty (base == pos, after a commit up to the last frame): the row
 *   still counts, with its score, its final word if it has one, and -1 elsewhere.  Rows >= num_hyps: scores -inf, every wide
 *   column -1, both lengths 0.  frames [B] = pos, committed [B] = base and status [B] (bit 0: a forced commit has happened,
 *   bit 1: pos >= 1 and the set is empty) as asg_beam_word_window_result writes them.
 * asg_beam_word_window_nbest_la, over a state that asg_beam_word_window_advance_la left: the same with the ends of
 *   asg_beam_word_stream_nbest_la -- final != 0: (v + final_w[q]) + ew[h] at the root, (v + final_w[q]) + ((a - L(h, state(q))) +
 *   ew[h']) in a word-end node; final == 0: v - L(h, state(q)), the prefix WITHOUT the estimate it still carries.  Rows as above.
 *   Mixing as for asg_beam_word_window_result_la: NOTHING HERE CAN CHECK which estimate a state carries.
 * REQUIRED PROPERTIES (no tolerance in any).  (a) Row 0 equals asg_beam_word_window_result(final) (_result_la) on every shared
 * field -- scores, path, tokens, token_lengths, states, lm_states, words, word_lengths, frames, committed, status -- bit for bit.
 * (b) While status bit 0 is clear: for EVERY row, everything advance has committed followed by the row's tail equals row r of
 * asg_beam_word_stream_nbest (_la) on a growing stream fed the same frames, for path, states, lm_states, tokens and words.  Why: a
 * convergence commit stops at a frame c at which every survivor of that moment has the same ancestor slot, so the committed chain
 * is an ancestor chain of every survivor of that frame and of every later one; carry / carry_state are the label and state of
 * frame base-1 on that chain, hence on every row's.  (c) With bit 0 set some frames were committed along the best prefix of the
 * moment only; the rows are then still exactly the chains specified above (deterministic, the same for every chunking) but need
 * not continue the committed prefix, and the word of a separator in column 0 is word_of_state[carry_state], whatever was
 * committed.  (d) The state is only read.
 * There are no emission_scores, graph_scores or lm_scores: the sums of the committed part are gone, and the header keeps
 * carry_state, not the product state or the LM history of frame base-1 that the edge into frame `base` would need.  The state is
 * not widened for them: asg_beam_word_window_state_bytes is unchanged.
 * `work` (asg_beam_word_window_nbest_work_bytes; serves both forms): B * (W*nb*4 rounded up to 256) bytes; its contents mean
 * nothing between calls.  ONE launch on `stream`, one 1024-thread workgroup per slot: no host synchronisation, no copy, no memset
 * -- every output element and every scratch word that is read is written by the kernel -- so a captured call replays.  One integer
 * LDS counter, no atomics on values: bit-identical run to run.  LDS: P2(K) * (8 + e) bytes, P2 the power of two >= K.
 * Errors: those of asg_beam_word_window_result (_result_la), first; nbest < 1: ASG_ERR_INVALID; nbest > 8192:
 * ASG_ERR_UNSUPPORTED; NULL state, work, scores, tokens, token_lengths, words, word_lengths, num_hyps, frames, committed or status:
 * ASG_ERR_INVALID; a `work` smaller than asg_beam_word_window_nbest_work_bytes: ASG_ERR_WORKSPACE.
 * asg_beam_word_window_nbest_work_bytes returns 0 for arguments the call refuses.  `flags` is reserved (pass 0).
 * Not here: score parts from the window, confidences from any stream. */
size_t asg_beam_word_window_nbest_work_bytes(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype,
                                             int beam_size, int64_t W, int64_t P, int nbest);
int asg_beam_word_window_nbest(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                               int64_t W, int64_t P, const void *state, size_t state_bytes, int final, int nbest, void *work,
                               size_t work_bytes, void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                               int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths, int64_t *num_hyps,
                               int64_t *frames, int64_t *committed, int64_t *status, int flags, void *stream);
int asg_beam_word_window_nbest_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                  const asg_word_lookahead *la, int64_t B, int beam_size, int64_t W, int64_t P, const void *state,
                                  size_t state_bytes, int final, int nbest, void *work, size_t work_bytes, void *scores,
                                  int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states,
                                  int64_t *words, int64_t *word_lengths, int64_t *num_hyps, int64_t *frames, int64_t *committed,
                                  int64_t *status, int flags, void *stream);

/* ---- The N BEST hypotheses of the search WITH LM LOOK-AHEAD: asg_beam_decode_words_nbest over the search of
 * asg_beam_decode_words_la, asg_beam_word_stream_nbest over a state that asg_beam_word_stream_advance_la left.  Each entry point is
 * the plain call with `la`, the look-ahead of that search, behind `lm`; everything the plain call's text says holds with the
 * changes below.  No counterpart in the reference.  The search is asg_beam_decode_words_la's, unchanged: the same sets and
 * back-pointers bit for bit (the same device code).  All sums in the dtype of the problem.
 *   candidates and order, final != 0 (the one-shot call always): every pair (h, q) of the last kept set whose end is > -inf, the
 *     end asg_beam_decode_words_la's: (v + final_w[q]) + ew[h] at the root; (v + final_w[q]) + ((a - L(h, state(q))) + ew[h']) in
 *     a word-end node; none mid-word, none where the LM rejects the word.  End descending (-0 equals +0), then pair order.
 *     num_hyps = min(nbest, candidates).
 *   candidates and order, final == 0 (stream only): every kept pair, with the end of asg_beam_word_stream_result_la's prefix rule,
 *     e = v - L(h, state(q)), finite for every kept pair.  e descending, then pair order.  (A mid-word pair with the largest v can
 *     come behind a root pair with a smaller v: its v carries an estimate, its e does not.)
 *   Row r: scores = that end exactly as the rule above forms it.  path, states, lm_states, tokens, token_lengths, words and
 *     word_lengths are asg_beam_decode_words_nbest's, word for word.
 *   THE SCORE SPLIT HAS NO FOURTH PART.  emission_scores, graph_scores and lm_scores are asg_beam_decode_words_nbest's three sums
 *     over the path, term for term; no look-ahead term enters any of them.  Along a complete path every L(h, n) the search added
 *     is taken back -- on the next edge, on the separator edge or at the end -- and in prefix mode the reported end takes back the
 *     one still open: the look-ahead is an estimate that cancels, not a score.  The parts therefore mean what they mean without
 *     look-ahead, and a caller re-weights them exactly as asg_beam_decode_words_nbest says.
 *   scores is the search's own sum, with the cancelling terms rounded in, and NOT the rounded sum of the parts: they agree within
 *     2 * n * eps * (the sum of the magnitudes of the terms), asg_beam_decode_words_nbest's bound with n and the magnitude sum
 *     extended: every look-ahead value the search adds on the path (L of the start pair, L of the target of every edge into a
 *     node) counts twice, once where it enters and once where it leaves (the next edge out of the node, the separator edge, the
 *     end, or the reported prefix).
 *   Padding rows, frames beyond len, the nbest limits: asg_beam_decode_words_nbest's.
 * REQUIRED PROPERTIES (no tolerance).  1. Row 0 of asg_beam_decode_words_nbest_la equals the eight outputs of
 * asg_beam_decode_words_la bit for bit.  2. Row 0 of asg_beam_word_stream_nbest_la equals asg_beam_word_stream_result_la(final) bit
 * for bit, for both values of final; frames and status are that call's.  3. For any chunking of an utterance of at most max_frames
 * frames, the stream's rows with final != 0 equal the one-shot rows bit for bit, on that call's columns.  4. With a beam that
 * prunes nothing and weights in eighths (no sum rounds) the whole list, the three parts included, equals
 * asg_beam_decode_words_nbest's bit for bit.
 * Workspace: asg_beam_decode_words_nbest_work_bytes and asg_beam_word_stream_nbest_work_bytes serve both forms; the look-ahead
 * adds read-only tables and nothing per utterance.  Launches as the plain calls (two on one stream; one for the stream), no
 * memset, no copy, no synchronisation, no float atomics: capturable, bit-identical run to run.
 * Mixing.  As for the streams above: a state advanced with a look-ahead is read with the same look-ahead, one advanced without by
 * asg_beam_word_stream_nbest; the stored values do not say which estimate they carry, and NOTHING HERE CAN CHECK IT.
 * Errors: the plain call's, then asg_beam_decode_words_la's for `la`: a NULL look-ahead, one of another dtype, a NULL or mis-sized
 * array, or S / H other than the LM view's: ASG_ERR_INVALID.  The n best of a window state with look-ahead:
 * asg_beam_word_window_nbest_la above. */
int asg_beam_decode_words_nbest_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                   const asg_word_lookahead *la, int beam_size, double beam_threshold, int nbest, void *work,
                                   size_t work_bytes, void *scores, void *emission_scores, void *graph_scores, void *lm_scores,
                                   int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states,
                                   int64_t *words, int64_t *word_lengths, int64_t *num_hyps, int flags, void *stream);
int asg_beam_word_stream_nbest_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                  const asg_word_lookahead *la, int64_t B, int beam_size, int64_t max_frames, const void *state,
                                  size_t state_bytes, int final, int nbest, void *work, size_t work_bytes, void *scores,
                                  void *graph_scores, void *lm_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                                  int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths, int64_t *num_hyps,
                                  int64_t *frames, int64_t *status, int flags, void *stream);

/* ---- Full score of the ASG lattice COMPOSED with a token automaton (the log-semiring counterpart of the decoder above), its
 * gradients, and the automaton's score of each target: the pieces of an ASG loss whose normaliser includes a token-level
 * prior.  No counterpart in the reference.  For utterance b with len = clamp(input_lengths[b], 0, T), in the dtype of the problem:
 *   alpha[0][q] = start_w[q] + I[0][i]
 *   alpha[t][q] = lse(stay: alpha[t-1][q] + tr[i][i];  edge e from q': (alpha[t-1][q'] + tr[i][src_label[e]]) + edge_w[e]) + I[t][i]
 *   scores[b]   = lse_q(alpha[len-1][q] + final_w[q])        (-inf, never NaN, when len == 0 or no path exists)
 * every lse max-then-sum in a fixed candidate order (the stay first, then the edges ascending).
 * Backward: grad_inputs [T,B,N] (contiguous, every element written, zero rows at t >= len) = grad_scores[b] * the label posteriors;
 * grad_transition [N,N] (contiguous) = sum_b grad_scores[b] * the expected counts of every (i, j) move.  No float atomics and
 * fixed reduction orders: bit-identical run to run on each route.  It needs the alpha that the forward stored in `work`
 * (ASG_FLAG_GRAPH_LOSS_KEEP_ALPHA), the scores of that forward, and the same problem (the emissions and transitions are read again).
 * Target scores: out[b] = arcw[start][y_1] + sum_k arcw[s_k][y_{k+1}] + finw[s_end] over targets[b][:target_lengths[b]] with
 * consecutive equal labels merged, -inf if the automaton rejects them (reads targets, target_lengths and S).
 *   work:    asg_graph_full_work_bytes(p, gl, store) = (store ? T : 2) * Q * B * e bytes (e = 4 or 8)
 *   scratch: asg_graph_full_scratch_bytes(p, gl) = align256(2 * Q * B * e) + (Q + E) * B * e bytes
 * Routes: resident (2*Q*e <= 128 KiB and E <= 4096; one workgroup per utterance) or streaming (one launch per frame and
 * direction).  Limits and validation as asg_viterbi_decode_graph.  Every output is written by kernels (no memset). */
#define ASG_FLAG_GRAPH_LOSS_KEEP_ALPHA 64        /* asg_graph_full_forward: store alpha in `work` for asg_graph_full_backward */
#define ASG_FLAG_GRAPH_LOSS_STREAMING 128   /* take the streaming route (for tests and timings) */
#define ASG_FLAG_GRAPH_LOSS_RESIDENT 256    /* take the resident route wherever the vectors fit (for tests and timings) */
typedef struct asg_token_graph_loss {
    const asg_token_graph *graph;  /* the product graph (its arrays on the device)                         */
    int64_t S;                     /* automaton states                                                      */
    int32_t start;                 /* start state                                                           */
    int32_t reserved;
    const int32_t *tgt;            /* [E] target product state of each incoming edge                       */
    const int32_t *orow;           /* [Q+1] CSR offsets of the outgoing edges of q                         */
    const int32_t *oedge;          /* [E] incoming-edge index of each outgoing edge, ascending by (src, tgt) */
    const int32_t *lrow;           /* [N+1] CSR offsets of the product states of each label                */
    const int32_t *lq;             /* [Q] product states grouped by label, ascending                       */
    const int64_t *pkey;           /* [E] label pair label[tgt] * N + src_label of the edges in pedge order, ascending */
    const int32_t *pedge;          /* [E] incoming-edge indices sorted by pair (stable)                    */
    const int32_t *next;           /* [S,N] next state, -1 where no arc                                    */
    const void *arcw;              /* [S,N] folded arc weights, -inf where no arc                          */
    const void *finw;              /* [S] folded final weights, -inf where not accepting                   */
} asg_token_graph_loss;
size_t asg_graph_full_work_bytes(const asg_problem *p, const asg_token_graph_loss *gl, int store);
size_t asg_graph_full_scratch_bytes(const asg_problem *p, const asg_token_graph_loss *gl);
int asg_graph_full_forward(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_loss *gl, void *work, size_t work_bytes,
                           void *scores, int flags, void *stream);
int asg_graph_full_backward(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_loss *gl, const void *work,
                            size_t work_bytes, const void *scores, const void *grad_scores, void *grad_inputs,
                            void *grad_transition, void *scratch, size_t scratch_bytes, int flags, void *stream);
int asg_graph_target_scores(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_loss *gl, void *out, void *stream);

/* ---- BEAM-PRUNED full score of the same composed lattice, and its gradients: asg_graph_full_forward / _backward over the
 * lattice that asg_beam_decode_graph's search keeps -- a normaliser Z_K whose work per frame follows the beam and not Q or E, so a
 * criterion can be trained with the automata (4-grams, lexicon tries) the beam decoder was built for.  No counterpart in the
 * reference.  Per utterance b, len = clamp(input_lengths[b], 0, T); product graph, folding, start_w, final_w, edge_w as in
 * asg_viterbi_decode_graph:
 *   1. Kept sets.  A_t, t = 0 .. len-1, are exactly the active sets of asg_beam_decode_graph for the same emissions, transition,
 *      graph, beam_size, beam_threshold, computed in the dtype of the problem (the same device code runs).  They are a discrete
 *      function of the inputs and constants to the gradient.
 *   2. Forced target states (only when p->targets is given).  y = targets[b][:clamp(target_lengths[b], 0, S)] with consecutive
 *      equal labels merged, n = |y|, s_0 = start, s_k = next[s_{k-1}][y_k], q_k = the product state (y_k, s_k), k = 1 .. n.
 *      F_t = { q_k : k-1 <= t and n-k <= len-1-t }.  Every F_t is empty when the target has no alignment (target length 0 or
 *      > len), holds a label outside [0, N), or the automaton rejects it (a missing arc, or final_w[q_n] = -inf).  The forced
 *      states do NOT feed back into the search of step 1.
 *   3. Lattice.  U_t = A_t united with F_t, ascending by q, no duplicates.
 *        alpha[0][q] = start_w[q] + I[0][i(q)]                                                          for q in U_0
 *        alpha[t][q] = lse(stay: alpha[t-1][q] + tr[i][i] if q in U_{t-1};  every edge q' -> q with q' in U_{t-1}:
 *                          (alpha[t-1][q'] + tr[i][j]) + edge_w) + I[t][i]                               for q in U_t
 *        scores[b] = Z_K = lse over q in U_{len-1} of (alpha[len-1][q] + final_w[q])
 *      Every lse is max-then-sum over the stay, then the edges ascending by source (asg_graph_full_forward's order restricted to
 *      the kept sources; the lanes that share a target meet in a fixed tree); all candidates -inf gives -inf, never NaN.
 *      len == 0 or an empty lattice: -inf.  beta, the label posteriors and the expected (i, j) counts are the mirror image
 *      over the same U_t; grad_inputs [T,B,N] (contiguous, every element written, zero rows at t >= len) and grad_transition
 *      [N,N] as asg_graph_full_backward.
 *   Z_K <= asg_graph_full_forward's score (a subset of its paths); without targets Z_K >= asg_beam_decode_graph's score; with
 *   beam_size >= Q and beam_threshold = +inf, U_t is every state with a finite alpha and everything equals asg_graph_full_*.
 *   With targets, every alignment of the target runs through the F_t, so Z_K - (aligned score + automaton score) >= 0 for ANY beam.
 * No float atomics: posteriors are summed as 64-bit fixed-point integers (62 fractional bits for a frame's label posteriors,
 * 62 - ceil(log2(len)) for an utterance's (i, j) counts) and the utterances are added in ascending order: bit-identical run to
 * run.  ASG_FLAG_BEAM_LOSS_ACCUMULATE (backward) continues that sum from what grad_transition holds, so a batch processed in
 * consecutive groups gives the bits of one call.  Every output and all scratch that is read is written by kernels (no memset).
 * K = min(beam_size, max(Q, 1)); nf = min(S, T) when p->targets is given, else 0; M = K + nf.  Every part rounded up to 256 bytes:
 *   work:    asg_beam_graph_full_work_bytes(p, gl, beam_size, store) =
 *            B * (asg_beam_decode_graph's bytes per utterance + 2*T*4 + 256 + nf*12 + T*M*4 + (store ? T : 2)*M*e)
 *            + 2*B*8 + 3*B*T*8          (what the search itself returns)
 *   scratch: asg_beam_graph_full_scratch_bytes(p, gl, beam_size) = B * (2*M*e + N*N*8)
 * Neither depends on E; Q enters only through the search's own slot arrays (Q*(8+e) per utterance).
 * The forward keeps alpha for the backward with ASG_FLAG_GRAPH_LOSS_KEEP_ALPHA; the backward takes the same problem (targets
 * included: they size the layout), the same beam_size, that work buffer and the scores of that forward.
 * Limits (ASG_ERR_UNSUPPORTED beyond): those of asg_beam_decode_graph (K <= 8192, ...), N <= 1024 (a frame's label posteriors
 * are summed in LDS, and the (i, j) counts too while they fit beside the lattice), min(S, T) <= 2048 with targets, T <= 2^20.  beam_size < 1, a
 * negative or NaN beam_threshold: ASG_ERR_INVALID.  float32 and float64. */
#define ASG_FLAG_BEAM_LOSS_ACCUMULATE 512   /* asg_beam_graph_full_backward: grad_transition += (it must hold finite values) */
typedef struct asg_token_graph_beam_loss {
    const asg_token_graph_beam *beam;  /* the source-side graph of asg_beam_decode_graph (and through it the product graph) */
    int64_t S;                         /* automaton states                                                               */
    int32_t start;                     /* start state                                                                    */
    int32_t reserved;
    const int32_t *next;               /* [S,N] next state, -1 where no arc                                              */
} asg_token_graph_beam_loss;
size_t asg_beam_graph_full_work_bytes(const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size, int store);
size_t asg_beam_graph_full_scratch_bytes(const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size);
int asg_beam_graph_full_forward(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                                double beam_threshold, void *work, size_t work_bytes, void *scores, int flags, void *stream);
int asg_beam_graph_full_backward(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                                 const void *work, size_t work_bytes, const void *scores, const void *grad_scores,
                                 void *grad_inputs, void *grad_transition, void *scratch, size_t scratch_bytes, int flags,
                                 void *stream);

/* ---- TOKEN CONFIDENCES and START FRAMES of asg_beam_decode_graph's hypothesis, from the lattice its search kept: for every token
 * of the winning path, the frame it starts at and how much of the probability mass inside the kept sets agrees that a token with
 * this label starts there -- what pseudo-label filters, highlighting of doubtful characters and token time stamps need.  With a
 * lexicon trie (TokenGraph.from_lexicon) the confidence of a separator token is the confidence of a word boundary.  No counterpart
 * in the reference.  Per utterance b, len = clamp(input_lengths[b], 0, T); graph, folded weights, the kept sets A_t
 * (K = min(beam_size, max(Q, 1))), the edges and the end exactly as in asg_beam_decode_graph / asg_beam_graph_full_forward WITHOUT
 * targets (p->targets is not looked at): U_t = A_t.
 *   1. Lattice paths.  A path is p_0 .. p_{len-1} with p_t in A_t, consecutive states equal (the stay) or joined by one outgoing
 *      edge of the product graph, and a finite end.  Its weight is what step 3 of asg_beam_graph_full_forward sums.  Z_K = lse over
 *      all of them = that call's score without targets, bit for bit (the same kernels run).  The winning path is one of them.
 *   2. Token events.  A path STARTS A TOKEN WITH LABEL i AT FRAME t when t == 0 and p_0 has label i, or 1 <= t <= len-1,
 *      p_t != p_{t-1} and p_t has label i (an edge of the product graph always changes the label: "not the stay").
 *      P(i, t) = sum over the paths with that event of exp(weight - Z_K): automaton states and source states are summed over.
 *   3. Hypothesis.  Token k of the winning path, k < token_lengths[b], has label c_k = tokens[b][k] and starts at s_k, the first
 *      frame of its run in path[b] (s_0 = 0).  s_k ascends strictly.
 *   4. Outputs.  scores, path, tokens, token_lengths, states: asg_beam_decode_graph's own, bit for bit (the same device code
 *      searches, ends and backtraces).  Beyond them:
 *        token_frames      [B][T] int64: s_k, then -1 behind the tokens;
 *        token_confidences [B][T] dtype: conf_k = sum over t in [s_k - tol, s_k + tol] meet [0, len-1] of P(c_k, t), then 0;
 *        normalisers       [B]    dtype: Z_K.
 *      tol = frame_tolerance.  At tol = 0, conf_k is a probability: exp(scores[b] - Z_K) <= conf_k <= 1 up to rounding (the
 *      winning path has the event).  At tol > 0 it is the EXPECTED NUMBER of starts of label c_k inside the window: it can pass 1
 *      ("a b a" inside one window starts a twice) and is returned unclipped.
 *   5. Degenerate utterances.  len == 0, an empty last set or no finite end: score -inf, normaliser -inf, integer outputs -1,
 *      lengths 0, confidences 0.  Never a NaN.
 * An edge posterior is exp((alpha[t-1][p] + c) - Z_K), c = beta[t][p'] + the edge's terms, with alpha of
 * asg_beam_graph_full_forward and beta its mirror image (max-then-sum per state, the sums of asg_beam_graph_full_backward); the
 * posterior of a start at frame 0 is exp((alpha[0][q] + beta[0][q]) - Z_K).  Each is added to the tokens it counts for as a 64-bit
 * fixed-point integer with 54 fractional bits: integer adds only, NO FLOAT ATOMICS, bit-identical run to run and for any grouping
 * of the batch.  Every output and every workspace word that is read is written by kernels (no memset, no host synchronisation):
 * the call can be captured and replayed.  The frame loop of the search runs ONCE per utterance.
 * M = K, e = 4 / 8.  Every part rounded up to 256 bytes:
 *   work: asg_beam_graph_confidence_work_bytes(p, gl, beam_size) =
 *         B * (asg_beam_graph_full_work_bytes' bytes per utterance without targets at store = 1, i.e.
 *              asg_beam_decode_graph's bytes per utterance + 2*T*4 + 256 + T*M*4 + T*M*e,     + 2*M*e (two rows of beta))
 * The search writes the caller's outputs, so there is no part behind the utterances; the token accumulators live in LDS.  No term
 * in S or E and none in N*N (no (i, j) tile is kept); targets in the problem change nothing.
 * Limits (ASG_ERR_UNSUPPORTED beyond): those of asg_beam_graph_full_forward without targets, and frame_tolerance <= 64;
 * frame_tolerance < 0: ASG_ERR_INVALID.  Argument errors, in this order: asg_beam_graph_full_forward's for p, gl and beam_size;
 * beam_threshold; frame_tolerance; a NULL buffer; ASG_ERR_WORKSPACE.  float32 and float64. */
size_t asg_beam_graph_confidence_work_bytes(const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size);
int asg_beam_graph_confidence(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                              double beam_threshold, int frame_tolerance, void *work, size_t work_bytes, void *scores,
                              int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *token_frames,
                              void *token_confidences, void *normalisers, int flags, void *stream);

/* ---- TOKEN CONFIDENCES and START FRAMES for EVERY ROW of asg_beam_decode_graph_nbest's list: what rescoring with a per-token
 * posterior, ROVER-style combination of the rows and pseudo-labelling on the tokens the rows agree on need, from ONE search.  The
 * quantity is not new: P(i, t) of asg_beam_graph_confidence does not depend on the hypothesis; a row only selects which
 * (frame, label) cells are read.  Per utterance b everything is asg_beam_decode_graph_nbest's and asg_beam_graph_confidence's on
 * the same arguments: the same search, run ONCE; the same kept sets A_t, candidates, order and num_hyps; the lattice with
 * U_t = A_t (p->targets is not looked at); the same Z_K; the same token events P(i, t).  The argument order is
 * asg_beam_decode_graph_nbest's with the view of asg_beam_graph_confidence in place of the beam view, frame_tolerance behind nbest
 * and token_frames, token_confidences, normalisers behind num_hyps.
 *   1. The eight n-best outputs of asg_beam_decode_graph_nbest, bit for bit (the same device text ranks, walks and writes).
 *      path and states may be NULL.
 *   2. token_frames [B][nbest][T] int64.  For row r < num_hyps[b] and k < token_lengths[b][r], s_{r,k} is the first frame of the
 *      k-th run of labels in the row's back-pointer path (step 3 of asg_beam_graph_confidence, applied to the row's path;
 *      s_{r,0} = 0).  It ascends strictly within a row.  -1 behind the tokens and in padding rows.
 *   3. token_confidences [B][nbest][T] dtype.  conf_{r,k} = sum of P(tokens[b][r][k], t) over t in [s_{r,k} - tol, s_{r,k} + tol]
 *      meet [0, len-1]; 0 behind the tokens and in padding rows; unclipped.  tol = frame_tolerance.
 *   4. normalisers [B] dtype: Z_K, asg_beam_graph_full_forward's score without targets bit for bit.
 * Properties.  Row 0's frames and confidences are asg_beam_graph_confidence's on the same arguments, bit for bit: an event is
 * added as the same 54-bit fixed-point integer, an integer sum does not depend on its order, and the conversion is the same
 * expression.  At tol = 0, exp(scores[b][r] - Z_K) <= conf_{r,k} <= 1 up to rounding for every row: a row's path is a lattice
 * path that has the event.  Rows that start the same label at the same frame get the same bits (they read one cell).  Degenerate
 * utterances (len == 0, an empty last set, no finite end): num_hyps 0, scores -inf, normaliser -inf, frames -1, confidences 0;
 * never a NaN.  NO FLOAT ATOMICS, no memset, no host synchronisation: bit-identical run to run and for any grouping of the
 * batch, and the call can be captured and replayed.  The frame loop of the search runs ONCE per utterance.
 * K = min(beam_size, max(Q, 1)), M = K, e = 4 / 8, nb = min(nbest, K), P2(x) = the power of two >= max(x, 2).  Every part rounded
 * up to 256 bytes:
 *   work: asg_beam_graph_nbest_confidence_work_bytes(p, gl, beam_size, nbest) =
 *         B * (asg_beam_graph_confidence_work_bytes' bytes per utterance
 *              + 8 + K*e (the last set) + T*nb*4 (the rows' product states) + 256 + (T+2)*4 (the first cell of every frame)
 *              + P2(nb*T)*8 (the rows' queries) + nb*T*8 (the cells) + nb*T*8 (their sums))
 *         + 2 * (B*8) + 3*B*T*8 (the one-best outputs of the search).
 * No term in S, E or N*N; targets in the problem change nothing.
 * Limits: the union of the two parent calls': nbest < 1 or frame_tolerance < 0: ASG_ERR_INVALID; nbest > 8192 or
 * frame_tolerance > 64: ASG_ERR_UNSUPPORTED; the limits of asg_beam_graph_confidence.  ONE new limit (ASG_ERR_UNSUPPORTED
 * beyond): the accumulators of the open cells live in LDS beside a frame's lattice set,
 *         16 * ceil(M*(e+4) / 16) + 1024 + 12 * P2(min(nbest, K) * (2*frame_tolerance + 2)) <= 163840   and   nb*T <= 2^30.
 * (A frame holds a label once among its cells, so min(nbest, K, N) rows would do; the bound keeps the expression of
 * asg_beam_words_nbest_confidence, whose ring function it shares.)
 * Argument errors, in this order: asg_beam_graph_confidence's for p, gl and beam_size; nbest; frame_tolerance and the new limit;
 * the threshold; a NULL among work and the outputs other than path and states; the workspace.  float32 and float64. */
size_t asg_beam_graph_nbest_confidence_work_bytes(const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                                                  int nbest);
int asg_beam_graph_nbest_confidence(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                                    double beam_threshold, int nbest, int frame_tolerance, void *work, size_t work_bytes,
                                    void *scores, void *emission_scores, void *graph_scores, int64_t *path, int64_t *tokens,
                                    int64_t *token_lengths, int64_t *states, int64_t *num_hyps, int64_t *token_frames,
                                    void *token_confidences, void *normalisers, int flags, void *stream);

/* ---- the LATTICE-KEEPING beam stream: asg_beam_stream_* with a state that also keeps what asg_beam_graph_confidence computes
 * its token confidences from, so that a stream gives a confidence and a start frame per token while the utterance is arriving
 * (additions only; asg_beam_stream_* and its state formula are unchanged).  The family takes the asg_token_graph_beam_loss view,
 * as asg_beam_graph_confidence does (the alpha pull reads the incoming rows), in asg_beam_stream_*'s argument order.
 *
 * STATE.  With a256(x) = x rounded up to 256, e = 4 or 8 (the dtype), T = max_frames, K = min(beam_size, Q), N = gl->beam->graph->N,
 * one slot is
 *     per = P + a256(4 T) + a256(e T N) + a256(4 T) + a256(4 T K) + a256(e T K) + a256(2 e K),
 * where P = asg_beam_stream_state_bytes(gl->beam, 1, dtype, beam_size, max_frames) is the plain stream's slot, unchanged, at the
 * front (the search's workspace, the header, the stored set), and behind it: cnt int32 [T] (|A_t| of every consumed frame), the
 * emissions [T][N], nu int32 [T], U int32 [T][K] (A_t ascending), A [T][K] (alpha), beta [2][K].  The header's fourth int32 word
 * is apos, the number of frames whose U / nu / A rows are valid (0 <= apos <= pos).  asg_beam_conf_stream_state_bytes = B * per.
 *
 * _reset, _advance, _result, _nbest and _nbest_work_bytes: asg_beam_stream_*'s, argument for argument and bit for bit (the frames
 * run the same device text; _result and _nbest run the plain stream's kernels over the wider slots).  _reset also sets apos = 0,
 * a masked reset in the chosen slots only.  _advance also writes, for every frame gt it consumes, cnt[gt] = min(|A_gt|, K) -- 0 for
 * the frames an empty beam skips -- and the frame's N emissions into row gt (a coalesced copy from the chunk's strides).
 *
 * _confidence(final, frame_tolerance): TWO launches, no host synchronisation, no memset, no copy; it captures and replays.
 *   (a) catch-up: for every slot U, nu and A are brought from apos up to pos (the sets are A_t sorted: no targets, nothing forced;
 *       alpha is asg_beam_graph_full_forward's pull, the same device text, resumed from rows apos-1 or from the start weights),
 *       then apos = pos.  THE ONE CALL OF THE FAMILY THAT WRITES THE STATE FROM A RESULT PATH: what it writes is idempotent and
 *       does not depend on `final` or the tolerance -- every frame's alpha is computed once, however often confidences are asked
 *       for -- and an _advance costs the plain one's plus a copy of N values per frame.
 *   (b) the hypothesis, Z and the beta pull.  Let L = pos.  The lattice: the kept sets A_0 .. A_{L-1}, the edges and weights of
 *       asg_beam_graph_confidence.
 *       final = 1: everything is asg_beam_graph_confidence's on x[0:L].  For ANY chunking of x[0:L], L <= max_frames, and wherever
 *         _confidence calls fall in between, _confidence(1, tol) equals asg_beam_graph_confidence(x, tol): scores, normalisers,
 *         token_lengths, token_frames and token_confidences bit for bit; the integer arrays on the one-shot's columns and -1
 *         beyond; the confidences 0 beyond.  No tolerance is involved.
 *       final = 0 (prefix): a path ends in any state of A_{L-1} with end weight 0; Z (normalisers) is the log-sum-exp of alpha
 *         over A_{L-1}; the hypothesis is _result(final = 0)'s; events and windows as asg_beam_graph_confidence's.  At
 *         frame_tolerance 0, exp(scores - Z) <= confidence <= 1 up to rounding.
 *       L = 0, an empty last set or no finite end: -inf, -inf, -1 and 0, never a NaN.  status is the overflow word, frames is L.
 *   outputs: scores [B], path / tokens / states / token_frames [B][max_frames] int64, token_lengths [B], token_confidences
 *   [B][max_frames] and normalisers [B] in the dtype, frames [B], status [B].
 *   `transition` ([N][N] in the dtype, strides in elements) MUST NOT CHANGE within an utterance for the property to hold: _advance
 *   reads it at the chunk, the lattice pass at the call, and a change in between gives sets and weights from different matrices.
 * Limits: asg_beam_stream_*'s and asg_beam_graph_confidence's (for T = max_frames).  frame_tolerance in 0 .. 64: negative is
 * ASG_ERR_INVALID, larger ASG_ERR_UNSUPPORTED; a state that is too small ASG_ERR_WORKSPACE.  float32 and float64. */
size_t asg_beam_conf_stream_state_bytes(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size,
                                        int64_t max_frames);
int asg_beam_conf_stream_reset(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t max_frames,
                               void *state, size_t state_bytes, const uint8_t *mask, int flags, void *stream);
int asg_beam_conf_stream_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                                 double beam_threshold, int64_t max_frames, void *state, size_t state_bytes, int flags,
                                 void *stream);
int asg_beam_conf_stream_result(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t max_frames,
                                const void *state, size_t state_bytes, int final, void *scores, int64_t *path, int64_t *tokens,
                                int64_t *token_lengths, int64_t *states, int64_t *frames, int64_t *status, int flags, void *stream);
size_t asg_beam_conf_stream_nbest_work_bytes(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size,
                                             int64_t max_frames, int nbest);
int asg_beam_conf_stream_nbest(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t max_frames,
                               const void *state, size_t state_bytes, int final, int nbest, void *work, size_t work_bytes,
                               void *scores, void *graph_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                               int64_t *states, int64_t *num_hyps, int64_t *frames, int64_t *status, int flags, void *stream);
int asg_beam_conf_stream_confidence(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t max_frames,
                                    void *state, size_t state_bytes, const void *transition, const int64_t *transition_strides,
                                    int final, int frame_tolerance, void *scores, int64_t *path, int64_t *tokens,
                                    int64_t *token_lengths, int64_t *states, int64_t *token_frames, void *token_confidences,
                                    void *normalisers, int64_t *frames, int64_t *status, int flags, void *stream);

/* ---- the LATTICE-KEEPING window stream: asg_beam_window_* with a state that also keeps, in a ring, what
 * asg_beam_graph_confidence computes its token confidences from, so that a stream WITHOUT A BOUND on its frames gives a confidence
 * and a start frame for every token at the moment it commits it (additions only; asg_beam_window_* and its state formula are
 * unchanged).  The family takes the asg_token_graph_beam_loss view, as asg_beam_conf_stream_* does, in asg_beam_window_*'s
 * argument order with two more parameters of the state behind W and P: frame_tolerance (tol, 0 .. 64) and max_chunk (C >= 1, the
 * longest chunk an _advance may bring).  The state is sized by them and every call passes the same four values.
 *
 * DEFINITION.  The window never touches the search, so the kept sets A_0 .. A_{pos-1} are those of asg_beam_conf_stream_* fed the
 * same frames, and the lattice is its lattice: those sets with the edges and weights of asg_beam_graph_confidence.  A confidence
 * belongs to a (frame, label) cell.  Take a commit attempt behind frame p1 - 1 (pos, counting the frame, is p1, and p1 mod P == 0).
 * For a token that attempt commits, with label i and a run that starts at frame f:
 *   new_token_frames      = f, the absolute frame at which the carried collapse kept the label (a first committed label that
 *                           differs from `carry` starts at the old base);
 *   new_token_confidences = the prefix-mode posterior of asg_beam_conf_stream_confidence over A_0 .. A_{p1-1}: a path ends in any
 *                           state of A_{p1-1} with end weight 0, Z is the log-sum-exp of alpha over A_{p1-1}, and the value sums
 *                           the event "a token with label i starts at frame t" over t in [f - tol, f + tol] clipped to [0, p1-1].
 * It is what a listener knows at the moment the token becomes final.  A forced commit of the same attempt uses the same p1: one
 * attempt is one lattice end.  No finite Z at the attempt: confidence 0, the frame still written; never a NaN.
 *   - The five outputs of asg_beam_window_advance, and _result, _nbest and _reset, are the plain family's byte for byte.
 *   - The concatenation of all new_token_frames / new_token_confidences is the same bits for every chunking (attempts, and so
 *     lattice ends, happen at frame indices).
 *   - While status bit 0 is clear, the tokens an attempt at p1 commits carry, at the same token indices, the token_frames and
 *     token_confidences of asg_beam_conf_stream_confidence(final = 0, tol) of a growing stream that stands at pos = p1, bit for
 *     bit: the alpha text is the same, resumed from stored rows; the sets are the same ascending lists; Z is the same; the beta
 *     recursion is the same from frame p1 - 1 downwards, and the integer accumulators do not depend on the order of the adds.
 *   - With status bit 0 set the values are still the cell posteriors defined above.
 *
 * STATE.  With a256(x) = x rounded up to 256, e = 4 or 8 (the dtype), K = min(beam_size, Q), N = gl->beam->graph->N,
 *     RW = W + tol + 1 + C   (rows of the lattice ring; frame t lives in row t mod RW, computed in 64 bits),
 *     L  = C / P + 1         (entries of the attempt log, integer division),
 * one slot is
 *     per = PW + a256(4 RW) + a256(e RW N) + a256(4 RW) + a256(4 RW K) + a256(e RW K) + a256(24 L) + L a256(2 e K),
 * where PW = asg_beam_window_state_bytes(gl->beam, 1, dtype, beam_size, W, P) is the plain window's slot, unchanged, at the front,
 * and behind it: cnt int32 [RW], the emissions [RW][N], nu int32 [RW], U int32 [RW][K] (A_t, ascending once caught up), A [RW][K]
 * (alpha), the attempt log (int64 p1, int64 base before the attempt, int32 first and one-past-last token of the call's output
 * row), beta [L][2][K].  The slot's 256-byte header block holds, at byte 64, int64 apos (the frames whose U / nu / A rows are
 * valid, pos - C <= apos <= pos) and int32 the number of attempts the last _advance logged.  asg_beam_conf_window_state_bytes =
 * B * per.  The ring is large enough: an attempt at p1 with old base b0 reads the frames b0 - tol - 1 .. p1 - 1, p1 - b0 <= W, and
 * the call has written at most C frames behind p1.
 *
 * _advance: THREE launches, no host synchronisation, no memset, no copy; it captures and replays.
 *   (a) the search: asg_beam_window_advance's kernel, which also copies the chunk's emissions, |A_t| and the kept states of every
 *       frame into the ring, writes new_token_frames, and logs every attempt that committed a token;
 *   (b) the catch-up over [apos, pos): the rows' states sorted, alpha by asg_beam_graph_full_forward's pull, resumed from row
 *       apos - 1 (or the start weights); apos = pos;
 *   (c) the pull, one workgroup per (slot, logged attempt): Z over row p1 - 1, beta from frame p1 - 1 down to max(b0 - tol, 0),
 *       with the frame-0 term when it gets there; the attempt's tokens are its sink.
 *   outputs: asg_beam_window_advance's five, then new_token_frames int64 [B][W + Tc] (-1 behind the data) and
 *   new_token_confidences [B][W + Tc] in the dtype (0 behind the data).  Every element is written, also for Tc = 0.
 *   Tc > max_chunk is ASG_ERR_UNSUPPORTED.  p->transition MUST NOT CHANGE within an utterance.
 * _reset, _result, _nbest, _nbest_work_bytes: asg_beam_window_*'s over the wider slot (a reset needs nothing more: the next
 *   _advance finds pos = 0 and takes apos back to it).
 * _confidence(final): TWO launches; it only reads the state (beta rows apart).  _result(final)'s eight outputs, and for the
 *   tokens of the uncommitted tail token_frames int64 [B][W] (absolute, -1 behind the data), token_confidences [B][W] (0 behind
 *   the data) and normalisers [B]: one pull from frame pos - 1 down to base - tol with the state's tolerance, end weight 0
 *   (final = 0) or the final weights (final = 1).  With final = 1 and status bit 0 clear the tail's values are
 *   asg_beam_graph_confidence's for those tokens on the frames consumed, bit for bit, and the start frames of all _advance calls
 *   followed by the tail's are its token_frames.  The catch-up was done by _advance.
 * Limits: asg_beam_window_*'s and asg_beam_graph_confidence's (for T = W); frame_tolerance < 0 or max_chunk < 1 is
 * ASG_ERR_INVALID, frame_tolerance > 64 ASG_ERR_UNSUPPORTED; L = max_chunk / P + 1 > 65535 (the pull runs one workgroup per slot
 * and log entry) ASG_ERR_UNSUPPORTED, from every call of the family; a state that is too small ASG_ERR_WORKSPACE.  float32 and
 * float64.  alpha and Z grow with pos, as the search's own scores do: in float32 a posterior loses resolution as |Z| passes about 1e5, so
 * streams of hours want float64 (a rebased alpha is not there). */
size_t asg_beam_conf_window_state_bytes(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size, int64_t W,
                                        int64_t P, int frame_tolerance, int64_t max_chunk);
int asg_beam_conf_window_reset(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t W, int64_t P,
                               int frame_tolerance, int64_t max_chunk, void *state, size_t state_bytes, const uint8_t *mask,
                               int flags, void *stream);
int asg_beam_conf_window_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam_loss *gl, int beam_size,
                                 double beam_threshold, int64_t W, int64_t P, int frame_tolerance, int64_t max_chunk, void *state,
                                 size_t state_bytes, int64_t *new_path, int64_t *new_states, int64_t *new_tokens,
                                 int64_t *new_frames, int64_t *new_token_lengths, int64_t *new_token_frames,
                                 void *new_token_confidences, int flags, void *stream);
int asg_beam_conf_window_result(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t W, int64_t P,
                                int frame_tolerance, int64_t max_chunk, const void *state, size_t state_bytes, int final,
                                void *scores, int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states,
                                int64_t *frames, int64_t *committed, int64_t *status, int flags, void *stream);
size_t asg_beam_conf_window_nbest_work_bytes(const asg_token_graph_beam_loss *gl, int64_t B, int dtype, int beam_size, int64_t W,
                                             int64_t P, int frame_tolerance, int64_t max_chunk, int nbest);
int asg_beam_conf_window_nbest(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t W, int64_t P,
                               int frame_tolerance, int64_t max_chunk, const void *state, size_t state_bytes, int final, int nbest,
                               void *work, size_t work_bytes, void *scores, int64_t *path, int64_t *tokens,
                               int64_t *token_lengths, int64_t *states, int64_t *num_hyps, int64_t *frames, int64_t *committed,
                               int64_t *status, int flags, void *stream);
int asg_beam_conf_window_confidence(asg_ctx *ctx, const asg_token_graph_beam_loss *gl, int64_t B, int beam_size, int64_t W,
                                    int64_t P, int frame_tolerance, int64_t max_chunk, void *state, size_t state_bytes,
                                    const void *transition, const int64_t *transition_strides, int final, void *scores,
                                    int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *token_frames,
                                    void *token_confidences, void *normalisers, int64_t *frames, int64_t *committed,
                                    int64_t *status, int flags, void *stream);

/* ---- the LATTICE-KEEPING word-LM beam stream: asg_beam_word_stream_* with a state that also keeps what asg_beam_words_confidence
 * computes its word confidences from, so that a stream over a lexicon and a word n-gram LM gives a confidence and an end frame per
 * word while the utterance is arriving (additions only; asg_beam_word_stream_* and its state formula are unchanged).  The family
 * takes the word stream's own views, asg_token_graph_beam + asg_word_lm (+ asg_word_lookahead behind them in the _la forms), as
 * asg_beam_words_confidence takes them, in asg_beam_word_stream_*'s argument order and with its error order.
 *
 * STATE.  With a256(x) = x rounded up to 256, e = 4 or 8 (the dtype), T = max_frames, K = beam_size, N = gb->graph->N, one slot is
 *     per = P + a256(4 T) + a256(e T N) + a256(4 T) + a256(8 T K) + a256(e T K) + a256(2 e K),
 * where P = asg_beam_word_stream_state_bytes(gb, lm, 1, dtype, beam_size, max_frames) is the plain word stream's slot, unchanged, at
 * the front (the search's workspace, the header, the stored set), and behind it: cnt int32 [T] (|A_t| of every consumed frame),
 * the emissions [T][N], nu int32 [T], U u64 [T][K] (the pairs of A_t as keys h << qbits | q, ascending), A [T][K] (alpha), beta
 * [2][K].  The header's fourth int32 word is apos, the number of frames whose U / nu / A rows are valid (0 <= apos <= pos).
 * asg_beam_word_conf_stream_state_bytes = B * per; no term in H, V, A or Q.  The state is the same with and without a look-ahead.
 *
 * _reset, _advance[_la], _result[_la], _nbest[_la] and _nbest_work_bytes: asg_beam_word_stream_*'s, argument for argument and bit
 * for bit (the frames run the same device text; _result and _nbest run the plain stream's kernels over the wider slots).  _reset
 * also sets apos = 0, a masked reset in the chosen slots only.  _advance also writes, for every frame gt it consumes, cnt[gt] =
 * min(|A_gt|, K) -- 0 for the frames an empty beam skips -- and the frame's N emissions into row gt (a coalesced copy from the
 * chunk's strides).
 *
 * _confidence[_la](final, frame_tolerance): TWO launches, no host synchronisation, no memset, no copy; it captures and replays.
 *   (a) catch-up: for every slot U, nu and A are brought from apos up to pos (the sets are the keys of A_t sorted: no targets,
 *       nothing forced; alpha is asg_beam_words_full_forward's push, the same device text, resumed from rows apos-1 or from the
 *       start weights), then apos = pos.  THE ONE CALL OF THE FAMILY THAT WRITES THE STATE FROM A RESULT PATH: what it writes is
 *       idempotent and does not depend on `final` or the tolerance -- every frame's alpha is computed once, however often
 *       confidences are asked for -- and an _advance costs the plain one's plus a copy of N values per frame.
 *   (b) the hypothesis, Z and the beta pull.  Let L = pos.  The lattice: the kept pair sets A_0 .. A_{L-1}, the edges and PLAIN
 *       weights of asg_beam_words_confidence; with a look-ahead the sets are the look-ahead search's and the weights stay plain.
 *       final = 1: everything is asg_beam_words_confidence's (asg_beam_words_confidence_la's with the same look-ahead) on x[0:L].
 *         For ANY chunking of x[0:L], L <= max_frames, and wherever _confidence calls fall in between, _confidence(1, tol) equals
 *         that call at tol: scores, normalisers, both lengths, word_frames and word_confidences bit for bit; the integer arrays on
 *         the one-shot's columns and -1 beyond; the confidences 0 beyond.  No tolerance is involved.
 *       final = 0 (prefix): a path ends in any pair of A_{L-1} with end weight 0 -- no final weight, no LM end, no final word; Z
 *         (normalisers) is the log-sum-exp of alpha over A_{L-1}; the hypothesis is _result(final = 0)'s (with a look-ahead the
 *         prefix of largest value without the estimate it still carries, and that value); word events are separator edges only,
 *         at frames 1 .. L-1: the event at frame L of asg_beam_words_confidence does not exist, and word_lengths counts the
 *         separator words.  At frame_tolerance 0, exp(scores - Z) <= confidence <= 1 up to rounding.
 *       L = 0, an empty last set or no finite end: -inf, -inf, -1 and 0, never a NaN.  status is the overflow word, frames is L.
 *   outputs: scores [B], path / tokens / states / lm_states / words / word_frames [B][max_frames] int64, token_lengths and
 *   word_lengths [B], word_confidences [B][max_frames] and normalisers [B] in the dtype, frames [B], status [B].
 *   `transition` ([N][N] in the dtype, strides in elements) MUST NOT CHANGE within an utterance for the property to hold: _advance
 *   reads it at the chunk, the lattice pass at the call, and a change in between gives sets and weights from different matrices.
 * Limits: asg_beam_word_stream_*'s and asg_beam_words_confidence's for T = max_frames -- a frame's set with a maximum and a sum per
 * member must stay in LDS (beam_size <= 8179 float32, 6816 float64), so a lattice-keeping stream refuses, with
 * ASG_ERR_UNSUPPORTED from _state_bytes (0) on, a beam_size that the plain stream accepts.  frame_tolerance in 0 .. 64: negative
 * is ASG_ERR_INVALID, larger ASG_ERR_UNSUPPORTED; a state that is too small ASG_ERR_WORKSPACE.  float32 and float64. */
size_t asg_beam_word_conf_stream_state_bytes(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype,
                                             int beam_size, int64_t max_frames);
int asg_beam_word_conf_stream_reset(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                                    int64_t max_frames, void *state, size_t state_bytes, const uint8_t *mask, int flags,
                                    void *stream);
int asg_beam_word_conf_stream_advance(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                      int beam_size, double beam_threshold, int64_t max_frames, void *state, size_t state_bytes,
                                      int flags, void *stream);
int asg_beam_word_conf_stream_advance_la(asg_ctx *ctx, const asg_problem *p, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                         const asg_word_lookahead *la, int beam_size, double beam_threshold, int64_t max_frames,
                                         void *state, size_t state_bytes, int flags, void *stream);
int asg_beam_word_conf_stream_result(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                                     int64_t max_frames, const void *state, size_t state_bytes, int final, void *scores,
                                     int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states,
                                     int64_t *words, int64_t *word_lengths, int64_t *frames, int64_t *status, int flags,
                                     void *stream);
int asg_beam_word_conf_stream_result_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                        const asg_word_lookahead *la, int64_t B, int beam_size, int64_t max_frames,
                                        const void *state, size_t state_bytes, int final, void *scores, int64_t *path,
                                        int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                        int64_t *word_lengths, int64_t *frames, int64_t *status, int flags, void *stream);
size_t asg_beam_word_conf_stream_nbest_work_bytes(const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int dtype,
                                                  int beam_size, int64_t max_frames, int nbest);
int asg_beam_word_conf_stream_nbest(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B, int beam_size,
                                    int64_t max_frames, const void *state, size_t state_bytes, int final, int nbest, void *work,
                                    size_t work_bytes, void *scores, void *graph_scores, void *lm_scores, int64_t *path,
                                    int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                    int64_t *word_lengths, int64_t *num_hyps, int64_t *frames, int64_t *status, int flags,
                                    void *stream);
int asg_beam_word_conf_stream_nbest_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                       const asg_word_lookahead *la, int64_t B, int beam_size, int64_t max_frames, const void *state,
                                       size_t state_bytes, int final, int nbest, void *work, size_t work_bytes, void *scores,
                                       void *graph_scores, void *lm_scores, int64_t *path, int64_t *tokens, int64_t *token_lengths,
                                       int64_t *states, int64_t *lm_states, int64_t *words, int64_t *word_lengths,
                                       int64_t *num_hyps, int64_t *frames, int64_t *status, int flags, void *stream);
int asg_beam_word_conf_stream_confidence(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm, int64_t B,
                                         int beam_size, int64_t max_frames, void *state, size_t state_bytes, const void *transition,
                                         const int64_t *transition_strides, int final, int frame_tolerance, void *scores,
                                         int64_t *path, int64_t *tokens, int64_t *token_lengths, int64_t *states, int64_t *lm_states,
                                         int64_t *words, int64_t *word_lengths, int64_t *word_frames, void *word_confidences,
                                         void *normalisers, int64_t *frames, int64_t *status, int flags, void *stream);
int asg_beam_word_conf_stream_confidence_la(asg_ctx *ctx, const asg_token_graph_beam *gb, const asg_word_lm *lm,
                                            const asg_word_lookahead *la, int64_t B, int beam_size, int64_t max_frames, void *state,
                                            size_t state_bytes, const void *transition, const int64_t *transition_strides, int final,
                                            int frame_tolerance, void *scores, int64_t *path, int64_t *tokens,
                                            int64_t *token_lengths, int64_t *states, int64_t *lm_states, int64_t *words,
                                            int64_t *word_lengths, int64_t *word_frames, void *word_confidences, void *normalisers,
                                            int64_t *frames, int64_t *status, int flags, void *stream);

/* ---- whole-loss entry points (no counterpart in the reference's native layer: they fold the Python-side
 * `full - aligned` and reduction of asg.py:128,136-142 and their autograd into the kernels, so one ASGLoss
 * step is 2 + 2 kernel launches with no PyTorch glue kernels in between) ------------------------------------ */

#define ASG_REDUCTION_NONE 0
#define ASG_REDUCTION_SUM 1
#define ASG_REDUCTION_MEAN 2

/* loss = reduce_b(full[b] - aligned[b]); `loss` is [B] (none) or [1]; `scores` is a [2][B] work buffer that
 * receives full_scores then aligned_scores.
 * Alphabets of 257 .. 1024 labels (float32: .. 2048 while B <= 16) in every forward entry point: the full-lattice
 * recursions of all frames are ONE launch whose workgroups wait for each other frame by frame (the transition matrix
 * stays in their registers), sized to the device's compute units.  It therefore wants the device to itself: another
 * kernel that keeps compute units for seconds (a second process running the same route, say) can keep part of the
 * grid from starting.  A wait that runs out (~2^22 polls) ends the launch early and the repair kernel enqueued behind it by the
 * same call redoes the recursion without co-residency (asg_cluster_timeouts above): never a wrong number, never a NaN, never
 * a hang.  ASG_NO_CLUSTER=1 in the environment selects the launch-per-frame kernels from the start (2-3x slower,
 * no co-residency needed). */
int asg_loss_forward(asg_ctx *ctx, const asg_problem *p, void *state, size_t state_bytes, int reduction,
                     void *loss, void *scores, int flags, void *stream);

/* The evaluation route as ONE call: loss = reduce_b(full[b] - aligned[b]) from the beta recursions alone, nothing stored, no gradient
 * -- asg_forward_only (fast_asg_gpu_forward_only, streamlined_fast_gpu.cpp:24-94) with the `full - aligned` and the reduction of
 * asg.py:62-64,137-142 folded into the kernels, as asg_loss_forward does for the training route (small alphabets: the last beta
 * pass to finish reduces; large ones: one small reduction launch).  `scores`: asg_loss_forward_only_scores_bytes(p) bytes of work
 * space ([2][B] scores + 256 bytes for the arrival ticket).  `state` as for asg_forward_only (scratch of the large-alphabet path;
 * may be NULL when N <= 64 and S <= 64). */
size_t asg_loss_forward_only_scores_bytes(const asg_problem *p);
int asg_loss_forward_only(asg_ctx *ctx, const asg_problem *p, void *state, size_t state_bytes, int reduction,
                          void *loss, void *scores, size_t scores_bytes, int flags, void *stream);

/* gradients of the reduced loss: grad_loss is [B] (none) or [1]. */
int asg_loss_backward(asg_ctx *ctx, const asg_problem *p, const void *state, size_t state_bytes, int reduction,
                      const void *grad_loss, void *scratch, size_t scratch_bytes, void *grad_transition,
                      void *grad_inputs, int flags, void *stream);

/* ---- fused training step: the whole criterion, forward AND gradient assembly, in one launch -----------------
 * The reference's GPU fast route runs every recursion in forward and none in backward
 * (fast_asg_gpu_forward / fast_asg_gpu_backward, streamlined_fast_gpu.cpp:104-297); this pair goes one step further:
 * asg_loss_fused_forward also assembles, as the alpha and beta recursions cross, the full-lattice part of
 * d(loss)/d(inputs) and the per-utterance transition-gradient tiles (two per utterance: the frames each direction
 * reached second), and leaves the aligned posteriors beside them; asg_loss_fused_backward finishes the grad_inputs rows
 * (minus the aligned posteriors scattered to labels, times the actual upstream gradient), reduces the tiles in a fixed
 * order into grad_transition and redoes, exactly, any utterance the fused path declined (row sums outside the
 * fp32-safe range, fewer than 4 frames, a bounded wait on another workgroup that ran out).  Results are
 * bit-deterministic as long as no wait runs out, i.e. while the three workgroups of every utterance are co-resident
 * (an utterance redone by the exact code differs from the fused result in summation order, within the 1e-4 contract).
 * Only half of the lattice state ever goes to device memory.
 *   supported: float32, N < 64, S <= 64, T <= 4000 (asg_loss_fused_supported returns 1); otherwise use
 *              asg_loss_forward/backward.
 *   fast while: B <= 80 on 256 compute units -- the launch gives every utterance three compute units of its own and
 *              every XCD must hold three workgroups for each of its utterances; above that it still works (in rounds)
 *              but asg_loss_forward is faster, and the Python binding routes larger batches there.
 *   state:     asg_state_bytes(p) bytes, as for asg_loss_forward; the SAME buffer must be passed to backward.
 *   scratch:   asg_loss_fused_scratch_bytes(p) bytes; the SAME buffer must be passed to backward.
 *   grad_inputs [T,B,N] contiguous: partly written by forward, completed in place by backward.
 *   sync:      asg_loss_fused_sync_bytes(p) bytes of device memory that are ZERO on entry; the call leaves them
 *              zero.  They hold the words through which the workgroups of the launch talk to each other.  Calls that
 *              may run concurrently (different streams) need different regions; calls on one stream may share one.
 * The library allocates nothing and keeps no state between calls. */
int asg_loss_fused_supported(const asg_problem *p);
size_t asg_loss_fused_scratch_bytes(const asg_problem *p);
size_t asg_loss_fused_sync_bytes(const asg_problem *p);
int asg_loss_fused_forward(const asg_problem *p, void *state, size_t state_bytes, int reduction, void *loss, void *scores,
                           void *scratch, size_t scratch_bytes, void *grad_inputs, void *sync, int flags, void *stream);
int asg_loss_fused_backward(const asg_problem *p, void *state, size_t state_bytes, int reduction, const void *grad_loss,
                            void *scratch, size_t scratch_bytes, void *grad_inputs, void *grad_transition, int flags,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASG_HIP_H */
