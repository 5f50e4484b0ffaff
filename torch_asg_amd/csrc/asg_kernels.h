// torch_asg_amd/csrc/asg_kernels.h -- parameter blocks + launch prototypes shared by the
// kernel translation units and the C-ABI (asg_api.hip).  Internal; the public surface is
// include/asg_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace asg {

// One ASG problem instance as the caller handed it over (device pointers, element strides).
struct Problem {
    const void *inputs;          // [T,B,N] emissions, any strides
    int64_t is0, is1, is2;
    const void *transition;      // [N,N], transition[i][j] = score of j -> i
    int64_t ts0, ts1;
    const int64_t *targets;      // [B,S]
    int64_t gs0, gs1;
    const int64_t *in_len;       // [B] or nullptr (= T)
    const int64_t *tg_len;       // [B] or nullptr (= S)
    int T, B, N, S;
    int in_bf16;                 // emissions are bfloat16 (fused training step only); strides stay in elements
};

// Saved lattice state (forward -> backward), all in log2 units and RELATIVE per frame.
//   ah  [B][T][N]  full-lattice alpha-hat          bh  [B][T][N]  full-lattice beta-hat
//   ab  [B][T][S]  aligned alpha-bar               bb  [B][T][S]  aligned beta-bar
//   ehat [N][npad] row-normalised exp2 of the transition matrix (written once per forward by the alpha pass of
//                  utterance 0; npad = N rounded up to 8 on the small path, to 4 on the generic path), rmax [N]
//   fhat/cmax      column-normalised twin (generic path only)
//   asu [B][S][2]  per target position: {Tr2[O_s][O_s], Tr2[O_s][O_{s-1}]}  (log-zero where undefined)
//   asi [B][S][2]  int32 {O_s, O_{s-1}}
// ScaleLog (small path, klog [B][T][2]): what the full-lattice alpha pass folded into frame t's emission factor besides the
// emission and the row maximum -- entry t = {zb, ex}: the block scale and the power-of-two exponent, such that
//     sum_j ehat[i][j] * 2^ah[t-1][j]  =  2^( ah[t][i] - (fma(I[t][i], log2 e, rmax[i] - zb) - ex) )       (t >= 1)
// holds for the stored states with the chain's own rounding of the bracket.  The gradient pass recovers the row sums of the
// forward recursion from it (bwd_mfma_kernel) instead of recomputing them.  zb = NaN: the frame was produced by the exact
// per-node code and has no such relation.  Entry 0 = {kScaleLogMark, 0}, written by every alpha pass that stores states.
constexpr float kScaleLogMark = 1.0f;

struct State {
    void *ah, *bh, *ab, *bb;
    void *klog;
    void *ehat, *fhat, *rmax, *cmax;
    void *etile, *ftile;   // generic path, fp32: ehat / fhat again in the MFMA step kernel's operand order (asg_generic.hip)
    void *asu;
    int *asi;
    void *dbg;
    unsigned *ticket;   // 256 B, zeroed per call: arrival counter of the in-kernel loss reduction
    void *work;      // generic path: forward work buffers (emission maxima, p vectors, normalisers, offsets)
    int npad;
};

struct FwdOut {
    void *full_scores;           // [B]  from the beta pass (as the reference: fully_connected_lattice.cpp:89)
    void *aligned_scores;        // [B]  from the beta pass (force_aligned_lattice.cpp:316)
    void *full_scores_alpha;     // [B] or nullptr: same score from the alpha pass (cross-check)
    void *aligned_scores_alpha;  // [B] or nullptr
    // optional in-kernel loss reduction (small path): the LAST of the `expected` beta passes to finish reduces
    // loss[b] = full[b] - aligned[b] (reduction: 0 none, 1 sum, 2 mean) -- no separate reduce launch
    void *loss;
    unsigned *counter;           // State::ticket of this call (zeroed on the stream before the launch)
    int reduction, expected;
    int no_store;                // 1: scores only (eval / forward-only route): no lattice state is written.  A run-time
                                 // flag (stores are dropped by a zero-sized buffer resource), not a second set of kernels
};

struct BwdArgs {
    const void *grad_full;       // d(loss)/d(full_scores):    element b read at index b*gstride, times gscale
    const void *grad_aligned;    // d(loss)/d(aligned_scores); nullptr + neg_aligned: = -grad_full (ASG loss)
    int gstride;                 // 1 = per-utterance gradients, 0 = one scalar broadcast (reduced loss)
    int neg_aligned;
    double gscale;               // 1, or 1/B for reduction='mean' 
    void *grad_inputs;           // [T,B,N] contiguous
    void *grad_transition;       // [N,N] contiguous
    void *scratch;               // partial tiles etc.
    int chunk;                   // frames per workgroup (small path)
    int nchunks;
    int unit_grad;               // 1: the upstream gradient is 1 for every utterance (grad_full is not read)
};

// Fused training step of the whole criterion (asg_fused.hip): the forward launch also assembles the gradients for an
// upstream gradient of 1; the backward launch scales them (nothing to do when the upstream gradient IS 1), reduces
// the per-utterance transition-gradient tiles in a fixed order and redoes flagged utterances exactly.
struct FusedArgs {
    void *loss;                  // [B] (reduction none) or [1]
    void *scores;                // [2][B]: full, aligned
    void *grad_inputs;           // [T,B,N] contiguous
    void *tiles;                 // [B][2][N][N] per-utterance transition-gradient tiles (times gscale): alpha-side, beta-side frames
    int *flags;                  // [B]: 1 = the fused path declined this utterance (range guard, very short, time-out)
    void *dump;                  // [2][B] scratch scores for the exact redo
    void *p2;                    // [B][T][S] aligned posteriors, aligned workgroup -> full workgroup
    void *edges;                 // [B][2][3][2][64] double: aligned edge posteriors (stay | arrive) of the alpha-/beta-side frames, per finisher
    void *ascore;                // [B] double: aligned scores (log2 units)
    void *fscore;                // [B] double: full-lattice scores (log2 units), beta workgroup -> closing workgroup
    void *xstate;                // [B][2][xstate_blocks(T)][2][64][4] first-half states each full chain hands to the other
    void *rows;                  // [T,B,N] fp32: where the forward launch leaves its rows -- grad_inputs itself, or (bfloat16
                                 // emissions: grad_inputs is bfloat16) a work buffer
    void *in32;                  // bfloat16 emissions only: [B][T][N] fp32 copies of the emissions of FLAGGED utterances, made by
                                 // the forward launch for the exact stand-alone code (which reads fp32)
    void *aoff;                  // [B][2][T/16 + 2][2] double: per-block offsets of the stored aligned states
    unsigned *sync;              // caller-zeroed, returned zeroed: 64 words (word 0 = arrival ticket of the loss reduction)
                                 // + 16 words per utterance (UttSync in asg_fused.hip)
    unsigned *ticket2;           // 256 B, zeroed by the forward launch for the backward launch
    const void *grad_loss;       // backward: [B] (none) or [1]
    void *grad_transition;       // backward: [N,N]
    int reduction;
    float gscale;                // 1/B for reduction mean, else 1
};

enum ChainBits { kFullAlpha = 1, kFullBeta = 2, kAlignedAlpha = 4, kAlignedBeta = 8 };

// ---- small path: N <= 64, S <= 64, one wavefront per chain -------------------------------
// Developer / test switches, read from the environment once (asg_api.hip; asg_reload_env() reads them again).  -1 = not set.
struct Knobs {
    int fork_in_capture, pair_min_b, bwd_rowsum, no_cluster, no_mid, no_tile_step, step_one_tile, step_row_blocks, step_full_tile, step_no_bf3, step_bf3_min_b;
    char aligned_kernel;          // first letter of ASG_ALIGNED_KERNEL, or 0
};
const Knobs &knobs();

// chain_mask selects which of the four recursions this launch runs.
template <typename R>
hipError_t launch_fwd_small(const Problem &P, const State &W, const FwdOut &O, int chain_mask, bool store,
                            hipStream_t stream);
template <typename R>
hipError_t launch_bwd_small(const Problem &P, const State &W, const BwdArgs &A, int parts, hipStream_t stream);
hipError_t launch_fused_forward(const Problem &P, const State &W, const FusedArgs &F, hipStream_t stream);
hipError_t launch_fused_backward(const Problem &P, const State &W, const FusedArgs &F, hipStream_t stream);
// loss[b] = full[b] - aligned[b], reduced: 0 = none ([B] out), 1 = sum, 2 = mean ([1] out); fixed-order tree
template <typename R>
hipError_t launch_loss_reduce(const void *full, const void *aligned, int B, int reduction, void *out, hipStream_t stream);

// ---- generic path: any N (p-vector in LDS), S <= 1024 ----------------------------------
template <typename R>
hipError_t launch_prep_generic(const Problem &P, const State &W, hipStream_t stream);
template <typename R>
hipError_t launch_fwd_generic(const Problem &P, const State &W, const FwdOut &O, int chain_mask, bool store,
                              hipStream_t stream);
// parts: 1 = full lattice (N > 64), 2 = aligned lattice, 4 = grad buffers already hold the full-lattice part
template <typename R>
hipError_t launch_bwd_generic(const Problem &P, const State &W, const BwdArgs &A, int parts, hipStream_t stream);

// ---- best-path force alignment (S <= 64): work = [B][T] 64-bit back-pointer masks
template <typename R>
hipError_t launch_viterbi_small(const Problem &P, void *work, void *scores, void *path, hipStream_t stream);

// ---- Viterbi decoding over the full lattice (asg_decode.hip).  Resident route (one launch) while decode_resident(): work =
// [B][T][N] uint8 back-pointers; otherwise the streaming route: work = Tr^T [PAD][PAD] (256-byte aligned) + V [T][B][PAD],
// PAD = N rounded up to 64 (decode_work_bytes)
bool decode_resident(int elem, int N);
size_t decode_work_bytes(int elem, int T, int B, int N);
template <typename R>
hipError_t launch_decode(const Problem &P, void *work, void *scores, long long *path, long long *tokens, long long *tlen,
                         hipStream_t stream);

// ---- Viterbi decoding over the ASG lattice composed with a token automaton (asg_decode_graph.hip).  The compiled product
// graph as the kernels read it (asg_token_graph; every array on the device, Q, E < 2^31).  Work = int32 back-pointers
// [B][T][Q] (resident route) or [T][Q][B] (streaming route), 256-byte aligned, then the streaming route's Viterbi vectors
// [2][Q][B]: the same size on both routes (graph_decode_work_bytes).
struct GraphArgs {
    int Q, E;
    const int *label, *state, *row, *src, *src_label;     // [Q], [Q], [Q+1], [E], [E]
    const void *start_w, *final_w, *edge_w;               // [Q], [Q], [E] in the dtype of the problem
};
// route: 0 = by graph_decode_resident, 1 = streaming, 2 = resident wherever the graph fits in LDS
bool graph_decode_resident(int elem, int N, int Q, int E);
size_t graph_decode_work_bytes(int elem, int T, int B, int Q);
template <typename R>
hipError_t launch_decode_graph(const Problem &P, const GraphArgs &G, int route, void *work, void *scores, long long *path,
                               long long *tokens, long long *tlen, long long *states, hipStream_t stream);

// ---- Beam-pruned Viterbi decoding over the same composed lattice (asg_beam_graph.hip).  The source-side arrays of
// asg_token_graph_beam.  K = beam_graph_k(Q, beam_size) slots; the touched list holds beam_graph_cap(..) targets.  Work, per
// utterance and each part 256-byte aligned: int32 [T][K] product states, int32 [T][K] source slots, u64 arg [Q], key val [Q],
// key [cap], int32 touched [cap] (key = 4 or 8 bytes).
struct BeamGraphArgs {
    int num_start, max_out;
    const int *orow;             // [Q+1]
    const void *oarc;            // [E] int32 pairs {target, label of the target}
    const void *ow;              // [E] folded arc weights in the dtype of the problem
    const int *start_q;          // [num_start]
};
constexpr int kBeamMaxK = 8192;  // the active set (value, q) stays in LDS
int beam_graph_k(int Q, int beam_size);
int beam_graph_cap(int Q, int K, int max_out, int num_start);
size_t beam_graph_work_bytes(int elem, int T, int B, int Q, int K, int cap);
// stride != 0: the utterances' workspaces lie `stride` bytes apart (each with the layout above at its front); cnt_off != 0: the
// kernel also writes |A_t| of every frame, int32 [T], at that offset of each of them (asg_beam_loss.hip); fin_off != 0: it also
// leaves |A_{len-1}| (int32) at that offset and that set's values, slot-aligned with its [K] product states, from byte 8 behind
// it (asg_beam_nbest.hip).  0, 0, 0: the decoder.
template <typename R>
hipError_t launch_beam_graph(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta, void *work,
                             void *scores, long long *path, long long *tokens, long long *tlen, long long *states,
                             hipStream_t stream, size_t stride = 0, size_t cnt_off = 0, size_t fin_off = 0);

// ---- Beam decoding with a lexicon and a word LM composed on the fly (asg_beam_word.hip): asg_beam_decode_words.  The search
// state is a pair (LM state h, product state q of the lexicon automaton).  K = beam_size (no clamp to Q); the touched list holds
// cap = beam_word_cap(..) target pairs; the table has C slots, the power of two >= 2 * cap.  Work, per utterance and each part
// 256-byte aligned: int32 [T][K] product states, LM states and source slots, u64 key [C], u64 arg [C], key val [C], key [cap],
// u64 pair [cap], int32 touched [cap].
struct WordLmArgs {
    int H, A, start, sep;
    const int *row, *word, *next, *backoff;   // [H+1], [A], [A], [H]
    const int *word_of_state;                 // [S] of the lexicon automaton
    const void *lw, *bw, *ew;                 // [A], [H], [H] folded, in the dtype of the problem
};
constexpr int kBeamWordMaxIndex = 1 << 25;    // H, Q: (source pair, source slot) is one 64-bit word
int beam_word_cap(int K, int max_out, int num_start);
size_t beam_word_work_bytes(int elem, int T, int B, int K, int cap);
// stride != 0: the utterances' workspaces lie `stride` bytes apart (each with the layout above at its front); fin_off != 0: the
// kernel also leaves |A_{len-1}| (int32) at that offset of each and, from byte 8 behind it, that set's values [K], then its int32
// product states [K], then its int32 LM states [K] (asg_beam_word_nbest.hip).  0, 0: the decoder.
template <typename R>
hipError_t launch_beam_words(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, int K,
                             double theta, void *work, void *scores, long long *path, long long *tokens, long long *tlen,
                             long long *states, long long *lm_states, long long *words, long long *wlen, hipStream_t stream,
                             size_t stride = 0, size_t fin_off = 0);

// ---- The same search carried across chunks of frames (asg_beam_stream.hip): asg_beam_stream_*.  One slot of the state (byte
// offsets, each part 256-byte aligned): the beam search's own layout for T = max_frames at the front, then hdr (int32 pos, |A|,
// overflow, apos -- the last is the lattice-keeping state's, asg_beam_stream_lat.h) and the stored set (values [K], then int32
// product states [K]).
struct BeamStreamLayout {
    size_t hdr, set, per;
};
BeamStreamLayout beam_stream_layout(int elem, int max_frames, int Q, int K, int cap);
size_t beam_stream_state_bytes(int elem, int max_frames, int B, int Q, int K, int cap);
// mask: one byte per slot (null: every slot); stride as launch_beam_stream_result's
hipError_t launch_beam_stream_reset(int elem, const GraphArgs &G, const BeamGraphArgs &BG, int K, int max_frames, int B, void *state,
                                    const unsigned char *mask, hipStream_t stream, size_t stride = 0);
// P.T frames of P.inputs per slot at the most (P.in_len: the chunk's lengths).  lattice: the state is a lattice-keeping one
// (beam_conf_stream_layout below) -- the same kernel with the policy that also keeps cnt and the emissions (asg_beam_stream_lat.h).
template <typename R>
hipError_t launch_beam_stream_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta,
                                      int max_frames, void *state, hipStream_t stream, bool lattice = false);
template <typename R>
hipError_t launch_beam_stream_result(const GraphArgs &G, const BeamGraphArgs &BG, int K, int max_frames, int B, const void *state,
                                     int final, void *scores, long long *path, long long *tokens, long long *tlen,
                                     long long *states, long long *frames, long long *status, hipStream_t stream,
                                     size_t stride = 0);      // != 0: the slots lie `stride` bytes apart (asg_beam_stream_conf.hip)

// ---- The same search with LM look-ahead (asg_beam_word_la.hip): asg_beam_decode_words_la.  K, cap, the table and the workspace
// are those of launch_beam_words, stride and fin_off too; the look-ahead adds read-only arrays and nothing per utterance.
struct WordLookArgs {
    int A, levels;                            // ranked arcs A', levels of the range-maximum table
    const int *rlo, *rhi;                     // [S] rank range of the words below each trie node
    const int *la_state;                      // [H] the (truncated) history whose rows the look-ahead of h reads
    const int *krow, *krank;                  // [H+1], [A'] ranked arcs of each LM state, rank ascending
    const void *tab;                          // [levels][A'] in the dtype of the problem
    const void *dense0;                       // [S] E(0, n): the range maximum of state 0 for every node
};
template <typename R>
hipError_t launch_beam_words_la(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                const WordLookArgs &LA, int K, double theta, void *work, void *scores, long long *path,
                                long long *tokens, long long *tlen, long long *states, long long *lm_states, long long *words,
                                long long *wlen, hipStream_t stream, size_t stride = 0, size_t fin_off = 0);

// ---- The search over pairs carried across chunks of frames (asg_beam_word_stream.hip): asg_beam_word_stream_*.  One slot of the
// state: the word decoder's own layout for T = max_frames at the front, then hdr (int32 pos, |A|, overflow) and the stored set
// (values [K], then int32 product states [K], then int32 LM states [K]).  K = beam_size, cap = beam_word_cap(..).  LA: the
// look-ahead of asg_beam_word_stream_*_la, nullptr without one (the state, its size and its reset do not depend on it).
BeamStreamLayout beam_word_stream_layout(int elem, int max_frames, int K, int cap);
size_t beam_word_stream_state_bytes(int elem, int max_frames, int B, int K, int cap);
// stride / lattice: as launch_beam_stream_reset's and launch_beam_stream_advance's (beam_word_conf_stream_layout below)
hipError_t launch_beam_word_stream_reset(int elem, const BeamGraphArgs &BG, int K, int max_frames, int B, void *state,
                                         const unsigned char *mask, hipStream_t stream, size_t stride = 0);
template <typename R>
hipError_t launch_beam_word_stream_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                           const WordLookArgs *LA, int K, double theta, int max_frames, void *state,
                                           hipStream_t stream, bool lattice = false);
template <typename R>
hipError_t launch_beam_word_stream_result(const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                          const WordLookArgs *LA, int K, int max_frames, int B, const void *state, int final,
                                          void *scores, long long *path, long long *tokens,
                                          long long *tlen, long long *states, long long *lm_states, long long *words,
                                          long long *wlen, long long *frames, long long *status, hipStream_t stream,
                                          size_t stride = 0);   // != 0: the slots lie `stride` bytes apart (asg_beam_word_stream_conf.hip)

// ---- The n best hypotheses of the search over pairs, with the score split three ways (asg_beam_word_nbest.hip):
// asg_beam_decode_words_nbest and asg_beam_word_stream_nbest.  One-shot, one utterance's workspace: the word decoder's own layout
// at the front, then (byte offsets, each part 256-byte aligned) fin (int32 |A_{len-1}|, then from byte 8 its values [K], product
// states [K], LM states [K]) and rows (int32 [T][nb] product states of every hypothesis, frame-major), nb = min(nbest, K).  Behind
// the utterances: what the one-best search returns (scores, two lengths, five [B][T] arrays).  The stream's scratch is the rows
// alone, [B][max_frames][nb].
struct BeamWordNbestLayout {
    size_t fin, rows, per;
    int nb;
};
BeamWordNbestLayout beam_word_nbest_layout(int elem, int T, int K, int cap, int nbest);
size_t beam_word_nbest_work_bytes(int elem, int T, int B, int K, int cap, int nbest);
size_t beam_word_stream_nbest_work_bytes(int max_frames, int B, int K, int nbest);
// Where a search left its results for the n-best kernel.  Slot b's block starts at base + b * per: the [Tw][K] rows bq / bh / bs
// at its front; the set (values [K], product states [K], LM states [K]) at set_off; int32 |A| at na_off; the length from the
// problem's lengths (pos_off == 0) or the int32 at pos_off; with ovf_off, the stream's overflow word.  A window state
// (kBeamWordNbestWindow) has its header -- int64 pos, int64 base, int32 |A|, carry, carry_state, status -- at pos_off instead, its
// rows are rings (Tw = W, frame u in row u mod W), and S is the number of automaton states word_of_state is indexed by.
struct BeamWordNbestSrc {
    const char *base;
    size_t per, set_off, na_off, pos_off, ovf_off;
    char *cols;                    // slot b's [Tw][nb] column block at cols + b * cols_per
    size_t cols_per;
    int Tw, nb;
    int S;
};
// The kernel's compile-time source.  kBeamWordNbestRows: rows from frame 0 on -- the one-shot workspace and the stream state, which
// one instantiation has always told apart by pos_off.  kBeamWordNbestWindow: the ring of a window state.
enum { kBeamWordNbestRows = 0, kBeamWordNbestWindow = 1 };
// the n-best kernel alone, one-shot, over what a search left at `src` (LA: that search's look-ahead, or NULL)
template <typename R>
hipError_t launch_beam_word_nbest_over(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                       const WordLookArgs *LA, const BeamWordNbestSrc &src, int K, int nbest, void *scores,
                                       void *emission_scores, void *graph_scores, void *lm_scores, long long *path,
                                       long long *tokens, long long *tlen, long long *states, long long *lm_states,
                                       long long *words, long long *wlen, long long *num_hyps, hipStream_t stream);
// path / states / lm_states may be null (then they are not written)
template <typename R>
hipError_t launch_beam_words_nbest(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, int K,
                                   double theta, int nbest, void *work, void *scores, void *emission_scores, void *graph_scores,
                                   void *lm_scores, long long *path, long long *tokens, long long *tlen, long long *states,
                                   long long *lm_states, long long *words, long long *wlen, long long *num_hyps,
                                   hipStream_t stream);
// ... behind the search with LM look-ahead (launch_beam_words_la): asg_beam_decode_words_nbest_la.  Same workspace.
template <typename R>
hipError_t launch_beam_words_nbest_la(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                      const WordLookArgs &LA, int K, double theta, int nbest, void *work, void *scores,
                                      void *emission_scores, void *graph_scores, void *lm_scores, long long *path,
                                      long long *tokens, long long *tlen, long long *states, long long *lm_states,
                                      long long *words, long long *wlen, long long *num_hyps, hipStream_t stream);
// The same kernel over a stream state (read only).  The state holds no emissions: there is no emission sum.
template <typename R>
hipError_t launch_beam_word_stream_nbest(const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, int K, int max_frames,
                                         int B, const void *state, int final, int nbest, void *work, void *scores,
                                         void *graph_scores, void *lm_scores, long long *path, long long *tokens, long long *tlen,
                                         long long *states, long long *lm_states, long long *words, long long *wlen,
                                         long long *num_hyps, long long *frames, long long *status, hipStream_t stream,
                                         size_t stride = 0);    // as launch_beam_word_stream_result's
// ... over a state that launch_beam_word_stream_advance left with the look-ahead LA: asg_beam_word_stream_nbest_la.
template <typename R>
hipError_t launch_beam_word_stream_nbest_la(const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                            const WordLookArgs &LA, int K, int max_frames, int B, const void *state, int final,
                                            int nbest, void *work, void *scores, void *graph_scores, void *lm_scores,
                                            long long *path, long long *tokens, long long *tlen, long long *states,
                                            long long *lm_states, long long *words, long long *wlen, long long *num_hyps,
                                            long long *frames, long long *status, hipStream_t stream, size_t stride = 0);

// ---- The stream in bounded memory (asg_beam_window.hip): asg_beam_window_*.  One slot of the state has the layout of a stream
// of W frames -- the back-pointers are a ring, frame u in row u mod W -- with the header int64 pos, int64 base, int32 |A|, carry,
// status.  CP: the commit period (a commit attempt after every frame whose count is a multiple of it), 1 <= CP <= W.
BeamStreamLayout beam_window_layout(int elem, int W, int Q, int K, int cap);
size_t beam_window_state_bytes(int elem, int W, int B, int Q, int K, int cap);
// (stride, here and below: as launch_beam_stream_result's -- a lattice-keeping state's slots, asg_beam_conf_window.hip)
hipError_t launch_beam_window_reset(int elem, const GraphArgs &G, const BeamGraphArgs &BG, int K, int W, int B, void *state,
                                    const unsigned char *mask, hipStream_t stream, size_t stride = 0);
// new_path / new_states / new_tokens [B][W + P.T], new_frames / new_tlen [B]: every element is written.  cw: the state is a
// lattice-keeping one (beam_conf_window_layout below) -- the same kernel with the policy that also keeps the ring's cnt, emissions
// and unsorted sets, writes new_token_frames [B][W + P.T] and logs the attempts that committed (asg_beam_window_lat.h).
struct BeamConfWindowLayout;
template <typename R>
hipError_t launch_beam_window_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta, int W,
                                      int CP, void *state, long long *new_path, long long *new_states, long long *new_tokens,
                                      long long *new_frames, long long *new_tlen, hipStream_t stream,
                                      const BeamConfWindowLayout *cw = nullptr, long long *new_token_frames = nullptr);
template <typename R>
hipError_t launch_beam_window_result(const GraphArgs &G, const BeamGraphArgs &BG, int K, int W, int B, const void *state, int final,
                                     void *scores, long long *path, long long *tokens, long long *tlen, long long *states,
                                     long long *frames, long long *committed, long long *status, hipStream_t stream,
                                     size_t stride = 0);

// ---- The search over pairs in bounded memory (asg_beam_word_window.hip): asg_beam_word_window_*.  One slot of the state has the
// layout of a word stream of W frames -- bq / bh / bs are rings, frame u in row u mod W -- with the header int64 pos, int64 base,
// int32 |A|, carry, carry_state, status.  K = beam_size, cap = beam_word_cap(..), CP the commit period, S the number of states of
// the lexicon automaton (word_of_state has S entries).  LA: the look-ahead of asg_beam_word_window_*_la, nullptr without one.
BeamStreamLayout beam_word_window_layout(int elem, int W, int K, int cap);
size_t beam_word_window_state_bytes(int elem, int W, int B, int K, int cap);
hipError_t launch_beam_word_window_reset(int elem, const BeamGraphArgs &BG, int K, int W, int B, void *state,
                                         const unsigned char *mask, hipStream_t stream);
// new_path / new_states / new_lm_states / new_tokens / new_words [B][W + P.T], new_frames / new_tlen / new_wlen [B]: every element
// is written
template <typename R>
hipError_t launch_beam_word_window_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                           const WordLookArgs *LA, int S, int K, double theta, int W, int CP, void *state,
                                           long long *new_path,
                                           long long *new_states, long long *new_lm_states, long long *new_tokens,
                                           long long *new_words, long long *new_frames, long long *new_tlen, long long *new_wlen,
                                           hipStream_t stream);
template <typename R>
hipError_t launch_beam_word_window_result(const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                          const WordLookArgs *LA, int S, int K, int W, int B, const void *state, int final,
                                          void *scores, long long *path, long long *tokens,
                                          long long *tlen, long long *states, long long *lm_states, long long *words,
                                          long long *wlen, long long *frames, long long *committed, long long *status,
                                          hipStream_t stream);
// The n-best kernel of asg_beam_word_nbest.hip over a window state (read only): asg_beam_word_window_nbest, with LA
// asg_beam_word_window_nbest_la.  Every row is the uncommitted tail of its chain, [B][nbest][W]; no sums.  work: [B] blocks of
// a256(W * nb * 4) bytes.  path / states / lm_states may be null.
size_t beam_word_window_nbest_work_bytes(int W, int B, int K, int nbest);
template <typename R>
hipError_t launch_beam_word_window_nbest(const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                         const WordLookArgs *LA, int S, int K, int W, int B, const void *state, int final,
                                         int nbest, void *work, void *scores, long long *path, long long *tokens, long long *tlen,
                                         long long *states, long long *lm_states, long long *words, long long *wlen,
                                         long long *num_hyps, long long *frames, long long *committed, long long *status,
                                         hipStream_t stream);

// ---- The n best final hypotheses of that search, with the score split (asg_beam_nbest.hip): asg_beam_decode_graph_nbest.
// One utterance's workspace: the beam search's own layout at the front, then (byte offsets, each part 256-byte aligned) fin
// (int32 |A_{len-1}|, then from byte 8 its values [K]) and rows (int32 [T][nb] product states of every hypothesis, frame-major),
// nb = min(nbest, K).  Behind the utterances: what the search itself returns (beam_loss_tail_bytes' layout).
struct BeamNbestLayout {
    size_t fin, rows, per;
    int nb;
};
constexpr int kBeamMaxNbest = 8192;
BeamNbestLayout beam_nbest_layout(int elem, int T, int Q, int K, int cap, int nbest);
size_t beam_nbest_work_bytes(int elem, int T, int B, int Q, int K, int cap, int nbest);
// path / states may be null (then they are not written)
template <typename R>
hipError_t launch_beam_nbest(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta, int nbest,
                             void *work, void *scores, void *emission_scores, void *graph_scores, long long *path,
                             long long *tokens, long long *tlen, long long *states, long long *num_hyps, hipStream_t stream);
// the n-best kernel alone over what a search left in blocks of `lay` (any `lay.per`, with the search's own layout at the front
// of a block, its last set at lay.fin and room for the [T][nb] rows at lay.rows): behind the decoder's search in
// launch_beam_nbest, behind the lattice's search in asg_beam_nbest_conf.hip
template <typename R>
hipError_t launch_beam_nbest_over(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const BeamNbestLayout &lay, int K,
                                  int nbest, void *work, void *scores, void *emission_scores, void *graph_scores, long long *path,
                                  long long *tokens, long long *tlen, long long *states, long long *num_hyps, hipStream_t stream);
// Where a search of this family lives for the n-best kernel (its three instantiations per dtype: kBeamNbestShot, kBeamNbestStream,
// kBeamNbestWindow).  Slot b's block starts at base + b * per, with the [Tw][K] rows bq / bs at its front (beam_work_layout for
// T = Tw); its int32 [Tw][nb] column block at cols + b * cols_per.
//   one-shot   fin: int32 |A_{len-1}|, from byte 8 that set's values [K]; its states are row len-1 of bq; the length comes from
//              the problem's lengths.
//   stream     hdr: int32 pos, |A|, overflow; set: values [K], then int32 product states [K].  Tw = max_frames.
//   window     hdr: int64 pos, int64 base, int32 |A|, carry, status; set as the stream's.  Tw = W, and the rows are a ring:
//              frame u in row u mod W.
struct BeamNbestSrc {
    const char *base;
    size_t per, fin, hdr, set;
    char *cols;
    size_t cols_per;
    int Tw, nb;
};
enum { kBeamNbestShot = 0, kBeamNbestStream = 1, kBeamNbestWindow = 2 };
// The same kernel over a stream state / a window state (read only).  The state holds no emissions: there is no emission sum,
// and for the window no graph sum either.  work: [B] blocks of a256(rows * nb * 4) bytes, rows = max_frames / W.
size_t beam_stream_nbest_work_bytes(int rows, int B, int K, int nbest);
template <typename R>
hipError_t launch_beam_stream_nbest(const GraphArgs &G, const BeamGraphArgs &BG, int K, int max_frames, int B, const void *state,
                                    int final, int nbest, void *work, void *scores, void *graph_scores, long long *path,
                                    long long *tokens, long long *tlen, long long *states, long long *num_hyps, long long *frames,
                                    long long *status, hipStream_t stream, size_t stride = 0);   // as launch_beam_stream_result's
template <typename R>
hipError_t launch_beam_window_nbest(const GraphArgs &G, const BeamGraphArgs &BG, int K, int W, int B, const void *state, int final,
                                    int nbest, void *work, void *scores, long long *path, long long *tokens, long long *tlen,
                                    long long *states, long long *num_hyps, long long *frames, long long *committed,
                                    long long *status, hipStream_t stream, size_t stride = 0);   // as launch_beam_stream_result's

// ---- Beam-pruned full score and gradients over the same composed lattice (asg_beam_loss.hip): asg_beam_graph_full_*.
struct BeamLossArgs {
    int S, start;
    const int *next;             // [S*N] next automaton state, -1 where no arc
};
// One utterance's workspace: the beam search's own layout at the front, then (byte offsets, each part 256-byte aligned) the
// kept counts cnt [T], the lattice counts nu [T], hdr (word 0: forced states n), the target walk's keys [nf] int64 and forced
// product states qk [nf], the lattice lists U [T][M], alpha [T or 2][M]; M = K + nf, nf = min(S, T) with targets, else 0.
struct BeamLossLayout {
    size_t cnt, nu, hdr, key, qk, U, A, per;
    int M, nf;
};
constexpr int kBeamLossMaxN = 1024;        // a frame's label posteriors are summed in LDS
constexpr int kBeamLossMaxForced = 2048;   // min(S, T): U_{t-1} with its values stays in LDS
BeamLossLayout beam_loss_layout(int elem, int T, int Q, int K, int cap, int nf, bool store);
size_t beam_loss_work_bytes(int elem, int T, int B, int Q, int K, int cap, int nf, bool store);
size_t beam_loss_scratch_per(int elem, int M, int N);
bool beam_loss_fits(int elem, int M, int N);
// behind the utterances: what the search returns besides its sets (scores [B], lengths [B], path / tokens / states [3][B][T])
size_t beam_loss_tail_bytes(int T, int B);
template <typename R>
hipError_t launch_beam_loss_forward(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const BeamLossArgs &L, int K,
                                    double theta, bool store, void *work, void *scores, hipStream_t stream);
template <typename R>
hipError_t launch_beam_loss_backward(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, const void *work,
                                     const void *scores, const void *grad_scores, void *grad_inputs, void *grad_transition,
                                     void *scratch, bool accumulate, hipStream_t stream);

// launches 1 - 4 of that forward behind a layout the caller made (`lay.per` may be wider than beam_loss_layout's: a caller with
// parts of its own behind an utterance's block), the search writing its five outputs where the caller says; fin_off is
// launch_beam_graph's (0: the last set is not left)
template <typename R>
hipError_t launch_beam_loss_lattice(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const BeamLossArgs &L,
                                    const BeamLossLayout &lay, int K, double theta, bool store, void *work, void *scores,
                                    void *beam_scores, long long *path, long long *tokens, long long *tlen, long long *states,
                                    size_t fin_off, hipStream_t stream);

// ---- Token confidences and start frames from the lattice of that search (asg_beam_conf.hip): asg_beam_graph_confidence.  One
// utterance's workspace: the beam-pruned loss's layout without targets with alpha stored for all frames (M = K), then two rows
// of beta [2][M] that the pull hands from one frame to the next.  The accumulators of the hypothesis' tokens live in LDS.
constexpr int kBeamConfMaxTol = 64;        // a ring of 256 accumulators holds every token whose window is open
struct BeamConfLayout {
    BeamLossLayout lat;          // lat.per is this layout's `per`
    size_t beta, per;
};
BeamConfLayout beam_conf_layout(int elem, int T, int Q, int K, int cap);
size_t beam_conf_work_bytes(int elem, int T, int B, int Q, int K, int cap);
template <typename R>
hipError_t launch_beam_conf(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const BeamLossArgs &L, int K, double theta,
                            int tol, void *work, void *scores, long long *path, long long *tokens, long long *tlen,
                            long long *states, long long *token_frames, void *token_conf, void *normalisers, hipStream_t stream);

// ---- The streaming search with a state that keeps its lattice (asg_beam_stream_conf.hip): asg_beam_conf_stream_*.  One slot: the
// plain stream's slot (beam_stream_layout) unchanged at the front, then (byte offsets, each part 256-byte aligned) cnt int32
// [max_frames], the emissions [max_frames][N], nu int32 [max_frames], U int32 [max_frames][K], A [max_frames][K], beta [2][K].
// Header word 3 is apos, the frames whose U / nu / A rows are valid.  `lat` is a BeamLossLayout (M = K, nf = 0) over those parts,
// so TokenLat<R>::Args and beam_conf_pull take it as they take BeamConfLayout's; st.per, lat.per and per are the slot's stride.
struct BeamConfStreamLayout {
    BeamStreamLayout st;
    BeamLossLayout lat;
    size_t em, beta, per;
};
BeamConfStreamLayout beam_conf_stream_layout(int elem, int max_frames, int Q, int K, int cap, int N);
size_t beam_conf_stream_state_bytes(int elem, int max_frames, int B, int Q, int K, int cap, int N);
// (reset, advance, result and n-best are the plain stream's launchers with this layout's stride / lattice = true)
// P: B, N and the transition (its emissions and lengths are not read: the state has both).  Two launches: the catch-up of U / nu /
// A from apos to pos (the only write to the state from a result path), then the hypothesis, Z and the beta pull.
template <typename R>
hipError_t launch_beam_conf_stream_confidence(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, int max_frames,
                                              void *state, int final, int tol, void *scores, long long *path, long long *tokens,
                                              long long *tlen, long long *states, long long *token_frames, void *token_conf,
                                              void *normalisers, long long *frames, long long *status, hipStream_t stream);

// ---- The window stream with a state that keeps its lattice in a ring (asg_beam_conf_window.hip): asg_beam_conf_window_*.  One
// slot: the plain window's slot (beam_window_layout) unchanged at the front -- its header block also holds apos and the number of
// logged attempts (asg_beam_window_lat.h) --, then (byte offsets, each part 256-byte aligned) a ring of RW = W + tol + 1 + C rows,
// frame t in row t mod RW: cnt int32 [RW], the emissions [RW][N], nu int32 [RW], U int32 [RW][K], A [RW][K]; the attempt log of
// nlog = C / CP + 1 entries; beta [nlog][2][K], a pair of rows per logged attempt.  C: the longest chunk an advance may bring.
constexpr int kBeamConfWindowMaxLog = 65535;   // C / CP + 1: the pull's grid is (B, log entries)
struct BeamConfWindowLayout {
    BeamStreamLayout st;
    BeamLossLayout lat;          // cnt, nu, U, A over the ring (M = K, nf = 0); lat.per is the slot's stride
    size_t em, log, beta, per;
    int RW, nlog;
};
BeamConfWindowLayout beam_conf_window_layout(int elem, int W, int CP, int tol, int C, int Q, int K, int cap, int N);
size_t beam_conf_window_state_bytes(int elem, int W, int CP, int tol, int C, int B, int Q, int K, int cap, int N);
// Three launches: the search (launch_beam_window_advance with cw), the catch-up of U / nu / A over [apos, pos), the pull of every
// logged attempt.  new_token_frames / new_token_conf [B][W + P.T]: every element is written.
template <typename R>
hipError_t launch_beam_conf_window_advance(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, double theta, int W,
                                           int CP, int tol, int C, void *state, long long *new_path, long long *new_states,
                                           long long *new_tokens, long long *new_frames, long long *new_tlen,
                                           long long *new_token_frames, void *new_token_conf, hipStream_t stream);
// Two launches: the plain result kernel, then token_frames / token_conf [B][W] and normalisers [B] by one pull from pos - 1 down
// to base - tol.  P: B, N and the transition.  It only reads the state (beta rows apart).
template <typename R>
hipError_t launch_beam_conf_window_confidence(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, int K, int W, int CP,
                                              int tol, int C, void *state, int final, void *scores, long long *path,
                                              long long *tokens, long long *tlen, long long *states, long long *token_frames,
                                              void *token_conf, void *normalisers, long long *frames, long long *committed,
                                              long long *status, hipStream_t stream);

// ---- Token confidences and start frames for every row of the n-best list (asg_beam_nbest_conf.hip):
// asg_beam_graph_nbest_confidence.  One utterance's workspace: asg_beam_graph_confidence's layout at the front (the search's
// [T][K] rows first), then (byte offsets, each part 256-byte aligned) fin and rows as in BeamNbestLayout, hdr (int32 number of
// cells), foff (int32 [T + 2]: the first cell of every frame), qk (u64 [P2(nb * T)]: the rows' (frame, label) queries, sorted
// there when they pass the LDS), cells (u64 [nb * T]: the distinct queries, ascending) and acc (u64 [nb * T]: a cell's fixed-point
// sum).  Behind the utterances: what the one-best search returns (beam_loss_tail_bytes).
struct BeamNbestConfLayout {
    BeamConfLayout conf;         // conf.lat.per and conf.per are this layout's `per`
    BeamNbestLayout nbest;       // fin, rows, nb; nbest.per is this layout's `per`
    size_t hdr, foff, qk, cells, acc, per;
    size_t qcap;                 // P2(nb * T)
    int nb;
};
// THE new limit: bwd_front + ring (u64) + mirror (int32) + window offsets and filter (1024 bytes) within 160 KiB of LDS, the
// ring beam_word_nbest_conf_ring's (the power of two >= min(nbest, K) * (2 tol + 2)), and nb * T <= 2^30.
bool beam_nbest_conf_fits(int elem, int T, int K, int nbest, int tol);
BeamNbestConfLayout beam_nbest_conf_layout(int elem, int T, int Q, int K, int cap, int nbest);
size_t beam_nbest_conf_work_bytes(int elem, int T, int B, int Q, int K, int cap, int nbest);
// path / states may be null (then they are not written)
template <typename R>
hipError_t launch_beam_nbest_conf(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const BeamLossArgs &L, int K,
                                  double theta, int nbest, int tol, void *work, void *scores, void *emission_scores,
                                  void *graph_scores, long long *path, long long *tokens, long long *tlen, long long *states,
                                  long long *num_hyps, long long *token_frames, void *token_conf, void *normalisers,
                                  hipStream_t stream);

// ---- Beam-pruned full score and gradients over the pairs of the word decoder (asg_beam_word_loss.hip): asg_beam_words_full_*.
// One utterance's workspace: the word decoder's own layout at the front (bq, bh: its [T][K] lists), then (byte offsets, each part
// 256-byte aligned) the kept counts cnt [T], the lattice counts nu [T], hdr (word 0: forced pairs n), the forced pairs' keys
// [nf] u64, the lattice lists U [T][M] u64, alpha [T or 2][M]; M = K + nf, nf = min(S, T) with targets, else 0.
struct BeamWordLossLayout {
    size_t bq, bh, cnt, nu, hdr, key, U, A, per;
    int M, nf;
};
BeamWordLossLayout beam_word_loss_layout(int elem, int T, int K, int cap, int nf, bool store);
size_t beam_word_loss_work_bytes(int elem, int T, int B, int K, int cap, int nf, bool store);
inline size_t beam_word_loss_scratch_per(int elem, int M, int N) { return beam_loss_scratch_per(elem, M, N); }   // the same pass
// the one bound on M: a frame's lattice set with a maximum and a sum per member stays in LDS (M <= 8179 float32, 6816 float64)
bool beam_word_loss_fits(int elem, int M, int N);
// LA: the look-ahead the search takes its sets with (asg_beam_words_full_forward_la), or NULL; nothing else of the pass reads it.
template <typename R>
hipError_t launch_beam_word_loss_forward(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                         const WordLookArgs *LA, int K, double theta, bool store, void *work, void *scores,
                                         hipStream_t stream);
// launches 2 - 4 of that forward alone (target walk, sets, alpha and Z_K) behind a search that left bq / bh / cnt in `lay`
template <typename R>
hipError_t launch_beam_word_loss_lattice(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                         const BeamWordLossLayout &lay, int K, bool store, void *work, void *scores,
                                         hipStream_t stream);
template <typename R>
hipError_t launch_beam_word_loss_backward(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM, int K,
                                          const void *work, const void *scores, const void *grad_scores, void *grad_inputs,
                                          void *grad_transition, void *scratch, bool accumulate, hipStream_t stream);
template <typename R>
hipError_t launch_beam_word_target_scores(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                          void *out, hipStream_t stream);

// ---- Word confidences and end frames from the lattice of the word decoder (asg_beam_word_conf.hip):
// asg_beam_words_confidence.  One utterance's workspace: the pair loss's layout without targets with alpha stored for all frames
// (M = K), then two rows of beta [2][M] that the pull hands from one frame to the next.  The accumulators of the hypothesis'
// words live in LDS.  LA: the look-ahead of the search, or NULL; nothing behind the search reads it.
constexpr int kBeamWordConfMaxTol = 64;     // a ring of 256 accumulators holds every word whose window is open
struct BeamWordConfLayout {
    BeamWordLossLayout lat;      // lat.per is this layout's `per`
    size_t beta, per;
};
BeamWordConfLayout beam_word_conf_layout(int elem, int T, int K, int cap);
size_t beam_word_conf_work_bytes(int elem, int T, int B, int K, int cap);
template <typename R>
hipError_t launch_beam_word_conf(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                 const WordLookArgs *LA, int K, double theta, int tol, void *work, void *scores, long long *path,
                                 long long *tokens, long long *tlen, long long *states, long long *lm_states, long long *words,
                                 long long *wlen, long long *word_frames, void *word_conf, void *normalisers, hipStream_t stream);

// launch 1 of that call alone: the search with the decoder's end.  With fin_off != 0 it also leaves int32 |A_{len-1}| and, from
// byte 8, the last set (values [K], product states [K], LM states [K]) at that offset of every utterance's block.
template <typename R>
hipError_t launch_beam_word_conf_search(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                        const WordLookArgs *LA, int K, double theta, void *work, size_t per, size_t cnt_off,
                                        size_t fin_off, void *scores, long long *path, long long *tokens, long long *tlen,
                                        long long *states, long long *lm_states, long long *words, long long *wlen,
                                        long long *word_frames, hipStream_t stream);

// ---- The search over pairs carried across chunks with a state that keeps its lattice (asg_beam_word_stream_conf.hip):
// asg_beam_word_conf_stream_*.  One slot: the plain word stream's slot (beam_word_stream_layout) unchanged at the front, then (byte
// offsets, each part 256-byte aligned) cnt int32 [max_frames], the emissions [max_frames][N], nu int32 [max_frames], U u64
// [max_frames][K] (pair keys h << qbits | q, ascending), A [max_frames][K], beta [2][K]:
//     per = P + a256(4 T) + a256(e T N) + a256(4 T) + a256(8 T K) + a256(e T K) + a256(2 e K),   P = beam_word_stream_layout(..).per.
// Header word 3 is apos, the frames whose U / nu / A rows are valid.  `lat` is a BeamWordLossLayout (M = K, nf = 0) over bq / bh /
// cnt / nu / U / A, so WordSets, WordLat<R>::Args and beam_word_conf_pull take it as they take BeamWordConfLayout's; st.per, lat.per
// and per are the slot's stride.  K = beam_size with beam_word_loss_fits(elem, K, N); LA as for the plain word stream.
struct BeamWordConfStreamLayout {
    BeamStreamLayout st;
    BeamWordLossLayout lat;
    size_t em, beta, per;
};
BeamWordConfStreamLayout beam_word_conf_stream_layout(int elem, int max_frames, int K, int cap, int N);
size_t beam_word_conf_stream_state_bytes(int elem, int max_frames, int B, int K, int cap, int N);
// (reset, advance, result and n-best are the plain word stream's launchers with this layout's stride / lattice = true)
// P: B, N and the transition (its emissions and lengths are not read: the state has both).  Two launches: the catch-up of U / nu /
// A from apos to pos (the only write to the state from a result path), then the hypothesis, Z and the beta pull.
template <typename R>
hipError_t launch_beam_word_conf_stream_confidence(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG,
                                                   const WordLmArgs &LM, const WordLookArgs *LA, int K, int max_frames, void *state,
                                                   int final, int tol, void *scores, long long *path, long long *tokens,
                                                   long long *tlen, long long *states, long long *lm_states, long long *words,
                                                   long long *wlen, long long *word_frames, void *word_conf, void *normalisers,
                                                   long long *frames, long long *status, hipStream_t stream);

// ---- Word confidences and end frames for every row of the n-best list (asg_beam_word_nbest_conf.hip):
// asg_beam_words_nbest_confidence.  One utterance's workspace: asg_beam_words_confidence's layout at the front (the search's
// [T][K] rows first), then (byte offsets, each part 256-byte aligned) fin and rows as in BeamWordNbestLayout, hdr (int32 number
// of cells), foff (int32 [T + 2]: the first cell of every frame), qk (u64 [P2(nb * T)]: the rows' (frame, word) queries, sorted
// there when they pass the LDS), cells (u64 [nb * T]: the distinct queries, ascending) and acc (u64 [nb * T]: a cell's fixed-point
// sum).  Behind the utterances: what the one-best search returns (scores, two lengths, six [B][T] arrays).
struct BeamWordNbestConfLayout {
    BeamWordConfLayout conf;     // conf.lat.per and conf.per are this layout's `per`
    size_t fin, rows, hdr, foff, qk, cells, acc, per;
    size_t qcap;                 // P2(nb * T)
    int nb;
};
constexpr int kBeamWordNbestConfSortLds = 2048;   // queries the prep kernel sorts in LDS; more are sorted in the workspace
// the ring of the row sink: the power of two >= min(nbest, K) * (2 tol + 2)
inline size_t beam_word_nbest_conf_ring(int K, int nbest, int tol) {
    const size_t need = (size_t) (nbest < K ? nbest : K) * (2 * (size_t) tol + 2);
    size_t r = 1;
    while (r < need) r *= 2;
    return r;
}
// THE new limit: bwd_front + ring (u64) + mirror (int32) + window offsets and filter (1024 bytes) within 160 KiB of LDS, and
// nb * T <= 2^30.
bool beam_word_nbest_conf_fits(int elem, int T, int K, int nbest, int tol);
BeamWordNbestConfLayout beam_word_nbest_conf_layout(int elem, int T, int K, int cap, int nbest);
size_t beam_word_nbest_conf_work_bytes(int elem, int T, int B, int K, int cap, int nbest);
// path / states / lm_states may be null (then they are not written)
template <typename R>
hipError_t launch_beam_word_nbest_conf(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                                       const WordLookArgs *LA, int K, double theta, int nbest, int tol, void *work, void *scores,
                                       void *emission_scores, void *graph_scores, void *lm_scores, long long *path,
                                       long long *tokens, long long *tlen, long long *states, long long *lm_states,
                                       long long *words, long long *wlen, long long *num_hyps, long long *word_frames,
                                       void *word_conf, void *normalisers, hipStream_t stream);

// ---- Full score, gradients and target walk over the same composed lattice (asg_graph_loss.hip).  The loss-only arrays of
// asg_token_graph_loss.  Work = alpha [T][Q][B] (stored) or [2][Q][B]; scratch = align256([2][Q][B] beta) + [Q+E][B]
// per-stay / per-edge posterior sums.
struct GraphLossArgs {
    int S, start;
    const int *tgt, *orow, *oedge, *lrow, *lq, *pedge, *next;   // [E], [Q+1], [E], [N+1], [Q], [E], [S*N]
    const int64_t *pkey;                                          // [E] label pair i*N + j, ascending (pedge order)
    const void *arcw, *finw;                                      // [S*N], [S] in the dtype of the problem
};
// route: 0 = by shape, 1 = streaming, 2 = resident wherever the vectors fit in LDS
bool graph_loss_resident(int route, int elem, int Q, int64_t E);
size_t graph_loss_work_bytes(int elem, int T, int B, int Q, bool store);
size_t graph_loss_scratch_bytes(int elem, int B, int Q, int E);
template <typename R>
hipError_t launch_graph_loss_forward(const Problem &P, const GraphArgs &G, int route, bool store, void *work, void *scores,
                                     hipStream_t stream);
template <typename R>
hipError_t launch_graph_loss_backward(const Problem &P, const GraphArgs &G, const GraphLossArgs &L, int route, const void *work,
                                      const void *scores, const void *grad_scores, void *grad_inputs, void *grad_transition,
                                      void *scratch, hipStream_t stream);
template <typename R>
hipError_t launch_graph_target_scores(const Problem &P, const GraphLossArgs &L, void *out, hipStream_t stream);

// launches of the resident-slice forward kernel (256 < N <= 2048) of this process whose bounded waits ran out (asg_generic.hip)
unsigned cluster_timeouts();

size_t bwd_scratch_bytes_small(int elem, int T, int B, int N, int S, int *chunk, int *nchunks);
size_t bwd_scratch_bytes_generic(int elem, int T, int B, int N, int S);
size_t fwd_work_bytes_generic(int elem, int T, int B, int N);
size_t step_tile_bytes_generic(int elem, int N, int B);      // one operand-order copy of the normalised transition matrix (0: not used)

}  // namespace asg
