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
//
// The kernel is beam_word_search<.., WordSearch::Decode> of asg_beam_word_search.h, the one text of the family's one-shot search:
// the loss (asg_beam_word_loss.hip) and the confidences (asg_beam_word_conf.hip) compile it in their own modes.  With a
// look-ahead (asg_beam_decode_words_la) it is the same kernel over the frame and the end compiled with the look-ahead flag on
// (asg_beam_word_frame.h says what a value then carries and how L(h, node) is evaluated).
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_word_search.h"  // the kernel and its launcher; the frame and the end are asg_beam_word_frame.h's

namespace asg {

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

// FIN (fin_off != 0): the instantiations behind the n-best stage (asg_beam_word_nbest.hip), which also leave the last set in
// memory; the decoder's own are the code objects they were before that stage existed.
template <typename R>
hipError_t launch_beam_words(const Problem &P, const GraphArgs &G, const BeamGraphArgs &BG, const WordLmArgs &LM,
                             const WordLookArgs *LA, int K, double theta, void *work, void *scores, long long *path,
                             long long *tokens, long long *tlen, long long *states, long long *lm_states, long long *words,
                             long long *wlen, hipStream_t stream, size_t stride, size_t fin_off) {
    const size_t per = stride ? stride : beam_word_work_bytes(sizeof(R), P.T, 1, K, beam_word_cap(K, BG.max_out, BG.num_start));
    return launch_beam_word_search<R, WordSearch::Decode>(P, G, BG, LM, LA, K, theta, work, per, 0, fin_off,
                                                          {scores, path, tokens, tlen, states, lm_states, words, wlen}, nullptr,
                                                          stream);
}
template hipError_t launch_beam_words<float>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                             const WordLookArgs *, int, double, void *, void *, long long *, long long *,
                                             long long *, long long *, long long *, long long *, long long *, hipStream_t, size_t,
                                             size_t);
template hipError_t launch_beam_words<double>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const WordLmArgs &,
                                              const WordLookArgs *, int, double, void *, void *, long long *, long long *,
                                              long long *, long long *, long long *, long long *, long long *, hipStream_t, size_t,
                                              size_t);

}  // namespace asg
