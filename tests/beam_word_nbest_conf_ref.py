"""Test-only numpy restatement of the word confidences and end frames of every row of the word-LM beam decoder's n-best list
(`torch_asg_amd.beam_decode_words_nbest_confidence`), written from the specification
(include/asg_hip.h::asg_beam_words_nbest_confidence).  A COMPOSITION, not a new model:

  rows with their paths   tests/beam_word_nbest_ref.py (`beam_word_nbest_ref`) or, with `order`, tests/beam_word_la_nbest_ref.py;
  events and Z_K          tests/beam_word_conf_ref.py (`beam_word_conf_ref(...)["events"]` / `["normalisers"]`);
  frames of a row         `hypothesis_frames` of that module on the row's path;
  the window sum          the formula, cell by cell.

P(w, t) does not depend on the hypothesis: a row only selects which (word, frame) cells are read.
"""
import numpy as np

from beam_word_conf_ref import beam_word_conf_ref, hypothesis_frames
from beam_word_la_nbest_ref import beam_word_la_nbest_ref
from beam_word_nbest_ref import NAMES, beam_word_nbest_ref
from graph_decode_ref import _clamped_lengths


def beam_word_nbest_conf_ref(inputs, transition, lexicon, lm, input_lengths=None, beam_size=1, nbest=1, beam_threshold=np.inf,
                             lm_weight=1.0, word_score=0.0, token_score=0.0, frame_tolerance=0, order=None, info=None):
    """inputs [T,B,N] (their dtype is the search's dtype) -> dict: the twelve n-best outputs (path, states, lm_states always),
    word_frames [B,nbest,T] int64, word_confidences [B,nbest,T] float64, normalisers [B] float64, events and sets as
    `beam_word_conf_ref` gives them, one_best (that call's whole result), cells (per utterance the sorted distinct (frame, word)
    of all rows) and queries (per utterance the number of (row, k))."""
    xs = np.asarray(inputs)
    T, B, N = xs.shape
    tol = int(frame_tolerance)
    if order is None:
        rows = beam_word_nbest_ref(xs, transition, lexicon, lm, input_lengths, beam_size, nbest, beam_threshold, lm_weight,
                                   word_score, token_score)
    else:
        rows = beam_word_la_nbest_ref(xs, transition, lexicon, lm, order, input_lengths, beam_size, nbest, beam_threshold, lm_weight,
                                      word_score, token_score)
    one = beam_word_conf_ref(xs, transition, lexicon, lm, input_lengths, beam_size, beam_threshold, lm_weight, word_score,
                             token_score, tol, order, info)
    lens = _clamped_lengths(input_lengths, T, B)
    sep = int(lexicon.separator)
    res = {n: rows[n] for n in NAMES}
    res["word_frames"] = np.full((B, nbest, T), -1, np.int64)
    res["word_confidences"] = np.zeros((B, nbest, T))
    res["normalisers"] = one["normalisers"]
    res["events"], res["sets"], res["one_best"] = one["events"], one["sets"], one
    res["cells"], res["queries"] = [], []
    for b in range(B):
        L, P = int(lens[b]), one["events"][b]
        cells, queries = set(), 0
        for r in range(int(rows["num_hyps"][b])):
            nw = int(rows["word_lengths"][b, r])
            if nw == 0:
                continue
            frames = hypothesis_frames(rows["path"][b, r], nw, L, sep)
            res["word_frames"][b, r, :nw] = frames
            for k, tk in enumerate(frames):
                w = int(rows["words"][b, r, k])
                res["word_confidences"][b, r, k] = sum(P.get((w, t), 0.0) for t in range(max(1, tk - tol), min(L, tk + tol) + 1))
                cells.add((tk, w))
                queries += 1
        res["cells"].append(sorted(cells))
        res["queries"].append(queries)
    return res
