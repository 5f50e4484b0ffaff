"""Test-only numpy restatement of the token confidences and start frames of every row of the token-graph beam decoder's n-best
list (`torch_asg_amd.beam_decode_graph_nbest_confidence`), written from the specification
(include/asg_hip.h::asg_beam_graph_nbest_confidence).  A COMPOSITION, not a new model:

  rows with their paths   tests/beam_nbest_ref.py (`beam_nbest_ref`);
  events and Z_K          tests/beam_conf_ref.py (`beam_conf_ref(...)["events"]` / `["normalisers"]`, from `token_events`);
  frames of a row         `start_frames` of that module on the row's path;
  the window sum          the formula, cell by cell.

P(i, t) does not depend on the hypothesis: a row only selects which (frame, label) cells are read.
"""
import numpy as np

from beam_conf_ref import beam_conf_ref, start_frames
from beam_nbest_ref import beam_nbest_ref
from graph_decode_ref import _clamped_lengths

NAMES = ("scores", "emission_scores", "graph_scores", "tokens", "token_lengths", "num_hyps", "path", "states")


def window_confidences(res, input_lengths, tol):
    """The token_confidences [B,nbest,T] of a `beam_nbest_conf_ref` result at another frame_tolerance (the events, the rows and
    their frames do not depend on it)."""
    B, nbest, T = res["token_frames"].shape
    lens = _clamped_lengths(input_lengths, T, B)
    conf = np.zeros((B, nbest, T))
    for b in range(B):
        L, P = int(lens[b]), res["events"][b]
        for r in range(int(res["num_hyps"][b])):
            for k in range(int(res["token_lengths"][b, r])):
                s = int(res["token_frames"][b, r, k])
                conf[b, r, k] = P[max(0, s - tol):min(L - 1, s + tol) + 1, int(res["tokens"][b, r, k])].sum()
    return conf


def beam_nbest_conf_ref(inputs, transition, next_, weight, final, start=0, input_lengths=None, beam_size=1, nbest=1,
                        beam_threshold=np.inf, lm_weight=1.0, token_score=0.0, frame_tolerance=0):
    """inputs [T,B,N] (their dtype is the search's dtype) -> dict: the eight n-best outputs (path and states always),
    token_frames [B,nbest,T] int64, token_confidences [B,nbest,T] float64, normalisers [B] float64, events / sets / sizes as
    `beam_conf_ref` gives them, one_best (that call's whole result), cells (per utterance the sorted distinct (frame, label) of
    all rows) and queries (per utterance the number of (row, k))."""
    xs = np.asarray(inputs)
    T, B, N = xs.shape
    tol = int(frame_tolerance)
    rows = beam_nbest_ref(xs, transition, next_, weight, final, start, input_lengths, beam_size, nbest, beam_threshold, lm_weight,
                          token_score)
    one = beam_conf_ref(xs, transition, next_, weight, final, start, input_lengths, beam_size, beam_threshold, lm_weight,
                        token_score, tol)
    lens = _clamped_lengths(input_lengths, T, B)
    res = dict(zip(NAMES, rows))
    res["token_frames"] = np.full((B, nbest, T), -1, np.int64)
    res["normalisers"] = one["normalisers"]
    res["events"], res["sets"], res["sizes"], res["one_best"] = one["events"], one["sets"], one["sizes"], one
    res["cells"], res["queries"] = [], []
    for b in range(B):
        L = int(lens[b])
        cells, queries = set(), 0
        for r in range(int(res["num_hyps"][b])):
            n = int(res["token_lengths"][b, r])
            s = start_frames(res["path"][b, r, :L])
            assert len(s) == n and [int(res["path"][b, r, t]) for t in s] == [int(v) for v in res["tokens"][b, r, :n]]
            res["token_frames"][b, r, :n] = s
            cells.update((t, int(res["path"][b, r, t])) for t in s)
            queries += n
        res["cells"].append(sorted(cells))
        res["queries"].append(queries)
    res["token_confidences"] = window_confidences(res, input_lengths, tol)
    return res
