"""CPU tests that pin tests/beam_word_nbest_ref.py, the yardstick of the GPU tests of the n-best over pairs
(tests/test_hip_beam_word_nbest.py): row 0 against the one-best restatements, the whole list against an enumeration of every
label path scored by a function written apart from the search, the bound that holds the three parts to the score, repeated
word sequences, the prefix mode, padding, short utterances and a beam without an end.  No device, no package kernels."""
import numpy as np
import pytest

from beam_word_cases import arpa_lm, eighths, small_lexicon
from beam_word_nbest_cases import enumerate_groups, split_bound
from beam_word_nbest_ref import NAMES, BeamWordNbestStreamRef, beam_word_nbest_ref
from beam_word_ref import beam_word_ref
from beam_word_stream_ref import BeamWordStreamRef

INF = np.inf
ALL = 1024
ONE_BEST = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths")
DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])


def _normal(T, B, N, seed, dt):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, B, N)).astype(dt), rng.standard_normal((N, N)).astype(dt)


def _padding_is_as_specified(res, nbest):
    for b, nh in enumerate(res["num_hyps"]):
        assert nh == min(nbest, res["num_cands"][b])
        for n in NAMES:
            if n == "num_hyps":
                continue
            pad = res[n][b, nh:]
            want = -np.inf if n.endswith("scores") else (0 if n.endswith("lengths") else -1)
            assert (pad == want).all(), n
        assert np.isfinite(res["scores"][b, :nh]).all()


@DTYPES
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_row_0_is_the_one_best_restatement_byte_for_byte(order, dt):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, order, 60 + order, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(7, 4, 5, 31, dt)
    il = np.array([7, 4, 1, 0])
    for K in (1, 3, 8, ALL):
        for theta in (INF, 2.0, 0.0):
            one = beam_word_ref(x, tr, lex, lm, il, K, theta, 0.7, -0.4, 0.3)
            for nbest in (1, 3):
                res = beam_word_nbest_ref(x, tr, lex, lm, il, K, nbest, theta, 0.7, -0.4, 0.3)
                for n in ONE_BEST:
                    assert res[n][:, 0].tobytes() == one[n].tobytes(), (n, K, theta)
                _padding_is_as_specified(res, nbest)


@DTYPES
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("lm_kind", ["full", "sparse"])
def test_the_full_list_equals_an_enumeration_of_every_label_path(lm_kind, T, dt):
    """3125 label paths at T = 5, K = all.  With every trigram in the LM ("full") no two token sequences of at most three words
    share a history, so a token sequence is a pair: the best path per collapsed token sequence is a row.  With a trigram LM that
    backs off ("sparse"), token sequences whose histories the LM no longer tells apart end in ONE pair and the search keeps the
    best of them (Viterbi recombination): the rows are the best path per pair, fewer than the token sequences."""
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 3, 63, keep=(1.0, 1.0, 1.0) if lm_kind == "full" else (1.0, 0.5, 0.5))
    x, tr = _normal(T, 1, 5, 41, dt)
    kw = dict(lm_weight=0.7, word_score=-0.4, token_score=0.3)
    groups = enumerate_groups(x[:, 0], tr, lex, lm, True, "tokens" if lm_kind == "full" else "pair", **kw)
    if lm_kind == "sparse" and T == 5:
        assert len(enumerate_groups(x[:, 0], tr, lex, lm, True, "tokens", **kw)) > len(groups)       # something recombined
    sc = [g[0][0] for g in groups]
    assert not any(g[1] for g in groups) and len(set(sc)) == len(sc)       # no exact tie for this seed: rows are comparable
    res = beam_word_nbest_ref(x, tr, lex, lm, None, ALL, ALL, INF, 0.7, -0.4, 0.3)
    nh = int(res["num_hyps"][0])
    assert nh == len(groups) and (T < 5 or nh > 20)
    assert res["scores"][0, :nh].tobytes() == np.array(sc, dt).tobytes()
    for r, ((v, em, gr, ls, tokens, words, _p), _) in enumerate(groups):
        assert res["tokens"][0, r, :len(tokens)].tolist() == tokens and res["token_lengths"][0, r] == len(tokens)
        assert res["words"][0, r, :len(words)].tolist() == words and res["word_lengths"][0, r] == len(words)
        assert (res["tokens"][0, r, len(tokens):] == -1).all() and (res["words"][0, r, len(words):] == -1).all()
        got = np.array([res[n][0, r] for n in ("emission_scores", "graph_scores", "lm_scores")], dt)
        assert got.tobytes() == np.array([em, gr, ls], dt).tobytes(), r
    _padding_is_as_specified(res, ALL)


@DTYPES
def test_the_three_parts_agree_with_the_score_within_the_bound(dt):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(9, 3, 5, 42, dt)
    res = beam_word_nbest_ref(x, tr, lex, lm, np.array([9, 5, 1]), 64, 64, INF, 0.7, -0.4, 0.3)
    diff, bound, fin = split_bound(res, dt)
    assert fin.sum() > 40 and (diff[fin] <= bound[fin]).all()
    assert (res["nterms"][fin] >= 4).all()                   # an emission, the start and final weights, the LM's end at least
    # every term a multiple of 1/8: every sum is exact, whatever its order
    rng = np.random.default_rng(43)
    xe = (rng.integers(-32, 32, (9, 3, 5)) / 8.0).astype(dt)
    te = (rng.integers(-16, 16, (5, 5)) / 8.0).astype(dt)
    res = beam_word_nbest_ref(xe, te, small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25]), eighths(lm), np.array([9, 5, 1]), 64, 64, INF,
                              1.0, 0.25, 0.125)
    diff, _, fin = split_bound(res, dt)
    assert fin.sum() > 40 and (diff[fin] == 0).all()


@DTYPES
def test_one_word_sequence_twice_with_and_without_its_closing_separator(dt):
    from torch_asg_amd import Lexicon, WordLM
    lex = Lexicon([[0], [0, 1]], 3, 2)                       # nodes: 0 root, 1 "0" (word 0), 2 "01" (word 1)
    lm = WordLM(2, [0, 2, 3], [0, 1, 0], [-0.5, -1.0, -0.25], [1, 1, 0], [-1, 0], [0.0, -0.125], 0, [-2.0, -0.75])
    tr = np.zeros((3, 3), dt)
    x = np.full((3, 2, 3), -9.0, dt)
    x[:, 0, 0] = 0.0
    x[2, 0, 2] = -0.5                                        # "0 0 |" a little behind "0 0 0"
    x[:, 1, 0] = 0.0
    x[2, 1, 2] = 0.5                                         # ... and a little ahead of it
    res = beam_word_nbest_ref(x, tr, lex, lm, None, ALL, 2, INF)
    for b, first in ((0, [0]), (1, [0, 2])):
        second = [0, 2] if first == [0] else [0]
        assert res["num_hyps"][b] == 2 and res["scores"][b, 0] > res["scores"][b, 1]
        assert res["words"][b, :, :2].tolist() == [[0, -1], [0, -1]] and res["word_lengths"][b].tolist() == [1, 1]
        assert res["tokens"][b, 0, :len(first)].tolist() == first and res["token_lengths"][b, 0] == len(first)
        assert res["tokens"][b, 1, :len(second)].tolist() == second and res["token_lengths"][b, 1] == len(second)
        ends = [int(res["states"][b, r, 2]) for r in range(2)]
        assert sorted(ends) == [0, 1] and ends[0] == (1 if first == [0] else 0)      # the word-end node and the root


@DTYPES
def test_prefix_mode(dt):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(5, 2, 5, 44, dt)
    kw = dict(lm_weight=0.7, word_score=-0.4, token_score=0.3)
    for K in (1, 3, 8, ALL):
        a = BeamWordNbestStreamRef(tr, lex, lm, 2, 6, K, 2.0 if K == 3 else INF, dtype=dt, **kw)
        b = BeamWordStreamRef(tr, lex, lm, 2, 6, K, 2.0 if K == 3 else INF, dtype=dt, **kw)
        for chunk, cl in ((x[:2], None), (x[2:5], np.array([3, 1]))):
            a.advance(chunk, cl)
            b.advance(chunk, cl)
            for final in (False, True):
                res, one = a.result_nbest(4, final), b.result(final)
                for n in ONE_BEST + ("frames", "status"):
                    got = res[n] if n in ("frames", "status") else res[n][:, 0]
                    assert got.tobytes() == one[n].tobytes(), (n, K, final)
                _padding_is_as_specified(res, 4)
    # K = all: every prefix, by an enumeration scored without end terms; mid-word prefixes are rows
    a = BeamWordNbestStreamRef(tr, lex, lm, 1, 5, ALL, INF, dtype=dt, **kw)
    a.advance(x[:, :1])
    res = a.result_nbest(ALL, False)
    groups = enumerate_groups(x[:, 0], tr, lex, lm, False, "pair", **kw)
    sc = [g[0][0] for g in groups]
    nh = int(res["num_hyps"][0])
    assert not any(g[1] for g in groups) and len(set(sc)) == len(sc) and nh == len(groups)
    assert res["scores"][0, :nh].tobytes() == np.array(sc, dt).tobytes()
    wos = np.asarray(lex.word_of_state)
    last = res["states"][0, np.arange(nh), 4]
    assert ((last != 0) & (wos[last] < 0)).any()             # some row ends mid-word
    for r, ((v, em, gr, ls, tokens, words, _p), _) in enumerate(groups):
        assert res["tokens"][0, r, :res["token_lengths"][0, r]].tolist() == tokens
        assert res["words"][0, r, :res["word_lengths"][0, r]].tolist() == words
        got = np.array([res[n][0, r] for n in ("emission_scores", "graph_scores", "lm_scores")], dt)
        assert got.tobytes() == np.array([em, gr, ls], dt).tobytes(), r
    assert a.result_nbest(ALL, True)["num_hyps"][0] < nh     # with the end, mid-word pairs are no rows


@DTYPES
def test_padding_rows_lengths_0_and_1_and_a_beam_without_an_end(dt):
    from torch_asg_amd import Lexicon, WordLM
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 2, 62, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(6, 3, 5, 45, dt)
    il = np.array([6, 1, 0])
    for K in (2, 6):
        for nbest in (1, 2, K, K + 5):
            res = beam_word_nbest_ref(x, tr, lex, lm, il, K, nbest, INF, 0.7, -0.4, 0.3)
            assert res["scores"].shape == (3, nbest) and res["tokens"].shape == (3, nbest, 6)
            _padding_is_as_specified(res, nbest)
            assert res["num_hyps"][2] == 0 and res["num_cands"][2] == 0
            assert (res["path"][1, :, 1:] == -1).all() and (res["token_lengths"][1, :res["num_hyps"][1]] == 1).all()
    assert beam_word_nbest_ref(x, tr, lex, lm, il, 6, 6, INF)["num_hyps"][1] >= 2            # T = 1: several one-token words
    long = Lexicon([[0, 1, 0]], 3, 2)
    res = beam_word_nbest_ref(x[:2, :, :3], tr[:3, :3], long, WordLM.null(1), None, 8, 3, INF)
    assert (res["num_hyps"] == 0).all() and (res["num_cands"] == 0).all()
    _padding_is_as_specified(res, 3)
