"""CPU tests of the word confidences and end frames of every row of the word-LM beam decoder's n-best list
(`torch_asg_amd.beam_decode_words_nbest_confidence`): the numpy restatement (tests/beam_word_nbest_conf_ref.py, a composition
of tests/beam_word_nbest_ref.py and tests/beam_word_conf_ref.py) against the enumeration of every label path, its properties,
and the argument checks of the C entry points and the Python surfaces, none of which needs a device."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, path_score_words, small_lexicon, without_unigrams
from beam_word_conf_ref import beam_word_conf_ref
from beam_word_la_nbest_ref import beam_word_la_nbest_ref
from beam_word_loss_ref import word_model
from beam_word_nbest_conf_ref import beam_word_nbest_conf_ref
from beam_word_nbest_ref import NAMES, beam_word_nbest_ref
from test_beam_word_conf_cpu import double_completion_case, path_events
from test_beam_word_la_cpu import _la, rescue_case
from test_beam_word_loss_cpu import _abi, _emissions, _lse, _pair_seq, _refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
ALL = 10_000
KW = dict(lm_weight=0.7, word_score=-0.4, token_score=0.3)
CALLS = ("asg_beam_words_nbest_confidence_work_bytes", "asg_beam_words_nbest_confidence", "asg_beam_words_nbest_confidence_la")


def _rows(r, b):
    """[(row, [(word, frame)])] of utterance b of a restatement result."""
    out = []
    for i in range(int(r["num_hyps"][b])):
        n = int(r["word_lengths"][b, i])
        out.append((i, [(int(r["words"][b, i, k]), int(r["word_frames"][b, i, k])) for k in range(n)]))
    return out


# ---------------------------------------------------------------------------------------------------------------- enumeration
@pytest.mark.parametrize("order", [2, 3])
def test_every_rows_confidences_are_sums_over_exactly_the_paths_inside_the_sets(order):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = without_unigrams(arpa_lm(5, order, 3 + order), {2})
    T = 5
    x, tr = _emissions(T, 1, 5, 31 + order)
    m = word_model(lex, lm, np.float64, **KW)
    scored = []
    for labels in itertools.product(range(5), repeat=T):                   # all 3125 label paths
        s = path_score_words(x[:, 0], tr, lex, lm, labels, **KW)
        if s > -np.inf:
            seq = _pair_seq(m, labels)
            scored.append((s, seq, path_events(m, labels, seq)))
    lower_rows = 0
    for K in (ALL, 1, 2, 3, 8):
        res = {tol: beam_word_nbest_conf_ref(x, tr, lex, lm, None, K, 8, INF, frame_tolerance=tol, **KW) for tol in (0, 1, 5)}
        sets = [set(u) for u in res[0]["sets"][0]]
        inside = [(s, ev) for s, seq, ev in scored if all(p in sets[t] for t, p in enumerate(seq))]
        Z = _lse([s for s, _ in inside])
        assert np.allclose(res[0]["normalisers"][0], Z, rtol=1e-9, atol=1e-9), K
        direct = {}
        for s, ev in inside:
            for key in ev:
                direct[key] = direct.get(key, 0.0) + np.exp(s - Z)
        nh = int(res[0]["num_hyps"][0])
        assert nh >= 1
        lower_rows += nh - 1
        for tol in (0, 1, 5):
            r = res[tol]
            for i, row in _rows(r, 0):
                # the row's path is a lattice path; its words and frames are that path's own events
                labels = [int(v) for v in r["path"][0, i, :T]]
                seq = _pair_seq(m, labels)
                assert all(p in sets[t] for t, p in enumerate(seq)) and path_events(m, labels, seq) == row, (K, i)
                n = len(row)
                assert (r["word_frames"][0, i, n:] == -1).all() and (r["word_confidences"][0, i, n:] == 0).all()
                for k, (w, tk) in enumerate(row):
                    want = sum(v for (w2, t), v in direct.items() if w2 == w and abs(t - tk) <= tol)
                    assert abs(r["word_confidences"][0, i, k] - want) < 1e-9, (K, tol, i, k)
            assert (r["word_frames"][0, nh:] == -1).all() and (r["word_confidences"][0, nh:] == 0).all()
    assert lower_rows >= 10


def test_one_row_is_the_one_best_call_and_rows_are_prefixes():
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    x, tr = _emissions(7, 4, 5, 31)
    il = np.array([7, 4, 1, 0])
    for K in (1, 3, 8, ALL):
        for tol in (0, 2):
            one = beam_word_conf_ref(x, tr, lex, lm, il, K, 2.0, frame_tolerance=tol, **KW)
            r1 = beam_word_nbest_conf_ref(x, tr, lex, lm, il, K, 1, 2.0, frame_tolerance=tol, **KW)
            r8 = beam_word_nbest_conf_ref(x, tr, lex, lm, il, K, 8, 2.0, frame_tolerance=tol, **KW)
            for r in (r1, r8):
                assert np.array_equal(r["word_frames"][:, 0], one["word_frames"])
                assert np.array_equal(r["word_confidences"][:, 0], one["word_confidences"])
                assert np.array_equal(r["normalisers"], one["normalisers"]) and np.array_equal(r["words"][:, 0], one["words"])
            nb = beam_word_nbest_ref(x, tr, lex, lm, il, K, 8, 2.0, **KW)
            for n in NAMES:
                assert np.array_equal(r8[n], nb[n]), n


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_at_tolerance_zero_every_rows_confidence_lies_between_its_share_and_one(dt):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    below_one = shared = near = 0
    for order in (2, 3):
        lm = arpa_lm(5, order, 60 + order, keep=(1.0, 0.5, 0.5))
        x, tr = _emissions(7, 4, 5, 31, dt)
        il = np.array([7, 4, 1, 0])
        for K in (3, 8, 1024):
            r = beam_word_nbest_conf_ref(x, tr, lex, lm, il, K, 8, INF, **KW)
            assert r["num_hyps"][3] == 0 and r["normalisers"][3] == -np.inf and (r["word_frames"][3] == -1).all()
            assert (r["word_confidences"][3] == 0).all() and not np.isnan(r["word_confidences"]).any()
            for b in range(3):
                cells = {}
                for i, row in _rows(r, b):
                    share = np.exp(float(r["scores"][b, i]) - r["normalisers"][b])
                    c = r["word_confidences"][b, i, :len(row)]
                    assert (c >= share - 1e-5).all() and (c <= 1 + 1e-9).all(), (order, K, b, i)
                    below_one += int((c < 0.999).sum())
                    f = r["word_frames"][b, i, :len(row)]
                    assert (np.diff(f) > 0).all() and (f >= 1).all() and (f <= il[b]).all()
                    for k, (w, t) in enumerate(row):       # rows that hold the same word ending at the same frame: one value
                        assert cells.setdefault((t, w), c[k]) == c[k]
                assert sorted(cells) == r["cells"][b]
                shared += r["queries"][b] - len(cells)
                near += sum(1 for (t, w) in cells if (t + 1, w) in cells)
    assert below_one > 20 and shared > 20 and near >= 2     # cells shared between rows, and one word one frame apart


def test_the_same_words_listed_twice_closed_at_the_root_and_by_the_end_rule():
    """0, 1 | 2, separator ends at the root with its word closed at frame 2; 0, 1 | 2, 2 holds the letter and the end rule closes
    the same word at len = 3."""
    lex, lm, x, tr = rescue_case(np.float64)
    r = beam_word_nbest_conf_ref(x, tr, lex, lm, None, ALL, 8)
    rows = _rows(r, 0)
    by_words = {}
    for i, row in rows:
        by_words.setdefault(tuple(w for w, _ in row), []).append([t for _, t in row])
    twice = [f for f in by_words.values() if len(f) >= 2]
    assert twice and any(sorted(a[-1] for a in f)[-1] == 3 and sorted(a[-1] for a in f)[0] == 2 for f in twice)
    for i, row in rows:
        for k, (w, t) in enumerate(row):
            assert abs(r["word_confidences"][0, i, k] - r["events"][0][(w, t)]) < 1e-15


def test_the_double_completion_on_a_lower_row():
    lex, lm, x, tr = double_completion_case()
    r0 = beam_word_nbest_conf_ref(x, tr, lex, lm, None, ALL, 8)
    r2 = beam_word_nbest_conf_ref(x, tr, lex, lm, None, ALL, 8, frame_tolerance=2)
    assert r0["num_hyps"][0] >= 2 and _rows(r0, 0)[0][1] == [(0, 1), (0, 3)]
    assert (r0["word_confidences"] <= 1 + 1e-12).all()
    lower = [(i, row) for i, row in _rows(r2, 0) if i >= 1 and row]
    assert lower and any((r2["word_confidences"][0, i, :len(row)] > 1.2).any() for i, row in lower)     # unclipped
    P = r2["events"][0]
    for i, row in _rows(r2, 0):
        for k, (w, t) in enumerate(row):
            assert abs(r2["word_confidences"][0, i, k] - sum(P.get((w, u), 0.0) for u in range(max(1, t - 2), min(4, t + 2) + 1))) < 1e-12


def test_lengths_one_and_zero():
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 2, 9)
    x, tr = _emissions(4, 2, 5, 46)
    r = beam_word_nbest_conf_ref(x, tr, lex, lm, np.array([1, 0]), ALL, 6, INF, frame_tolerance=3, **KW)
    assert r["num_hyps"][0] >= 2
    for i, row in _rows(r, 0):
        assert len(row) == 1 and row[0][1] == 1 and 0 < r["word_confidences"][0, i, 0] < 1
    assert abs(sum(r["word_confidences"][0, i, 0] for i, _ in _rows(r, 0)) - sum(r["events"][0][(w, 1)] for _, ((w, _),) in _rows(r, 0))) < 1e-12
    assert r["num_hyps"][1] == 0 and r["normalisers"][1] == -np.inf
    assert (r["word_frames"][1] == -1).all() and (r["word_confidences"][1] == 0).all() and r["cells"][1] == []


@pytest.mark.parametrize("order", [1, 2, 3])
def test_look_ahead_rows_with_plain_weights(order):
    lex, lm, x, tr = rescue_case(np.float64)
    plain = beam_word_nbest_conf_ref(x, tr, lex, lm, None, 1, 4)
    r = beam_word_nbest_conf_ref(x, tr, lex, lm, None, 1, 4, order=order)
    la = beam_word_la_nbest_ref(x, tr, lex, lm, order, None, 1, 4)
    for n in NAMES:
        assert np.array_equal(r[n], la[n]), n
    assert plain["words"][0, 0, 0] == 0 and r["words"][0, 0, 0] == 1 and r["sets"] != plain["sets"]
    one = beam_word_conf_ref(x, tr, lex, lm, None, 1, order=order)
    assert np.array_equal(r["word_frames"][:, 0], one["word_frames"]) and r["normalisers"][0] == one["normalisers"][0]
    assert abs(r["word_confidences"][0, 0, 0] - 1.0) < 1e-12 and r["word_frames"][0, 0, 0] == 2


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in CALLS:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    assert "#define ASG_HIP_VERSION 230" in src and _lib.ABI_VERSION == 230


def _p2(n):
    r = 2
    while r < n:
        r *= 2
    return r


def test_work_bytes_are_the_stated_formula_and_have_no_term_in_the_lm():
    lex = small_lexicon()
    small, big = arpa_lm(5, 2, 1), arpa_lm(5, 3, 1, keep=(1.0, 1.0, 1.0))
    assert big.H > 2 * small.H and big.A > 2 * small.A
    al = lambda n: (n + 255) // 256 * 256                                                       # noqa: E731
    for dtype, e in ((torch.float32, 4), (torch.float64, 8)):
        for T, B, K, nbest in ((7, 3, 16, 1), (100, 2, 300, 40), (5, 1, 8, 9), (33, 2, 64, 64)):
            L, p, gb, w, keep = _abi(lex, small, T, B, dtype, 0)
            L2, p2, gb2, w2, keep2 = _abi(lex, big, T, B, dtype, 0)
            conf = int(L.asg_beam_words_confidence_work_bytes(*_refs(p, gb, w), K))
            a = int(L.asg_beam_words_nbest_confidence_work_bytes(*_refs(p, gb, w), K, nbest))
            assert a == int(L2.asg_beam_words_nbest_confidence_work_bytes(*_refs(p2, gb2, w2), K, nbest)) > 0
            nb = min(nbest, K)
            per = (conf // B + al(8 + K * (e + 8)) + al(T * nb * 4) + 256 + al((T + 2) * 4) + al(_p2(nb * T) * 8)
                   + 2 * al(nb * T * 8))
            assert a == B * per + 3 * al(B * 8) + al(6 * B * T * 8)


def test_abi_argument_checks_without_a_device():
    from torch_asg_amd import _lib
    lex, lm = small_lexicon(), arpa_lm(5, 2, 1)
    for dtype, e in ((torch.float32, 4), (torch.float64, 8)):
        L, p, gb, w, keep = _abi(lex, lm, 7, 3, dtype, 0)
        wb = lambda K, n=4: int(L.asg_beam_words_nbest_confidence_work_bytes(*_refs(p, gb, w), K, n))     # noqa: E731
        mmax = (160 * 1024 - 256) // (16 + e)              # the pair loss's bound on M = K
        assert wb(min(mmax, 8192)) > 0 and wb(0) == 0 and wb(8193) == 0 and wb(8, 0) == 0 and wb(8, 8193) == 0
        assert wb(8, 8192) > 0
        outs = ["scores", "emission_scores", "graph_scores", "lm_scores", "path", "tokens", "token_lengths", "states", "lm_states",
                "words", "word_lengths", "num_hyps", "word_frames", "word_confidences", "normalisers"]
        optional = ("path", "states", "lm_states")

        def call(K=8, th=1.0, nbest=4, tol=0, work=256, nbytes=1 << 40, la=None, **null):
            ptrs = [None if n in null else 256 for n in outs]
            if la is not None:
                return L.asg_beam_words_nbest_confidence_la(None, *_refs(p, gb, w), la, K, th, nbest, tol, work, nbytes, *ptrs, 0, None)
            return L.asg_beam_words_nbest_confidence(None, *_refs(p, gb, w), K, th, nbest, tol, work, nbytes, *ptrs, 0, None)
        # the decoder's argument checks
        assert call(K=0) == 1 and call(th=-1.0) == 1 and call(th=float("nan")) == 1 and call(K=8193) == 2
        assert call(work=None) == 1
        for n in outs:
            assert call(nbytes=wb(8) - 1, **{n: None}) == (3 if n in optional else 1), n
        # the n-best's, then the tolerance: each in front of what comes behind it
        assert call(nbest=0) == 1 and call(nbest=8193) == 2 and call(nbest=0, tol=65) == 1 and call(nbest=8193, tol=-1) == 2
        assert call(K=0, nbest=8193) == 1 and call(K=8193, nbest=0) == 2
        assert call(tol=-1) == 1 and call(tol=65) == 2 and call(tol=-1, work=None) == 1 and call(tol=65, th=-1.0) == 2
        # one combination either side of the new limit: 16 * ceil(M (e + 8) / 16) + 1024 + 12 * P2(min(nbest, K) (2 tol + 2))
        fits = lambda K, n, tol: 16 * ((K * (e + 8) + 15) // 16) + 1024 + 12 * _p2(min(n, K) * (2 * tol + 2)) <= 163840     # noqa: E731
        assert fits(64, 63, 64) and not fits(64, 64, 64) and fits(1024, 1024, 3) and not fits(1024, 1024, 4)
        assert call(K=64, nbest=63, tol=64, nbytes=wb(64, 63) - 1) == 3 and call(K=64, nbest=64, tol=64) == 2
        assert call(K=1024, nbest=2000, tol=3, nbytes=wb(1024, 2000) - 1) == 3 and call(K=1024, nbest=2000, tol=4) == 2
        assert call(K=64, nbest=64, tol=64, th=-1.0) == 2 and wb(64, 64) > 0       # the limit is the call's, not the workspace's
        # a workspace one byte short, before anything is launched
        assert call(nbytes=wb(8) - 1) == 3 and call(tol=64, nbytes=wb(8) - 1) == 3 and call(nbest=5, nbytes=wb(8, 5) - 1) == 3
        assert wb(8, 5) > wb(8, 4)
        w.dtype = 1 - w.dtype
        assert call() == 1 and wb(8) == 0
        w.dtype = 1 - w.dtype
        for field, bad in (("start", lm.H), ("separator", 5), ("H", 0), ("row", None), ("word_of_state", None)):
            old = getattr(w, field)
            setattr(w, field, bad)
            assert call() == 1, field
            setattr(w, field, old)
        p.T = (1 << 20) + 1
        assert call() == 2 and wb(8) == 0
        p.T = 7
        # the look-ahead's checks, behind the tolerance and in front of the threshold
        look = _la(_lib, S=int(w.S), H=int(w.H), A=min(int(w.A), 4), levels=2, dtype=p.dtype)
        ref = ctypes.byref(look)
        assert call(la=ref, nbytes=wb(8) - 1) == 3 and call(la=ref, tol=65) == 2 and call(la=ref, K=0) == 1
        assert call(la=ref, nbest=0) == 1
        assert L.asg_beam_words_nbest_confidence_la(None, *_refs(p, gb, w), None, 8, 1.0, 4, 0, 256, 1 << 40, *([256] * 15), 0,
                                                    None) == 1
        look.H += 1
        assert call(la=ref) == 1 and call(la=ref, tol=65) == 2 and call(la=ref, th=-1.0) == 1
        look.H -= 1
        look.dtype = 1 - look.dtype
        assert call(la=ref) == 1
        look.dtype = 1 - look.dtype
        look.rlo = None
        assert call(la=ref) == 1


# ---------------------------------------------------------------------------------------------------------------- Python
def test_python_surfaces_refuse_bad_arguments_before_any_launch():
    import torch_asg_amd as A
    from torch_asg_amd.asg import native
    lex, lm = small_lexicon(), arpa_lm(5, 2, 1)
    x, tr = torch.zeros(4, 2, 5), torch.zeros(5, 5)
    crit = A.ASGLoss(5)
    surfaces = (lambda *a, **k: A.beam_decode_words_nbest_confidence(x, tr, *a, **k),
                lambda lex_, lm_, **k: native().beam_decode_words_nbest_confidence(x, tr, lex_, lm_, None, k.pop("beam_size", 8),
                                                                                   k.pop("nbest", 3), **k),
                lambda *a, **k: crit.beam_decode_words_nbest_confidence(x, *a, **k))
    other = small_lexicon()
    for f in surfaces:
        with pytest.raises(TypeError, match="Lexicon"):
            f(lex.graph, lm)
        with pytest.raises(TypeError, match="WordLM"):
            f(lex, None)
        with pytest.raises(RuntimeError, match="knows"):
            f(lex, A.WordLM.null(3))
        with pytest.raises(TypeError, match="WordLookahead"):
            f(lex, lm, lookahead=3)
        with pytest.raises(RuntimeError, match="another lexicon"):
            f(lex, lm, lookahead=A.WordLookahead(other, lm, 2))
        with pytest.raises(RuntimeError, match="ROCm device"):                     # the pair is checked before the device
            f(lex, lm, frame_tolerance=1)
    with pytest.raises(ValueError, match="beam_size"):
        A.beam_decode_words_nbest_confidence(x, tr, lex, lm, beam_size=0)
    with pytest.raises(ValueError, match="beam_threshold"):
        crit.beam_decode_words_nbest_confidence(x, lex, lm, beam_threshold=-1.0)
    with pytest.raises(ValueError, match="nbest"):
        A.beam_decode_words_nbest_confidence(x, tr, lex, lm, nbest=0)
    with pytest.raises(ValueError, match="nbest"):
        crit.beam_decode_words_nbest_confidence(x, lex, lm, nbest=0)
    for name in ("BeamWordsNbestConfidence", "beam_decode_words_nbest_confidence"):
        assert name in A.__all__ and hasattr(A, name)
    assert A.BeamWordsNbestConfidence._fields == A.BeamWordsNbest._fields + ("word_frames", "word_confidences", "normalisers")
