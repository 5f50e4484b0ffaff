"""CPU tests that pin the numpy restatement of the word confidences (tests/beam_word_conf_ref.py) before the GPU tests compare
the kernels with it: every P(w, t) against the enumeration of all label paths, the properties the specification states (K = 1,
the bounds at tolerance 0, the expected word count as a derivative, a double completion above 1, both kinds of final word,
lengths 1 and 0, the look-ahead sets with plain weights), and the C ABI of asg_beam_words_confidence* (symbols, sizes, argument
checks) and the Python surfaces' argument errors -- no kernel is launched here."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, path_score_words, small_lexicon, without_unigrams
from beam_word_conf_ref import DECODE, beam_word_conf_ref, word_events
from beam_word_la_loss_ref import beam_word_la_loss_ref
from beam_word_la_ref import beam_word_la_ref
from beam_word_loss_ref import beam_word_loss_ref, lattice_sets, word_model
from beam_word_ref import beam_word_ref
from test_beam_word_la_cpu import _la, rescue_case
from test_beam_word_loss_cpu import _abi, _emissions, _lse, _pair_seq, _refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
ALL = 10_000
KW = dict(lm_weight=0.7, word_score=-0.4, token_score=0.3)


def path_events(m, labels, seq):
    """The word-end events of one label path with pairs `seq`: [(word, frame)]."""
    L = len(labels)
    ev = [(int(m.wos[m.state[seq[t - 1][1]]]), t) for t in range(1, L) if labels[t] == m.sep and labels[t - 1] != m.sep]
    s = int(m.state[seq[-1][1]])
    if s != 0:
        ev.append((int(m.wos[s]), L))
    return ev


# ---------------------------------------------------------------------------------------------------------------- enumeration
@pytest.mark.parametrize("order", [2, 3])
def test_every_event_posterior_is_the_sum_over_exactly_the_paths_inside_the_sets(order):
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
    assert len(scored) > 20
    pruned, windows_differ = 0, 0
    for K in (ALL, 1, 2, 3, 8):
        res = {tol: beam_word_conf_ref(x, tr, lex, lm, None, K, INF, frame_tolerance=tol, **KW) for tol in (0, 1, 5)}
        sets = [set(u) for u in res[0]["sets"][0]]
        inside = [(s, ev) for s, seq, ev in scored if all(p in sets[t] for t, p in enumerate(seq))]
        pruned += len(inside) < len(scored)
        Z = _lse([s for s, _ in inside])
        assert np.allclose(res[0]["normalisers"][0], Z, rtol=1e-9, atol=1e-9), K
        direct = {}
        for s, ev in inside:
            for key in ev:
                direct[key] = direct.get(key, 0.0) + np.exp(s - Z)
        got = res[0]["events"][0]
        assert set(got) == set(direct) and len(direct) >= 1
        for key, v in direct.items():
            assert abs(got[key] - v) < 1e-9, (K, key)
        # the hypothesis: the winning path is the best path inside the sets, its frames are its own events' frames
        best = max(inside, key=lambda it: it[0])
        nw = int(res[0]["word_lengths"][0])
        assert nw == len(best[1]) and [w for w, _ in best[1]] == list(res[0]["words"][0, :nw])
        assert [t for _, t in best[1]] == list(res[0]["word_frames"][0, :nw])
        for tol in (0, 1, 5):
            r = res[tol]
            assert (r["word_frames"][0, nw:] == -1).all() and (r["word_confidences"][0, nw:] == 0).all()
            for k, (w, tk) in enumerate(best[1]):
                want = sum(v for (w2, t), v in direct.items() if w2 == w and abs(t - tk) <= tol)
                assert abs(r["word_confidences"][0, k] - want) < 1e-9, (K, tol, k)
        windows_differ += not np.allclose(res[0]["word_confidences"], res[5]["word_confidences"])
    assert pruned >= 3 and windows_differ >= 1


# ---------------------------------------------------------------------------------------------------------------- properties
def test_a_beam_of_one_is_sure_of_every_word():
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 2, 9)
    x, tr = _emissions(9, 3, 5, 45)
    for tol in (0, 2):
        r = beam_word_conf_ref(x, tr, lex, lm, np.array([9, 6, 2]), 1, INF, frame_tolerance=tol, **KW)
        assert (r["word_lengths"] >= 1).all()
        for b in range(3):
            nw = int(r["word_lengths"][b])
            wd, wf = r["words"][b, :nw], r["word_frames"][b, :nw]
            # one path: a word counts itself and every equal word of the hypothesis that ends inside its window
            want = [sum(1 for j in range(nw) if wd[j] == wd[k] and abs(wf[j] - wf[k]) <= tol) for k in range(nw)]
            assert tol > 0 or want == [1] * nw
            assert np.allclose(r["word_confidences"][b, :nw], want, rtol=0, atol=1e-12)
        assert np.allclose(r["normalisers"], r["scores"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_at_tolerance_zero_a_confidence_lies_between_the_paths_share_and_one(dt):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    below_one = 0
    for order in (2, 3):
        lm = arpa_lm(5, order, 60 + order, keep=(1.0, 0.5, 0.5))
        x, tr = _emissions(7, 4, 5, 31, dt)
        il = np.array([7, 4, 1, 0])
        for K in (1, 2, 3, 8, ALL):
            for theta in (INF, 2.0, 0.0):
                r = beam_word_conf_ref(x, tr, lex, lm, il, K, theta, **KW)
                assert r["scores"][3] == -np.inf and r["normalisers"][3] == -np.inf and (r["word_frames"][3] == -1).all()
                assert (r["word_confidences"][3] == 0).all() and not np.isnan(r["word_confidences"]).any()
                for b in range(3):
                    nw = int(r["word_lengths"][b])
                    share = np.exp(float(r["scores"][b]) - r["normalisers"][b])
                    c = r["word_confidences"][b, :nw]
                    assert (c >= share - 1e-5).all() and (c <= 1 + 1e-9).all(), (order, K, theta, b)
                    below_one += int((c < 0.999).sum())
                    f = r["word_frames"][b, :nw]
                    assert (np.diff(f) > 0).all() and (f >= 1).all() and (f <= il[b]).all()
    assert below_one > 20


def test_the_events_sum_to_the_derivative_of_z_in_the_word_score():
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 3, 7)
    x, tr = _emissions(8, 2, 5, 52)
    il = np.array([8, 5])
    seen = []
    for K in (3, ALL):
        r = beam_word_conf_ref(x, tr, lex, lm, il, K, INF, **KW)
        eps = 1e-5
        for b in range(2):
            z = []
            for ws in (KW["word_score"] + eps, KW["word_score"] - eps):
                m = word_model(lex, lm, np.float64, KW["lm_weight"], ws, KW["token_score"])
                z.append(word_events(m, x[:, b], tr, int(il[b]), r["sets"][b])[0])          # the sets frozen
            total = sum(r["events"][b].values())
            assert abs((z[0] - z[1]) / (2 * eps) - total) < 1e-7, (K, b)
            seen.append(total)
    assert min(seen) > 0.5 and sum(1 for s in seen if abs(s - round(s)) > 0.05) >= 2        # not a count of one path's words


def double_completion_case(dt=np.float64):
    """One one-letter word; the emissions favour letter, separator, letter, separator: the word is completed at frames 1 and 3."""
    from torch_asg_amd import Lexicon, WordLM
    lex = Lexicon([[0]], 2, 1)
    lm = WordLM(1, [0, 1], [0], [-0.5], [0], [-1], [0.0], 0, [-0.25])
    x = np.full((4, 1, 2), -3.0, dt)
    x[0, 0, 0] = x[1, 0, 1] = x[2, 0, 0] = x[3, 0, 1] = 0.0
    return lex, lm, x, np.zeros((2, 2), dt)


def test_a_short_word_completed_twice_inside_the_window_counts_twice():
    lex, lm, x, tr = double_completion_case()
    r0 = beam_word_conf_ref(x, tr, lex, lm, None, ALL, INF)
    assert list(r0["path"][0]) == [0, 1, 0, 1] and list(r0["words"][0, :2]) == [0, 0] and list(r0["word_frames"][0, :2]) == [1, 3]
    assert (r0["word_confidences"][0, :2] <= 1 + 1e-12).all() and (r0["word_confidences"][0, :2] > 0.5).all()
    r1 = beam_word_conf_ref(x, tr, lex, lm, None, ALL, INF, frame_tolerance=1)       # |1 - 3| = 2: the windows do not meet
    assert (r1["word_confidences"][0, :2] <= 1 + 1e-12).all()
    r2 = beam_word_conf_ref(x, tr, lex, lm, None, ALL, INF, frame_tolerance=2)
    c = r2["word_confidences"][0, :2]
    assert (c > 1.2).all() and (c <= 2 + 1e-12).all()                               # an expected count, unclipped
    P = r2["events"][0]
    assert abs(c[0] - (P[(0, 1)] + P.get((0, 2), 0.0) + P[(0, 3)])) < 1e-12


def test_a_final_word_by_the_end_rule_and_one_closed_at_the_root():
    lex, lm, x, tr = rescue_case(np.float64)
    closed = beam_word_conf_ref(x, tr, lex, lm, None, ALL)                          # 0, 1 | 2, separator: ends at the root
    assert closed["path"][0, 2] == lex.separator and closed["word_lengths"][0] == 1 and closed["word_frames"][0, 0] == 2
    w = int(closed["words"][0, 0])
    assert (w, 2) in closed["events"][0] and set(t for _, t in closed["events"][0]) == {2, 3}   # (3: letter held, then the end rule)
    opened = beam_word_conf_ref(x[:2], tr, lex, lm, None, ALL)                      # two frames: the end rule closes the word
    assert opened["word_lengths"][0] == 1 and opened["word_frames"][0, 0] == 2 and opened["path"][0, 1] != lex.separator
    assert set(t for _, t in opened["events"][0]) == {2}
    for r in (closed, opened):
        both = r["events"][0]
        assert {w_ for w_, _ in both} == {0, 1} and abs(sum(both.values()) - 1.0) < 1e-12    # every path ends exactly one word
        assert abs(r["word_confidences"][0, 0] - both[(int(r["words"][0, 0]), 2)]) < 1e-15
        assert 0.5 < r["word_confidences"][0, 0] < 1.0


def test_lengths_one_and_zero():
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 2, 9)
    x, tr = _emissions(4, 2, 5, 46)
    r = beam_word_conf_ref(x, tr, lex, lm, np.array([1, 0]), ALL, INF, frame_tolerance=3, **KW)
    assert r["word_lengths"][0] == 1 and r["word_frames"][0, 0] == 1 and (r["word_frames"][0, 1:] == -1).all()
    assert 0 < r["word_confidences"][0, 0] < 1 and set(t for _, t in r["events"][0]) == {1}
    assert abs(sum(r["events"][0].values()) - 1.0) < 1e-12                          # one frame: every path ends a one-letter word
    assert r["normalisers"][1] == -np.inf and (r["word_frames"][1] == -1).all() and (r["word_confidences"][1] == 0).all()
    assert r["events"][1] == {}


@pytest.mark.parametrize("order", [1, 2, 3])
def test_look_ahead_sets_and_hypothesis_with_plain_weights(order):
    lex, lm, x, tr = rescue_case(np.float64)
    plain = beam_word_conf_ref(x, tr, lex, lm, None, 1)
    assert plain["words"][0, 0] == 0                                                # K = 1 without look-ahead: the poor word
    info = {}
    r = beam_word_conf_ref(x, tr, lex, lm, None, 1, order=order, info=info)
    la = beam_word_la_ref(x, tr, lex, lm, order, None, 1)
    for n in DECODE:
        assert np.array_equal(r[n], la[n]), n
    assert r["words"][0, 0] == 1 and r["sets"][0] == [list(k) for k in info["kept"][0]] != plain["sets"][0]
    Z = beam_word_la_loss_ref(x, tr, lex, lm, order, None, 1)[0]
    assert r["normalisers"][0] == Z[0] == beam_word_loss_ref(x, tr, lex, lm, None, 1, sets=lattice_sets_of(r, lex, lm, x, tr))[0][0]
    assert abs(r["word_confidences"][0, 0] - 1.0) < 1e-12 and r["word_frames"][0, 0] == 2
    best = beam_word_ref(x, tr, lex, lm, None, ALL)                                 # the plain score of that path
    assert abs(r["normalisers"][0] - best["scores"][0]) < 1e-12


def lattice_sets_of(r, lex, lm, x, tr):
    """A `lattice_sets` tuple with the sets of a restatement result in the place of the plain search's."""
    m, lens, A, F, _ = lattice_sets(x, tr, lex, lm, None, 1)
    return m, lens, A, F, r["sets"]


# ---------------------------------------------------------------------------------------------------------------- the C ABI
NAMES = ("asg_beam_words_confidence_work_bytes", "asg_beam_words_confidence", "asg_beam_words_confidence_la")


def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    assert "#define ASG_HIP_VERSION 230" in src and _lib.ABI_VERSION == 230


def test_work_bytes_are_the_stated_formula_and_have_no_term_in_the_lm():
    lex = small_lexicon()
    small, big = arpa_lm(5, 2, 1), arpa_lm(5, 3, 1, keep=(1.0, 1.0, 1.0))
    assert big.H > 2 * small.H and big.A > 2 * small.A
    al = lambda n: (n + 255) // 256 * 256                                                       # noqa: E731
    for dtype, e in ((torch.float32, 4), (torch.float64, 8)):
        for T, B, K, S in ((7, 3, 16, 0), (100, 2, 300, 40), (5, 1, 8, 9)):
            L, p, gb, w, keep = _abi(lex, small, T, B, dtype, S)                 # (S > 0: targets in the problem change nothing)
            L2, p2, gb2, w2, keep2 = _abi(lex, big, T, B, dtype, S)
            dec = int(L.asg_beam_decode_words_work_bytes(*_refs(p, gb, w), K))
            a = int(L.asg_beam_words_confidence_work_bytes(*_refs(p, gb, w), K))
            assert a == int(L2.asg_beam_words_confidence_work_bytes(*_refs(p2, gb2, w2), K)) > 0
            assert a == B * (dec // B + 2 * al(T * 4) + 256 + al(T * K * 8) + al(T * K * e) + al(2 * K * e))
            p.targets = None
            assert a == int(L.asg_beam_words_confidence_work_bytes(*_refs(p, gb, w), K))
            assert a == int(L.asg_beam_words_full_work_bytes(*_refs(p, gb, w), K, 1)) + B * al(2 * K * e)


def test_abi_argument_checks_without_a_device():
    from torch_asg_amd import _lib
    lex, lm = small_lexicon(), arpa_lm(5, 2, 1)
    for dtype, e in ((torch.float32, 4), (torch.float64, 8)):
        L, p, gb, w, keep = _abi(lex, lm, 7, 3, dtype, 0)
        wb = lambda K: int(L.asg_beam_words_confidence_work_bytes(*_refs(p, gb, w), K))              # noqa: E731
        mmax = (160 * 1024 - 256) // (16 + e)              # the pair loss's bound on M = K
        assert wb(min(mmax, 8192)) > 0 and wb(0) == 0 and wb(8193) == 0
        if mmax < 8192:
            assert wb(mmax + 1) == 0
        outs = ["scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths", "word_frames",
                "word_confidences", "normalisers"]

        def call(K=8, th=1.0, tol=0, work=256, nbytes=1 << 40, la=None, **null):
            ptrs = [None if n in null else 256 for n in outs]
            if la is not None:
                return L.asg_beam_words_confidence_la(None, *_refs(p, gb, w), la, K, th, tol, work, nbytes, *ptrs, 0, None)
            return L.asg_beam_words_confidence(None, *_refs(p, gb, w), K, th, tol, work, nbytes, *ptrs, 0, None)
        # the decoder's argument checks
        assert call(K=0) == 1 and call(th=-1.0) == 1 and call(th=float("nan")) == 1 and call(K=8193) == 2
        assert call(work=None) == 1
        for n in outs:
            assert call(**{n: None}) == 1, n
        # the tolerance
        assert call(tol=-1) == 1 and call(tol=65) == 2 and call(tol=-1, work=None) == 1
        # a workspace one byte short, before anything is launched
        assert call(nbytes=wb(8) - 1) == 3 and call(tol=64, nbytes=wb(8) - 1) == 3
        if mmax < 8192:
            assert call(K=mmax + 1) == 2
        w.dtype = 1 - w.dtype
        assert call() == 1 and wb(8) == 0
        w.dtype = 1 - w.dtype
        for field, bad in (("start", lm.H), ("separator", 5), ("H", 0), ("row", None), ("word_of_state", None)):
            old = getattr(w, field)
            setattr(w, field, bad)
            assert call() == 1, field
            setattr(w, field, old)
        w.H = (1 << 25) + 1
        assert call() == 2
        w.H = lm.H
        p.T = (1 << 20) + 1
        assert call() == 2 and wb(8) == 0
        p.T = 7
        # the look-ahead's checks, behind the decoder's
        look = _la(_lib, S=int(w.S), H=int(w.H), A=min(int(w.A), 4), levels=2, dtype=p.dtype)
        ref = ctypes.byref(look)
        assert call(la=ref, nbytes=wb(8) - 1) == 3 and call(la=ref, tol=65) == 2 and call(la=ref, K=0) == 1
        assert call(la=None, nbytes=wb(8) - 1) == 3
        assert L.asg_beam_words_confidence_la(None, *_refs(p, gb, w), None, 8, 1.0, 0, 256, 1 << 40, *([256] * 11), 0, None) == 1
        look.H += 1
        assert call(la=ref) == 1
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
    surfaces = (lambda *a, **k: A.beam_decode_words_confidence(x, tr, *a, **k),
                lambda lex_, lm_, **k: native().beam_decode_words_confidence(x, tr, lex_, lm_, None, k.pop("beam_size", 8), **k),
                lambda *a, **k: crit.beam_decode_words_confidence(x, *a, **k))
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
        A.beam_decode_words_confidence(x, tr, lex, lm, beam_size=0)
    with pytest.raises(ValueError, match="beam_threshold"):
        crit.beam_decode_words_confidence(x, lex, lm, beam_threshold=-1.0)
    for name in ("BeamWordsConfidence", "beam_decode_words_confidence"):
        assert name in A.__all__ and hasattr(A, name)
    assert A.BeamWordsConfidence._fields == A.BeamWords._fields + ("word_frames", "word_confidences", "normalisers")
