"""CPU tests of the n-best lists of the word-LM beam search WITH LM LOOK-AHEAD (`beam_decode_words_nbest(..., lookahead=)`,
`BeamWordStream._result_nbest` of a look-ahead stream, include/asg_hip.h::asg_beam_decode_words_nbest_la and
asg_beam_word_stream_nbest_la).  They pin tests/beam_word_la_nbest_ref.py, the yardstick of tests/test_hip_beam_word_la_nbest.py:
the bound that holds the three parts to the score (on the restatement alone, first), row 0 against the one-best restatements
with look-ahead, the whole list against the list without look-ahead where no sum rounds (every label path of T = 5, unpruned),
the prefix mode and the hand case its order is for, the rescue case, padding, short utterances and a beam without an end; then
the two C entry points' argument checks and the Python surface.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, eighths, small_lexicon
from beam_word_la_nbest_ref import BeamWordLaNbestStreamRef, beam_word_la_nbest_ref
from beam_word_la_ref import beam_word_la_ref
from beam_word_la_stream_ref import BeamWordLaStreamRef
from beam_word_nbest_cases import split_bound
from beam_word_nbest_ref import NAMES, beam_word_nbest_ref
from test_beam_word_la_cpu import LA_ARRAYS, _la, hand_case, rescue_case
from test_beam_word_la_stream_cpu import prefix_case
from test_beam_word_stream_abi import LM_ARRAYS, _graph, _lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
ALL = 1024
ONE_BEST = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths")
SCORES = [0.5, -1.0, 0.0, 2.0, -0.25]
DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
ORDERS = pytest.mark.parametrize("order", [1, 2, 3])
NEW = ("asg_beam_decode_words_nbest_la", "asg_beam_word_stream_nbest_la")


def _normal(T, B, N, seed, dt):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, B, N)).astype(dt), rng.standard_normal((N, N)).astype(dt)


def _eighths(T, B, N, seed, dt):
    rng = np.random.default_rng(seed)
    return (rng.integers(-32, 32, (T, B, N)) / 8.0).astype(dt), (rng.integers(-16, 16, (N, N)) / 8.0).astype(dt)


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


def _within_the_bound(res, dt):
    diff, bound, fin = split_bound(res, dt)
    assert (diff[fin] <= bound[fin]).all()
    return diff, fin


# ---------------------------------------------------------------------------------------------------------------- the bound, first
@DTYPES
@ORDERS
def test_the_restatement_keeps_the_three_parts_within_the_bound_of_the_score(order, dt):
    """Before anything else uses it.  With random weights the parts differ from `scores` in bits (the bound is not vacuous:
    something is there to bound); in eighths every sum is exact and they are equal."""
    lex = small_lexicon(SCORES)
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(9, 3, 5, 42, dt)
    il = np.array([9, 5, 1])
    res = beam_word_la_nbest_ref(x, tr, lex, lm, order, il, 64, 64, INF, 0.7, -0.4, 0.3)
    diff, fin = _within_the_bound(res, dt)
    assert fin.sum() > 40 and (diff[fin] > 0).sum() > 10
    plain = beam_word_nbest_ref(x, tr, lex, lm, il, 64, 64, INF, 0.7, -0.4, 0.3)
    assert (res["nterms"][fin] >= plain["nterms"][fin].min() + 2).all()      # the start pair's L at least, in and out
    pre = BeamWordLaNbestStreamRef(tr, lex, lm, order, 3, 9, 64, INF, 0.7, -0.4, 0.3, dt)
    pre.advance(x, il)
    diff, fin = _within_the_bound(pre.result_nbest(64, False), dt)      # prefixes: the open estimate is taken back by the end
    assert fin.sum() > 40 and (diff[fin] > 0).sum() > 10
    xe, te = _eighths(9, 3, 5, 43, dt)
    res = beam_word_la_nbest_ref(xe, te, lex, eighths(lm), order, il, 64, 64, INF, 1.0, 0.25, 0.125)
    diff, fin = _within_the_bound(res, dt)
    assert fin.sum() > 40 and (diff[fin] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- row 0
@DTYPES
@ORDERS
@pytest.mark.parametrize("lm_order", [2, 3], ids=["bigram", "trigram"])
def test_row_0_is_the_one_best_restatement_with_look_ahead_byte_for_byte(lm_order, order, dt):
    lex = small_lexicon(SCORES)
    lm = arpa_lm(5, lm_order, 60 + lm_order, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(7, 4, 5, 31, dt)
    il = np.array([7, 4, 1, 0])
    for K in (1, 3, 8, ALL):
        for theta in (INF, 2.0, 0.0):
            one = beam_word_la_ref(x, tr, lex, lm, order, il, K, theta, 0.7, -0.4, 0.3)
            for nbest in (1, 3):
                res = beam_word_la_nbest_ref(x, tr, lex, lm, order, il, K, nbest, theta, 0.7, -0.4, 0.3)
                for n in ONE_BEST:
                    assert res[n][:, 0].tobytes() == one[n].tobytes(), (n, K, theta)
                _padding_is_as_specified(res, nbest)
                _within_the_bound(res, dt)


# ---------------------------------------------------------------------------------------------------------------- property 4
@DTYPES
@ORDERS
@pytest.mark.parametrize("lm_kind", ["full", "sparse"])
def test_unpruned_and_in_eighths_the_list_is_the_list_without_look_ahead_bit_for_bit(lm_kind, order, dt):
    """All 3125 label paths of T = 5 are in the beam (K = all, no threshold), as in the enumeration of
    tests/test_beam_word_nbest_cpu.py; the plain list is held to that enumeration there.  Every weight is a multiple of 1/8, so
    the cancelling terms leave no rounding behind."""
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 3, 63, keep=(1.0, 1.0, 1.0) if lm_kind == "full" else (1.0, 0.5, 0.5)))
    x, tr = _eighths(5, 2, 5, 41, dt)
    il = np.array([5, 3])
    info = {}
    want = beam_word_nbest_ref(x, tr, lex, lm, il, ALL, ALL, INF, 1.0, 0.25, 0.125, info=info)
    got = beam_word_la_nbest_ref(x, tr, lex, lm, order, il, ALL, ALL, INF, 1.0, 0.25, 0.125)
    assert max(max(s) for s in info["sizes"]) < ALL and want["num_hyps"][0] > 20
    for n in NAMES:
        assert got[n].dtype == want[n].dtype and got[n].tobytes() == want[n].tobytes(), n
    _within_the_bound(got, dt)


# ---------------------------------------------------------------------------------------------------------------- prefix mode
@DTYPES
@ORDERS
def test_prefix_mode_row_0_is_the_streams_result(order, dt):
    lex = small_lexicon(SCORES)
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(5, 2, 5, 44, dt)
    kw = dict(lm_weight=0.7, word_score=-0.4, token_score=0.3)
    mid = 0
    for K in (1, 3, 8, ALL):
        a = BeamWordLaNbestStreamRef(tr, lex, lm, order, 2, 6, K, 2.0 if K == 3 else INF, dtype=dt, **kw)
        b = BeamWordLaStreamRef(tr, lex, lm, order, 2, 6, K, 2.0 if K == 3 else INF, dtype=dt, **kw)
        for chunk, cl in ((x[:2], None), (x[2:5], np.array([3, 1]))):
            a.advance(chunk, cl)
            b.advance(chunk, cl)
            for final in (False, True):
                res, one = a.result_nbest(4, final), b.result(final)
                for n in ONE_BEST + ("frames", "status"):
                    got = res[n] if n in ("frames", "status") else res[n][:, 0]
                    assert got.tobytes() == one[n].tobytes(), (n, K, final)
                _padding_is_as_specified(res, 4)
                if not final:                                # every kept pair is a row: e is finite for each
                    assert (res["num_cands"] == [len(s.A) for s in a.slots]).all()
                    wos = np.asarray(lex.word_of_state)
                    full = a.result_nbest(ALL, False)
                    for b_ in range(2):
                        last = full["states"][b_, :full["num_hyps"][b_], full["frames"][b_] - 1]
                        mid += int(((last != 0) & (wos[last] < 0)).sum())
    assert mid > 0                                           # some prefix rows end mid-word


@DTYPES
def test_the_prefix_list_orders_the_root_pair_before_the_mid_word_pair_with_the_largest_value(dt):
    lex, lm, x, tr, ws = prefix_case(dt)
    for order in (1, 2):
        a = BeamWordLaNbestStreamRef(tr, lex, lm, order, 1, 4, ALL, INF, 1.0, ws, 0.0, dt)
        a.advance(x)
        s = a.slots[0]
        (hv, qv), vmax = min(s.A, key=lambda it: (-it[1], it[0]))             # the largest v ...
        assert a.search.state[qv] != 0 and a.search.L(hv, qv) == 2.0            # ... is mid-word and carries + 2
        res = a.result_nbest(ALL, False)
        assert res["num_hyps"][0] == len(s.A) >= 2
        assert res["states"][0, 0, 3] == 0 and res["scores"][0, 0] == vmax - 1.0          # the root pair first
        r = [i for i in range(res["num_hyps"][0]) if res["path"][0, i, :4].tolist() == [0, 1, 3, 0]]
        assert len(r) == 1 and r[0] >= 1 and res["scores"][0, r[0]] == vmax - 2.0         # v - L behind it
        assert (np.diff(res["scores"][0, :res["num_hyps"][0]]) <= 0).all()
        # no look-ahead term in the parts: the plain list's rows for the same paths
        from beam_word_nbest_ref import BeamWordNbestStreamRef
        p = BeamWordNbestStreamRef(tr, lex, lm, 1, 4, ALL, INF, 1.0, ws, 0.0, dt)
        p.advance(x)
        want = p.result_nbest(ALL, False)
        for n in NAMES:
            assert res[n].tobytes() == want[n].tobytes(), n


# ---------------------------------------------------------------------------------------------------------------- rescue
def rescue_case_k2(dt):
    """5r's rescue (tests/test_beam_word_la_cpu.py::rescue_case) for a beam of TWO.  5r's two words share their first letter, so
    at K = 2 both children fit in the beam and nothing is there to rescue; a third word on the same letter makes K = 2 prune as
    K = 1 prunes there: the acoustics of the second letter slightly prefer the two words the LM dislikes.
    -> lexicon, LM, x [3, 1, 5], transition."""
    from torch_asg_amd import Lexicon, WordLM
    lex = Lexicon([[0, 1], [0, 2], [0, 3]], 5, 4)
    lm = WordLM(3, [0, 3], [0, 1, 2], [-5.0, -5.0, -1.0], [0, 0, 0], [-1], [0.0], 0, [0.0])
    x = np.full((3, 1, 5), -9.0, dt)
    x[0, 0, 0] = 0.0
    x[1, 0, 1], x[1, 0, 2], x[1, 0, 3] = 0.0, -0.25, -0.5
    x[2, 0, 4] = 0.0
    return lex, lm, x, np.zeros((5, 5), dt)


@DTYPES
def test_the_list_under_look_ahead_holds_the_word_the_lm_likes_and_the_plain_list_does_not(dt):
    """The LM here has one state, so every word that ends with its separator ends in ONE pair and the list keeps the best of
    them (recombination); the other rows end in word-end nodes."""
    def first_words(res):
        return [int(w) for w in res["words"][0, :res["num_hyps"][0], 0]]
    # 5r's case as it stands, K = 1: one row, the poor word without look-ahead, the unpruned best with it
    lex, lm, x, tr = rescue_case(dt)
    best = beam_word_nbest_ref(x, tr, lex, lm, None, ALL, 2, INF)
    assert first_words(best)[0] == 1
    plain = beam_word_nbest_ref(x, tr, lex, lm, None, 1, 2, INF)
    assert first_words(plain) == [0]
    for order in (1, 2):
        got = beam_word_la_nbest_ref(x, tr, lex, lm, order, None, 1, 2, INF)
        assert first_words(got) == [1]
        for n in ("scores", "emission_scores", "graph_scores", "lm_scores"):
            assert got[n][0, 0] == best[n][0, 0], n
    # ... and at K = 2
    lex, lm, x, tr = rescue_case_k2(dt)
    best = beam_word_nbest_ref(x, tr, lex, lm, None, ALL, 3, INF)
    assert first_words(best)[0] == 2
    info = {}
    plain = beam_word_nbest_ref(x, tr, lex, lm, None, 2, 3, INF, info=info)
    assert info["sizes"][0] == [1, 2, 2]
    assert plain["num_hyps"][0] == 2 and 2 not in first_words(plain)                # the liked word is not there
    for order in (1, 2):
        info = {}
        got = beam_word_la_nbest_ref(x, tr, lex, lm, order, None, 2, 3, INF, info=info)
        assert info["sizes"][0] == [1, 2, 2]
        assert got["num_hyps"][0] == 2 and first_words(got)[0] == 2
        for n in ("scores", "emission_scores", "graph_scores", "lm_scores"):
            assert got[n][0, 0] == best[n][0, 0], n


# ---------------------------------------------------------------------------------------------------------------- padding, lengths
@DTYPES
def test_padding_rows_lengths_0_and_1_and_a_beam_without_an_end(dt):
    from torch_asg_amd import Lexicon, WordLM
    lex = small_lexicon(SCORES)
    lm = arpa_lm(5, 2, 62, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(6, 3, 5, 45, dt)
    il = np.array([6, 1, 0])
    for K in (2, 6):
        for nbest in (1, 2, K, K + 5):
            res = beam_word_la_nbest_ref(x, tr, lex, lm, 2, il, K, nbest, INF, 0.7, -0.4, 0.3)
            assert res["scores"].shape == (3, nbest) and res["tokens"].shape == (3, nbest, 6)
            _padding_is_as_specified(res, nbest)
            _within_the_bound(res, dt)
            assert res["num_hyps"][2] == 0 and res["num_cands"][2] == 0
            assert (res["path"][1, :, 1:] == -1).all() and (res["token_lengths"][1, :res["num_hyps"][1]] == 1).all()
    assert beam_word_la_nbest_ref(x, tr, lex, lm, 2, il, 6, 6, INF)["num_hyps"][1] >= 2         # T = 1: several one-token words
    long = Lexicon([[0, 1, 0]], 3, 2)
    res = beam_word_la_nbest_ref(x[:2, :, :3], tr[:3, :3], long, WordLM.null(1), 1, None, 8, 3, INF)
    assert (res["num_hyps"] == 0).all() and (res["num_cands"] == 0).all()
    _padding_is_as_specified(res, 3)
    # a dead end (nothing below the node that the LM knows) and a rejected final word: neither is a row
    lex, lm = hand_case()
    x, tr = _normal(4, 2, 5, 46, dt)
    info = {}
    res = beam_word_la_nbest_ref(x, tr, lex, lm, 2, None, ALL, ALL, INF, info=info)
    wos = np.asarray(lex.word_of_state)
    for b in range(2):
        nh = int(res["num_hyps"][b])
        assert nh >= 2 and not (res["words"][b, :nh] == 4).any() and not (res["path"][b, :nh] == 3).any()
        assert (wos[res["states"][b, :nh, 3]] >= 0).all() or (res["states"][b, :nh, 3] == 0).any()


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    import torch_asg_amd as A
    import inspect
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"\bint %s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS, n
        plain = getattr(L, n[:-3]).argtypes
        at = plain.index(ctypes.POINTER(_lib.AsgWordLM)) + 1
        assert getattr(L, n).argtypes == plain[:at] + [ctypes.POINTER(_lib.AsgWordLookahead)] + plain[at:]
    assert int(L.asg_hip_version()) == 230 and "#define ASG_HIP_VERSION 230" in src       # additions only
    assert "Not there: look-ahead in" not in src
    for f in (A.beam_decode_words_nbest, A.ASGLoss.beam_decode_words_nbest):
        assert inspect.signature(f).parameters["lookahead"].default is None
    assert hasattr(A.BeamWordStream, "_result_nbest")


def _la_checks(call):
    """The look-ahead's own checks, exactly asg_beam_decode_words_la's; `call(ll=, n=)`, n the workspace bytes."""
    from torch_asg_amd import _lib
    F64 = _lib.ASG_DTYPE_F64
    assert call(ll=None) == 1 and call(ll=None, n=16) == 1
    assert call(ll=_la(_lib, dtype=F64)) == 1 and call(ll=_la(_lib, dtype=F64), n=16) == 1
    for a in LA_ARRAYS:
        m = _la(_lib)
        setattr(m, a, None)
        assert call(ll=m, n=16) == 1, a
    for kw in (dict(S=59999), dict(H=20000), dict(A=-1), dict(A=400001), dict(levels=0), dict(levels=32), dict(A=100, levels=8)):
        assert call(ll=_la(_lib, **kw), n=16) == 1, kw
    assert call(ll=_la(_lib, A=128, levels=8), n=16) == 3                           # a good one: on to the workspace
    empty = _la(_lib, A=0, levels=1)
    empty.krank = empty.tab = None
    assert call(ll=empty, n=16) == 3


def test_one_shot_argument_checks_without_a_device():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32, F64 = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64
    g, gb = _graph(_lib)
    w = _lm(_lib)
    la = _la(_lib)
    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.dtype = 8, 2, 40, F32
    p.inputs = p.transition = 256
    ref = lambda x: None if x is None else ctypes.byref(x)                          # noqa: E731
    wb = int(L.asg_beam_decode_words_nbest_work_bytes(ref(p), ref(gb), ref(w), 8, 4))
    assert wb > 0
    big = 1 << 50
    outs = (256,) * 12
    call = lambda K=8, th=1.0, nb=4, work=256, n=big, o=outs, lm=w, pp=p, gg=gb, ll=la: L.asg_beam_decode_words_nbest_la(      # noqa: E731
        None, ref(pp), ref(gg), ref(lm), ref(ll), K, th, nb, work, n, *o, 0, None)
    plain = lambda n: L.asg_beam_decode_words_nbest(None, ref(p), ref(gb), ref(w), 8, 1.0, 4, 256, n, *outs, 0, None)  # noqa: E731
    # one workspace function serves both forms: both refuse one byte less than it returns
    assert call(n=wb - 1) == 3 and plain(wb - 1) == 3 and call(n=16) == 3
    # the plain call's checks
    assert call(nb=0) == 1 and call(nb=-1) == 1 and call(nb=8193) == 2
    assert call(K=0) == 1 and call(K=8193) == 2 and call(th=-1.0) == 1 and call(th=float("nan")) == 1 and call(work=None) == 1
    assert call(pp=None) == 1 and call(gg=None) == 1 and call(lm=None) == 1
    assert call(lm=_lm(_lib, H=(1 << 25) + 1), ll=_la(_lib, H=(1 << 25) + 1)) == 2
    for name in LM_ARRAYS:
        m = _lm(_lib)
        setattr(m, name, None)
        assert call(lm=m) == 1, name
    optional = {4, 7, 8}                                             # path, states, lm_states may be NULL
    for i in range(12):
        assert call(o=outs[:i] + (None,) + outs[i + 1:], n=16) == (3 if i in optional else 1), i
    _la_checks(lambda ll, n=big: call(ll=ll, n=n))
    p.dtype = F64
    assert call() == 1                                               # not the graph's dtype
    p.dtype = F32


def test_stream_argument_checks_without_a_device():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32 = _lib.ASG_DTYPE_F32
    g, gb = _graph(_lib)
    w = _lm(_lib)
    la = _la(_lib)
    ref = lambda x: None if x is None else ctypes.byref(x)                          # noqa: E731
    sb = int(L.asg_beam_word_stream_state_bytes(ref(gb), ref(w), 2, F32, 8, 10))
    wb = int(L.asg_beam_word_stream_nbest_work_bytes(ref(gb), ref(w), 2, F32, 8, 10, 4))
    assert sb > 0 and wb > 0
    big = 1 << 50
    outs = (256,) * 13
    call = lambda K=8, B=2, M=10, state=256, n=big, nb=4, work=256, wn=big, o=outs, lm=w, gg=gb, ll=la, fin=1: (       # noqa: E731
        L.asg_beam_word_stream_nbest_la(None, ref(gg), ref(lm), ref(ll), B, K, M, state, n, fin, nb, work, wn, *o, 0, None))
    plain = lambda wn: L.asg_beam_word_stream_nbest(None, ref(gb), ref(w), 2, 8, 10, 256, big, 1, 4, 256, wn, *outs, 0, None)  # noqa: E731
    assert call(wn=wb - 1) == 3 and plain(wb - 1) == 3 and call(n=sb - 1) == 3 and call(wn=wb - 1, fin=0) == 3
    assert call(nb=0) == 1 and call(nb=8193) == 2 and call(K=0) == 1 and call(K=8193) == 2 and call(M=0) == 1 and call(B=0) == 1
    assert call(state=None) == 1 and call(work=None) == 1 and call(gg=None) == 1 and call(lm=None) == 1
    for name in LM_ARRAYS:
        m = _lm(_lib)
        setattr(m, name, None)
        assert call(lm=m) == 1, name
    optional = {3, 6, 7}                                             # path, states, lm_states may be NULL
    for i in range(13):
        assert call(o=outs[:i] + (None,) + outs[i + 1:], wn=16) == (3 if i in optional else 1), i
    _la_checks(lambda ll, n=big: call(ll=ll, wn=n))


# ---------------------------------------------------------------------------------------------------------------- Python
def test_python_surface_refuses_a_wrong_look_ahead_before_the_device_check():
    import torch_asg_amd as A
    from torch_asg_amd import asg
    lex, lm = hand_case()
    la = A.WordLookahead(lex, lm, 2)
    x, tr = torch.zeros(5, 2, 5), torch.zeros(5, 5)
    loss = A.ASGLoss(5)
    calls = (lambda lx, m, **kw: A.beam_decode_words_nbest(x, tr, lx, m, beam_size=4, nbest=2, **kw),
             lambda lx, m, **kw: loss.beam_decode_words_nbest(x, lx, m, beam_size=4, nbest=2, **kw),
             lambda lx, m, **kw: asg.native().beam_decode_words_nbest(x, tr, lx, m, None, 4, 2, **kw))
    other = A.Lexicon([[0], [1]], 5, 4)
    same_shape = A.Lexicon([[0], [0, 1], [1], [2], [3, 0]], 5, 4)                   # equal S, another object
    for call in calls:
        with pytest.raises(TypeError, match="lookahead"):
            call(lex, lm, lookahead=lm)
        for lx, m in ((other, lm), (same_shape, lm), (lex, hand_case()[1]), (lex, A.WordLM.null(6))):
            with pytest.raises(RuntimeError, match="built for"):       # (CPU tensors: the device check would say "no CPU")
                call(lx, m, lookahead=la)
        with pytest.raises(RuntimeError):
            call(lex, lm, lookahead=la)                                # CPU tensors: there is no CPU implementation
        with pytest.raises(RuntimeError):
            call(lex, lm, lookahead=None)
    with pytest.raises(ValueError, match="nbest"):
        A.beam_decode_words_nbest(x, tr, lex, lm, beam_size=4, nbest=0, lookahead=la)
    # the private stream method is the public one's body: the same ValueError, no device needed to reach it
    s = object.__new__(A.BeamWordStream)
    s.lookahead = la
    with pytest.raises(ValueError, match="nbest"):
        s._result_nbest(0, False, False)
    with pytest.raises(NotImplementedError, match="look-ahead"):
        s.result_nbest(2)
