"""CPU tests of LM look-ahead in the two word streams (`BeamWordStream(..., lookahead=)`, `BeamWordWindowStream(..., lookahead=)`,
include/asg_hip.h::asg_beam_word_stream_advance_la): the restatements with explicit carried state
(tests/beam_word_la_stream_ref.py) against the one-shot restatement with look-ahead (tests/beam_word_la_ref.py) for every
chunking, and against the streams without look-ahead where the prefix rule says the two agree; the hand case the prefix rule is
for; the window's search identity, exactness and forced commit; the four C entry points' argument checks and the Python
surface.  Every regime is asserted from the restatement's own records first -- no kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, eighths, integers, small_lexicon
from beam_word_la_ref import beam_word_la_ref
from beam_word_la_stream_ref import BeamWordLaStreamRef, BeamWordLaWindowRef
from beam_word_stream_ref import NAMES as STREAM_NAMES, BeamWordStreamRef
from beam_word_window_ref import RESULT
from test_beam_word_la_cpu import LA_ARRAYS, _emissions, _la, hand_case
from test_beam_word_stream_abi import LM_ARRAYS, _graph, _lm
from test_beam_word_window_cpu import check_exact, chunkings, run, same_results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
ONE_SHOT = STREAM_NAMES[:8]
ALL = 1024
SCORES = [0.5, -1.0, 0.0, 2.0, -0.25]
LA_CALLS = ("asg_beam_word_stream_advance_la", "asg_beam_word_stream_result_la", "asg_beam_word_window_advance_la",
            "asg_beam_word_window_result_la")


def feed(s, x, il, cuts):
    """Advance by the chunks x[t0:t1], slot b taking the frames below il[b]."""
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        s.advance(x[t0:t1], np.clip(il - t0, 0, t1 - t0))


def all_chunkings(T, rng):
    yield "frames", list(range(T + 1))
    yield from chunkings(T, rng)                           # one chunk, and random cuts with chunks of no frames


# ---------------------------------------------------------------------------------------------------------------- 1. the stream
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("weights", ["eighths", "integers"])
@pytest.mark.parametrize("lm_order", [2, 3], ids=["bigram", "trigram"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_any_chunking_gives_the_one_shot_look_ahead_decode(order, lm_order, weights, dt):
    lex = small_lexicon(SCORES)
    lm = (eighths if weights == "eighths" else integers)(arpa_lm(5, lm_order, 60 + lm_order, keep=(1.0, 0.5, 0.5)))
    T, B = 8, 4
    x, tr = _emissions(T, B, 5, 35 + order, dt)
    if weights == "integers":
        x, tr = np.round(x), np.round(tr)
    il = np.array([T, 5, 1, 0])
    rng = np.random.default_rng(5 + order)
    pruned = 0
    for K in (1, 3, 8, ALL):
        for theta in (INF, 2.0, 0.0):
            info = {}
            want = beam_word_la_ref(x, tr, lex, lm, order, il, K, theta, 0.75, -0.5, 0.25, info=info)
            pruned += any(len(k) < c for ks, cs in zip(info["kept"], info["cands"]) for k, c in zip(ks, cs))
            for name, cuts in all_chunkings(T, rng):
                s = BeamWordLaStreamRef(tr, lex, lm, order, B, T, K, theta, 0.75, -0.5, 0.25, dt)
                feed(s, x, il, cuts)
                got = s.result(True)
                for n in ONE_SHOT:
                    assert got[n].dtype == want[n].dtype and got[n].tobytes() == want[n].tobytes(), (n, K, theta, name)
                assert got["frames"].tolist() == il.tolist() and not got["status"].any()
                assert s.kept() == info["kept"] and s.sizes() == info["sizes"] and s.cands() == info["cands"], (K, theta, name)
    assert pruned > 0


# ---------------------------------------------------------------------------------------------------------------- 2. the prefix, unpruned
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_unpruned_the_prefix_is_the_plain_streams_bit_for_bit(order, dt):
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 3, 43))
    T, B = 8, 4
    x, tr = _emissions(T, B, 5, 35, dt)
    il = np.array([T, 5, 1, 0])
    rng = np.random.default_rng(6)
    mid = 0
    for name, cuts in all_chunkings(T, rng):
        plain = BeamWordStreamRef(tr, lex, lm, B, T, ALL, INF, 1.0, 0.25, 0.125, dt)
        s = BeamWordLaStreamRef(tr, lex, lm, order, B, T, ALL, INF, 1.0, 0.25, 0.125, dt)
        assert s.dead == 0
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            n = np.clip(il - t0, 0, t1 - t0)
            plain.advance(x[t0:t1], n)
            s.advance(x[t0:t1], n)
            want, got = plain.result(False), s.result(False)
            for k in STREAM_NAMES:
                assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, name, t1)
            assert s.kept() == plain.kept()
            for b in range(B):                             # prefixes that end mid-word: the estimate had to be taken back
                L = int(got["frames"][b])
                mid += L > 0 and got["states"][b, L - 1] != 0 and s.look.L(int(got["lm_states"][b, L - 1]),
                                                                             int(got["states"][b, L - 1])) != 0
        assert max(max(z) for z in s.sizes() if z) < ALL
    assert mid > 0


# ---------------------------------------------------------------------------------------------------------------- 3. the prefix rule matters
def prefix_case(dt):
    """Two words [0, 1] and [0, 2] under a unigram whose folded weights are positive (word_score 3): after the frames 0 1 3 the
    path is at the root; frame 3 either stays there (emission 0) or enters node [0] (emission -1, look-ahead +2).  The mid-word
    pair then holds the largest value, s + 1 against s, and the smaller prefix score, s - 1.
    -> lexicon, LM, x [4, 1, 4], transition, word_score."""
    from torch_asg_amd import Lexicon, WordLM
    lex = Lexicon([[0, 1], [0, 2]], 4, 3)
    lm = WordLM(2, [0, 2], [0, 1], [-1.0, -1.0], [0, 0], [-1], [0.0], 0, [0.0])
    x = np.full((4, 1, 4), -9.0, dt)
    x[0, 0, 0] = x[1, 0, 1] = x[2, 0, 3] = 0.0
    x[3, 0, 3], x[3, 0, 0] = 0.0, -1.0
    return lex, lm, x, np.zeros((4, 4), dt), 3.0


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_prefix_is_ranked_without_the_estimate_it_still_carries(dt):
    lex, lm, x, tr, ws = prefix_case(dt)
    for order in (1, 2):
        s = BeamWordLaStreamRef(tr, lex, lm, order, 1, 4, ALL, INF, 1.0, ws, 0.0, dt)
        s.advance(x)
        A = s.slots[0].A
        (hv, qv), vmax = min(A, key=lambda it: (-it[1], it[0]))                 # "largest v"
        assert s.state[qv] != 0 and s.L(hv, qv) == 2.0                          # ... is mid-word and carries + 2
        e, (h, q), _ = s.winner(A, False)
        assert s.state[q] == 0 and (h, q) != (hv, qv) and e == vmax - 1.0 and e > vmax - s.L(hv, qv)
        got = s.result(False)
        assert got["scores"][0] == e and got["path"][0].tolist() == [0, 1, 3, 3] and got["words"][0].tolist() == [0, -1, -1, -1]
        plain = BeamWordStreamRef(tr, lex, lm, 1, 4, ALL, INF, 1.0, ws, 0.0, dt)
        plain.advance(x)
        want = plain.result(False)
        for k in STREAM_NAMES:
            assert got[k].tobytes() == want[k].tobytes(), k
        # the window's forced commit follows the same pair: W = 2, P = 1 forces at every frame from the second on
        w = BeamWordLaWindowRef(tr, lex, lm, order, 1, 2, 1, ALL, INF, 1.0, ws, 0.0, dt)
        w.advance(x)
        assert w.slots[0].forced[-1] == ((h, q), (hv, qv)) and w.result(False)["scores"][0] == e


# ---------------------------------------------------------------------------------------------------------------- 4. the window
WP = [(1, 1), (2, 1), (5, 3), (5, 5), (16, 3), (16, 16)]


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_window_scores_commits_and_chunk_invariance(order, dt):
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5)))
    T, B = 12, 4
    x, tr = _emissions(T, B, 5, 11 + order, dt)
    il = np.array([T, 0, 1, 7])
    rng = np.random.default_rng(79)
    LW, WS, TS = 0.75, 2.5, 0.25                           # (a positive word score: L > 0, so that v and v - L rank apart)
    exact = forced = differ = turn = 0
    for K in (1, 3, 8, ALL):
        for theta in (INF, 2.0):
            one = beam_word_la_ref(x, tr, lex, lm, order, il, K, theta, LW, WS, TS)
            un = BeamWordLaStreamRef(tr, lex, lm, order, B, T, K, theta, LW, WS, TS, dt)
            un.advance(x, il)
            assert un.result(True)["scores"].tobytes() == one["scores"].tobytes()
            cks = list(all_chunkings(T, rng))
            for W, P in WP:
                what = "K=%d theta=%s W=%d P=%d" % (K, theta, W, P)
                s = BeamWordLaWindowRef(tr, lex, lm, order, B, W, P, K, theta, LW, WS, TS, dt)
                cat, trace, _ = run(s, x, il, list(range(T + 1)))
                at = dict(trace)
                res = s.result(True)
                assert res["scores"].tobytes() == one["scores"].tobytes(), what
                assert s.result(False)["scores"].tobytes() == un.result(False)["scores"].tobytes(), what
                exact += check_exact(cat, res, one, il, what)
                forced += int((res["status"] & 1).sum())
                differ += sum(a != b for v in s.slots for a, b in getattr(v, "forced", []))
                if W - P >= T:
                    assert not (res["status"] & 1).any(), what
                cname, cuts = cks[turn % len(cks)]
                turn += 1
                r = BeamWordLaWindowRef(tr, lex, lm, order, B, W, P, K, theta, LW, WS, TS, dt)
                cat2, trace2, _ = run(r, x, il, cuts)
                for t1, state in trace2:
                    if t1:
                        assert state == at[t1], (what, cname, t1)
                assert cat2 == cat and same_results(r.result(True), res) and same_results(r.result(False), s.result(False)), \
                    (what, cname)
    assert exact > 50 and forced > 0 and differ > 0        # ... and some forced commit followed another pair than "largest v"


def forced_case(dt):
    """The grid's lexicon under a trigram with a positive word score, T = 12, W = 4, P = 2 (W - P < T: the window must force),
    K = 3.  -> lexicon, LM, x, transition, (lm_weight, word_score, token_score)"""
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5)))
    x, tr = _emissions(12, 1, 5, 13, dt)
    return lex, lm, x, tr, (0.75, 2.5, 0.25)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_forced_commit_follows_the_prefix_pair_of_the_rule(dt):
    lex, lm, x, tr, fold = forced_case(dt)
    T, W, P = 12, 4, 2
    assert W - P < T
    il = np.array([T])
    outs = []
    for cuts in ([0, T], list(range(T + 1)), [0, 0, 3, 3, 8, T]):
        s = BeamWordLaWindowRef(tr, lex, lm, 2, 1, W, P, 3, INF, *fold, dt)
        cat, _, _ = run(s, x, il, cuts)
        v = s.slots[0]
        assert v.status & 1 and any(F > 0 for _, _, _, F in v.attempts)         # the case forces
        assert any(a != b for a, b in v.forced)                                 # ... along another pair than the largest v
        outs.append((cat, {(f, n): s.result(f)[n].tobytes() for f in (False, True) for n in RESULT}, v.forced, v.commits))
    assert outs[0] == outs[1] == outs[2]
    un = BeamWordLaStreamRef(tr, lex, lm, 2, 1, T, 3, INF, *fold, dt)
    un.advance(x)
    for f in (False, True):                                # the ring cannot alter a score, forced or not
        assert s.result(f)["scores"].tobytes() == un.result(f)["scores"].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 5. the C ABI
def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in LA_CALLS:
        assert re.search(r"\bint %s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS, n
        plain = getattr(L, n[:-3]).argtypes
        assert len(getattr(L, n).argtypes) == len(plain) + 1
    assert int(L.asg_hip_version()) == 230 and "#define ASG_HIP_VERSION 230" in src       # additions only


def test_abi_argument_checks_without_a_device():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32, F64 = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64
    g, gb = _graph(_lib)
    w = _lm(_lib)
    la = _la(_lib)
    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.dtype = 4, 2, 40, F32
    p.inputs = p.transition = 256
    big = 1 << 50
    ref = lambda x: None if x is None else ctypes.byref(x)                          # noqa: E731
    sb = int(L.asg_beam_word_stream_state_bytes(ref(gb), ref(w), 2, F32, 8, 10))
    wb = int(L.asg_beam_word_window_state_bytes(ref(gb), ref(w), 2, F32, 8, 10, 3))
    assert sb > 0 and wb > 0
    o10, o8, o11 = (256,) * 10, (256,) * 8, (256,) * 11
    calls = {
        "s_adv": lambda K=8, th=1.0, state=256, n=big, lm=w, pp=p, gg=gb, ll=la, o=(): L.asg_beam_word_stream_advance_la(
            None, ref(pp), ref(gg), ref(lm), ref(ll), K, th, 10, state, n, 0, None),
        "s_res": lambda K=8, th=None, state=256, n=big, lm=w, pp=p, gg=gb, ll=la, o=o10: L.asg_beam_word_stream_result_la(
            None, ref(gg), ref(lm), ref(ll), 2, K, 10, state, n, 0, *o, 0, None),
        "w_adv": lambda K=8, th=1.0, state=256, n=big, lm=w, pp=p, gg=gb, ll=la, o=o8: L.asg_beam_word_window_advance_la(
            None, ref(pp), ref(gg), ref(lm), ref(ll), K, th, 10, 3, state, n, *o, 0, None),
        "w_res": lambda K=8, th=None, state=256, n=big, lm=w, pp=p, gg=gb, ll=la, o=o11: L.asg_beam_word_window_result_la(
            None, ref(gg), ref(lm), ref(ll), 2, K, 10, 3, state, n, 1, *o, 0, None),
    }
    for name, call in calls.items():
        need = sb if name[0] == "s" else wb
        # a good look-ahead gets as far as the state's size: one byte less is refused there, like the plain call
        assert call(n=need - 1) == 3 and call(n=16) == 3, name
        # the plain call's own checks
        assert call(K=0) == 1 and call(K=8193) == 2 and call(state=None) == 1 and call(gg=None) == 1 and call(lm=None) == 1, name
        if name.endswith("adv"):
            assert call(th=-1.0) == 1 and call(th=float("nan")) == 1 and call(pp=None) == 1, name
        for a in LM_ARRAYS:
            m = _lm(_lib)
            setattr(m, a, None)
            assert call(lm=m) == 1, (name, a)
        outs = call.__defaults__[-1]
        for i in range(len(outs)):
            assert call(o=outs[:i] + (None,) + outs[i + 1:]) == 1, (name, i)
        # the look-ahead's own, exactly asg_beam_decode_words_la's
        assert call(ll=None) == 1 and call(ll=None, n=16) == 1, name
        assert call(ll=_la(_lib, dtype=F64)) == 1 and call(ll=_la(_lib, dtype=F64), n=16) == 1, name
        for a in LA_ARRAYS:
            m = _la(_lib)
            setattr(m, a, None)
            assert call(ll=m, n=16) == 1, (name, a)
        for kw in (dict(S=59999), dict(H=20000), dict(A=-1), dict(A=400001), dict(levels=0), dict(levels=32), dict(A=100, levels=8)):
            assert call(ll=_la(_lib, **kw), n=16) == 1, (name, kw)
        assert call(ll=_la(_lib, A=128, levels=8), n=16) == 3, name
        empty = _la(_lib, A=0, levels=1)
        empty.krank = empty.tab = None
        assert call(ll=empty, n=16) == 3, name
    # the window's own shape checks
    assert L.asg_beam_word_window_advance_la(None, ref(p), ref(gb), ref(w), ref(la), 8, 1.0, 10, 11, 256, big, *o8, 0, None) == 1
    assert L.asg_beam_word_window_result_la(None, ref(gb), ref(w), ref(la), 2, 8, 0, 1, 256, big, 1, *o11, 0, None) == 1
    # no frames: the stream's advance returns before a launch, the look-ahead checked all the same
    p.T = 0
    assert calls["s_adv"]() == 0 and calls["s_adv"](ll=None) == 1
    p.T, p.dtype = 4, F64
    assert calls["s_adv"]() == 1 and calls["w_adv"]() == 1                          # not the graph's dtype
    p.dtype = F32


# ---------------------------------------------------------------------------------------------------------------- 6. Python
def test_python_surface_refuses_a_wrong_look_ahead_before_any_device_work():
    import torch_asg_amd as A
    lex, lm = hand_case()
    la = A.WordLookahead(lex, lm, 2)
    tr = torch.zeros(5, 5)
    other = A.Lexicon([[0], [1]], 5, 4)
    same_shape = A.Lexicon([[0], [0, 1], [1], [2], [3, 0]], 5, 4)
    loss = A.ASGLoss(5)
    makers = (lambda lx, m, **kw: A.BeamWordStream(tr, lx, m, 2, 10, beam_size=4, **kw),
              lambda lx, m, **kw: A.BeamWordWindowStream(tr, lx, m, 2, 8, 2, beam_size=4, **kw),
              lambda lx, m, **kw: loss.beam_word_stream(lx, m, 2, 10, beam_size=4, **kw),
              lambda lx, m, **kw: loss.beam_word_window_stream(lx, m, 2, 8, beam_size=4, **kw))
    for make in makers:
        with pytest.raises(TypeError, match="lookahead"):
            make(lex, lm, lookahead=lm)
        for lx, m in ((other, lm), (same_shape, lm), (lex, hand_case()[1]), (lex, A.WordLM.null(6))):
            with pytest.raises(RuntimeError, match="built for"):       # (a CPU transition: the device check would say "no CPU")
                make(lx, m, lookahead=la)
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            make(lex, lm, lookahead=la)
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            make(lex, lm, lookahead=None)


def test_result_nbest_of_a_look_ahead_stream_fails_before_any_launch_and_the_state_has_one_size():
    import torch_asg_amd as A
    from torch_asg_amd import _lib
    lex, lm = hand_case()
    la = A.WordLookahead(lex, lm, 2)
    s = object.__new__(A.BeamWordStream)                   # (no device here: the attributes the check reads, nothing else)
    s.lookahead = la
    with pytest.raises(NotImplementedError, match="look-ahead"):
        s.result_nbest(0)                                  # before the ValueError of nbest < 1, before any library call
    s.lookahead = None
    with pytest.raises(ValueError):
        s.result_nbest(0)
    # a stream with a look-ahead sizes and resets its state through the plain entry points: there is no _la form of either
    L = _lib.lib()
    for api in ("asg_beam_word_stream", "asg_beam_word_window"):
        for sfx in ("_state_bytes", "_reset"):
            assert hasattr(L, api + sfx) and (api + sfx + "_la") not in _lib.SYMBOLS
    for cls in (A.BeamWordStream, A.BeamWordWindowStream):
        assert cls._look == () and cls.lookahead is None   # without the keyword: the plain calls, nothing behind the LM view
