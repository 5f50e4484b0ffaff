"""GPU tests (-m gpu) of LM look-ahead in the windowed lexicon + word-LM stream (`BeamWordWindowStream(..., lookahead=)`,
csrc/asg_beam_word_window.hip compiled with the look-ahead flag): the bytes of every commit output of every `advance` and of
every `result`, final and prefix, against the test-side restatement (tests/beam_word_la_stream_ref.py::BeamWordLaWindowRef, pinned
on the CPU by tests/test_beam_word_la_stream_cpu.py), the scores against the device's own `beam_decode_words(..., lookahead=)`,
and committed + tail against its transcript.  Every case first asserts its regime from the restatement's records."""
import numpy as np
import pytest
import torch

import test_beam_word_window_cpu as cpu
import test_hip_beam_word_window as plain
from beam_word_cases import arpa_lm, eighths, small_lexicon
from beam_word_la_stream_ref import BeamWordLaWindowRef
from beam_word_window_ref import COMMIT, RESULT
from test_beam_word_la_stream_cpu import forced_case
from test_hip_beam_word_stream import grid_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
ALL = 1024
LW, WS, TS = cpu.LW, cpu.WS, cpu.TS
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
NP = {torch.float32: np.float32, torch.float64: np.float64}
ONE = plain.ONE
SEED_BOUNDARY = 3                                          # (a seed at which the restatement shows the regime, order 2)


def _asg():
    import torch_asg_amd
    return torch_asg_amd


class Both(plain.Both):
    """The device window stream with a look-ahead and its restatement, driven by the same calls; every output compared."""

    def __init__(self, tr, lex, lm, la, B, W, P, K, theta=INF, lw=LW, ws=WS, ts=TS):
        self.dev = _asg().BeamWordWindowStream(tr.to(DEV), lex, lm, B, W, P, K, theta, lw, ws, ts, tr.dtype, DEV, lookahead=la)
        self.ref = BeamWordLaWindowRef(tr.numpy(), lex, lm, la.order, B, W, P, K, theta, lw, ws, ts, NP[tr.dtype])
        self.B, self.W = B, W
        self.cat = [tuple([] for _ in cpu.WIDE) for _ in range(B)]


def _gpu_one_shot(x, tr, lex, lm, la, il, K, theta=INF, lw=LW, ws=WS, ts=TS):
    out = _asg().beam_decode_words(x.to(DEV), tr.to(DEV), lex, lm, None if il is None else il.to(DEV), K, theta, lw, ws, ts,
                                   lookahead=la)
    return {n: o.cpu().numpy() for n, o in zip(ONE, out)}


# ---------------------------------------------------------------------------------------------------------------- 1. the grid
@DTYPES
@pytest.mark.parametrize("order", [1, 2, 3])
def test_every_output_of_every_call_equals_the_restatement(order, dtype):
    lex, lm, x, tr, il = grid_case(3, dtype)
    la = _asg().WordLookahead(lex, lm, order)
    T, B = 12, 4
    turn = order
    exact = forced = words = 0
    for K in (1, 3, 8, ALL):
        for theta in (INF, 2.0):
            one = _gpu_one_shot(x, tr, lex, lm, la, il, K, theta)
            for W, P in ((4, 1), (8, 4), (32, 8)):
                cuts = ([0, T], list(range(T + 1)), [0, 1, 5, 5, 12], [0, 0, 7, 12, 12])[turn % 4]
                turn += 1
                what = "order=%d K=%d theta=%s W=%d P=%d cuts %s" % (order, K, theta, W, P, cuts)
                s = Both(tr, lex, lm, la, B, W, P, K, theta)
                res = s.feed(x, il, cuts, what, results=True)
                assert res[True]["scores"].tobytes() == one["scores"].tobytes(), what
                exact += cpu.check_exact(s.cat, res[True], one, il.numpy(), what)
                forced += int((res[True]["status"] & 1).sum())
                words += sum(len(c[4]) for c in s.cat)
                if W - P >= T:
                    assert not (res[True]["status"] & 1).any(), what
    assert exact > 0 and words > 0 and forced > 0


# ---------------------------------------------------------------------------------------------------------------- 2. words
def test_a_separator_edge_on_a_commit_boundary_and_on_a_call_boundary():
    A = _asg()
    for one_call in (True, False):
        lex, lm, x, tr, il = cpu.word_case(SEED_BOUNDARY)
        la = A.WordLookahead(lex, lm, 2)
        x, tr, il = torch.from_numpy(x), torch.from_numpy(tr), torch.from_numpy(il)
        s = Both(tr, lex, lm, la, 1, 8, 2, 3, INF)
        T = int(il[0])
        calls = []
        for t0, t1 in ((0, T),) if one_call else zip(range(T), range(1, T + 1)):
            base = s.ref.slots[0].base
            got = s.advance(x[t0:t1], None, "boundary %d:%d" % (t0, t1))
            calls.append((base, int(got["frames"][0])))
            s.results("boundary after %d" % t1)
        v = s.ref.slots[0]
        starts = [f0 for f0, _ in v.commits if f0 in cpu.edge_frames(s.cat[0][0])]
        assert v.status == 0 and starts                    # the regime: a segment begins with the separator of an edge
        if one_call:
            assert len(v.commits) > 1 and min(starts) > v.commits[0][0]       # ... behind an earlier segment of the same call
        else:
            assert [b for b, n in calls if n and b in starts]                  # ... as the first frame that a call commits
        one = _gpu_one_shot(x, tr, lex, lm, la, il, 3)
        assert cpu.check_exact(s.cat, s.results("boundary")[True], one, il.numpy(), "boundary") == 1
        assert len(s.cat[0][4]) >= len(starts)


# ---------------------------------------------------------------------------------------------------------------- 3. the window
@DTYPES
def test_a_forced_commit_follows_the_best_prefix_by_value_minus_look_ahead(dtype):
    lex, lm, x, tr, fold = forced_case(NP[dtype])
    la = _asg().WordLookahead(lex, lm, 2)
    x, tr = torch.from_numpy(x), torch.from_numpy(tr)
    T, W, P = 12, 4, 2
    ends = []
    for cuts in ([0, 5, 6, T], list(range(T + 1))):
        s = Both(tr, lex, lm, la, 1, W, P, 3, INF, *fold)
        ends.append((s.feed(x, None, cuts, "forced", results=True), s.cat))
        v = s.ref.slots[0]
        assert v.status == 1 and sum(F for _, _, _, F in v.attempts) > 0        # the regime: the window forces,
        assert any(a != b for a, b in v.forced)                                 # ... along another pair than the largest v
    assert ends[0][1] == ends[1][1]
    for final in (False, True):
        plain._same(ends[0][0][final], ends[1][0][final], "forced, two chunkings", RESULT)
    assert ends[0][0][True]["scores"].tobytes() == _gpu_one_shot(x, tr, lex, lm, la, None, 3, INF, *fold)["scores"].tobytes()


def test_dozens_of_wraps_with_one_slot():
    lex = small_lexicon(cpu.SCORES)
    lm = eighths(arpa_lm(5, 2, 62, keep=(1.0, 1.0)))
    la = _asg().WordLookahead(lex, lm, 2)
    T, W = 200, 4
    x, tr, _ = plain._np_case(T, 1, 5, 61, torch.float32)
    for P in (1, 4):
        s = Both(tr, lex, lm, la, 1, W, P, 1)
        res = s.feed(x, None, list(range(0, T, 37)) + [T], "K=1 P=%d" % P)
        v = s.ref.slots[0]
        assert v.status == 0 and v.pos == T > 40 * W and v.base == v.pos // P * P
        one = _gpu_one_shot(x, tr, lex, lm, la, None, 1)
        assert one["scores"][0] > -INF and cpu.check_exact(s.cat, res[True], one, np.array([T]), "wraps") == 1
        assert len(s.cat[0][4]) > 10                       # dozens of words committed


def test_capture_and_replay():
    lex = small_lexicon(cpu.SCORES)
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    la = _asg().WordLookahead(lex, lm, 2)
    Tc, B, N, K, theta, W, P = 4, 3, 5, 12, 6.0, 6, 3
    T = 3 * Tc
    x, tr, _ = plain._np_case(T, B, N, 53, torch.float32)
    il = torch.tensor([T, 9, T - 2])
    s = Both(tr, lex, lm, la, B, W, P, K, theta)
    buf = torch.zeros(Tc, B, N, device=DEV)
    n = torch.zeros(B, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.dev.advance(buf, n)                                        # warm-up; n = 0: the state stays as it is
        s.dev.result()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        new = s.dev.advance(buf, n)
        tail = s.dev.result(False)
    s.dev.reset()                                                    # (the capture itself ran nothing)
    for c in range(3):
        buf.copy_(x[c * Tc:(c + 1) * Tc])
        cn = (il - c * Tc).clamp(0, Tc)
        n.copy_(cn)
        gr.replay()
        torch.cuda.synchronize()
        want = dict(zip(COMMIT, s.ref.advance(x[c * Tc:(c + 1) * Tc].numpy(), cn.numpy())))
        plain._same({k: getattr(new, k).cpu().numpy() for k in COMMIT}, want, "replay %d" % c, COMMIT)
        plain._same({k: o.cpu().numpy() for k, o in zip(RESULT, tail)}, s.ref.result(False), "result of replay %d" % c, RESULT)
    r = s.results("after the replays")[True]
    assert r["frames"].tolist() == il.tolist() and r["committed"].max() > 0


@DTYPES
def test_no_look_ahead_is_the_window_as_it_was_and_the_state_has_one_size(dtype):
    A = _asg()
    lex, lm, x, tr, il = grid_case(3, dtype)
    la = A.WordLookahead(lex, lm, 2)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    a = A.BeamWordWindowStream(trd, lex, lm, 4, 8, 2, 6, 4.0, LW, WS, TS)
    b = A.BeamWordWindowStream(trd, lex, lm, 4, 8, 2, 6, 4.0, LW, WS, TS, lookahead=None)
    c = A.BeamWordWindowStream(trd, lex, lm, 4, 8, 2, 6, 4.0, LW, WS, TS, lookahead=la)
    assert a._state.numel() == b._state.numel() == c._state.numel()
    ref = plain.BeamWordWindowRef(tr.numpy(), lex, lm, 4, 8, 2, 6, 4.0, LW, WS, TS, NP[dtype])
    c.advance(xd[:7], ild.clamp(max=7))                    # (a look-ahead stream at work beside the two)
    for t0, t1 in ((0, 5), (5, 12)):
        n = (il - t0).clamp(0, t1 - t0)
        want = dict(zip(COMMIT, ref.advance(x[t0:t1].numpy(), n.numpy())))
        for s in (a, b):
            out = s.advance(xd[t0:t1], n.to(DEV))
            plain._same({k: getattr(out, k).cpu().numpy() for k in COMMIT}, want, "lookahead=None", COMMIT)
        c.result(False)
        for final in (False, True):
            for s in (a, b):
                plain._same({k: o.cpu().numpy() for k, o in zip(RESULT, s.result(final))}, ref.result(final), "lookahead=None", RESULT)
