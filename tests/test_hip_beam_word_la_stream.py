"""GPU tests (-m gpu) of LM look-ahead in the streaming lexicon + word-LM beam decoder (`BeamWordStream(..., lookahead=)`,
csrc/asg_beam_word_stream.hip compiled with the look-ahead flag): the bytes of all ten outputs, final and prefix, against the
test-side restatement with explicit carried state (tests/beam_word_la_stream_ref.py, held to the one-shot look-ahead restatement
on the CPU by tests/test_beam_word_la_stream_cpu.py), and `result(final=True)` against the device's own
`beam_decode_words(..., lookahead=)`.  Every case first asserts, from the restatement's own sets, the regime it names."""
import numpy as np
import pytest
import torch

import test_hip_beam_word_stream as plain
from beam_word_la_stream_ref import BeamWordLaStreamRef
from beam_word_stream_ref import NAMES, BeamWordStreamRef
from test_beam_word_la_cpu import hand_case, rescue_case
from test_beam_word_la_stream_cpu import prefix_case
from test_hip_beam_word import ties_case, wide_lexicon_and_lm
from test_hip_beam_word_stream import _normal, _res, _same, _same_as_one_shot, grid_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
ONE = NAMES[:8]
ALL = 1024
LW, WS, TS = 0.7, -0.4, 0.3
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
NP = {torch.float32: np.float32, torch.float64: np.float64}


def _asg():
    import torch_asg_amd
    return torch_asg_amd


class Both(plain.Both):
    """The device stream with a look-ahead of `order` and its restatement, driven by the same calls."""

    def __init__(self, tr, lex, lm, la, B, M, K, theta=INF, lw=LW, ws=WS, ts=TS):
        self.dev = _asg().BeamWordStream(tr.to(DEV), lex, lm, B, M, K, theta, lw, ws, ts, tr.dtype, DEV, lookahead=la)
        self.ref = BeamWordLaStreamRef(tr.numpy(), lex, lm, la.order, B, M, K, theta, lw, ws, ts, NP[tr.dtype])


def _gpu_one_shot(x, tr, lex, lm, la, il, K, theta=INF, lw=LW, ws=WS, ts=TS):
    out = _asg().beam_decode_words(x.to(DEV), tr.to(DEV), lex, lm, None if il is None else il.to(DEV), K, theta, lw, ws, ts,
                                   lookahead=la)
    torch.cuda.synchronize()
    return {n: o.cpu().numpy() for n, o in zip(ONE, out)}


# ---------------------------------------------------------------------------------------------------------------- 1. chunks
@DTYPES
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("lm_order", [2, 3], ids=["bigram", "trigram"])
def test_any_chunking_gives_the_one_shot_look_ahead_decode(lm_order, order, dtype):
    lex, lm, x, tr, il = grid_case(lm_order, dtype)
    la = _asg().WordLookahead(lex, lm, order)
    T, B, sep = 12, 4, 4
    changed = carried = 0
    for K in (1, 2, 3, 8, ALL):
        for theta in (INF, 2.0, 0.0):
            what = "K=%d theta=%s order=%d" % (K, theta, order)
            one = _gpu_one_shot(x, tr, lex, lm, la, il, K, theta)
            ends = []
            for name, cuts in (("ones", list(range(T + 1))), ("whole", [0, T]), ("mixed", [0, 1, 5, 5, 12])):
                s = Both(tr, lex, lm, la, B, T, K, theta)
                s.feed(x, il, cuts, check="%s %s" % (name, what))        # the prefix result after every chunk
                ends.append(s.check("%s %s" % (name, what))[True])
                if name == "ones" and K == ALL and theta == INF:
                    # separator edges on slot 0's path: under "ones" each is the first frame of a chunk, so `look` read an h
                    # that an earlier call stored; the regime of order >= 2 is an h whose row is not the empty history's
                    p, h = ends[-1]["path"][0], ends[-1]["lm_states"][0]
                    edges = [t for t in range(1, T) if p[t] == sep and p[t - 1] != sep]
                    assert len(edges) >= 2
                    carried += sum(int(la.la_state[h[t - 1]]) != 0 for t in edges)
            s = Both(tr, lex, lm, la, B, T, K, theta)                    # per-slot chunk_lengths inside one Tc
            s.advance(x[:7], torch.tensor([7, 2, 1, 0]))
            second = torch.zeros(5, B, 5, dtype=dtype)
            second[:5, 0], second[:3, 1] = x[7:12, 0], x[2:5, 1]
            s.advance(second, torch.tensor([5, 3, 0, 0]))
            ends.append(s.check("lengths " + what)[True])
            for e in ends:
                _same_as_one_shot(e, one, T, what)
                assert e["frames"].tolist() == il.tolist() and not e["status"].any()
            if K <= 3 and theta == INF:
                p = BeamWordStreamRef(tr.numpy(), lex, lm, B, T, K, theta, LW, WS, TS, NP[dtype])
                p.advance(x.numpy(), il.numpy())
                changed += p.kept() != s.ref.kept()
            if K == ALL and theta == INF:
                assert max(max(z) for z in s.ref.sizes() if z) < ALL
    assert changed > 0                                     # the look-ahead changed what a narrow beam keeps
    assert carried > 0 or order == 1                       # (order 1 reads the empty history's row for every h)


# ---------------------------------------------------------------------------------------------------------------- 2. ties
@DTYPES
def test_integer_ties_at_the_last_rank_and_between_sources(dtype):
    lex, lm, x, tr, il = ties_case(dtype)
    cuts = srcs = 0
    for order in (1, 2):
        la = _asg().WordLookahead(lex, lm, order)
        for K in (1, 2, 3, 5, 8):
            for theta in (INF, 1.0, 0.0):
                for chunks in ([0, 3, 3, 8], list(range(9))):
                    s = Both(tr, lex, lm, la, 5, 8, K, theta, 1.0, 1.0, 0.0)
                    s.feed(x, il, chunks)
                    s.check("ties K=%d theta=%s order=%d %s" % (K, theta, order, chunks))
                    cuts += s.ref.tie_cuts
                    srcs += s.ref.src_ties
    assert cuts > 0 and srcs > 0


# ---------------------------------------------------------------------------------------------------------------- 3. rescue
@DTYPES
def test_look_ahead_rescues_the_word_through_one_frame_chunks_at_a_beam_of_one(dtype):
    A = _asg()
    lex, lm, x, tr = rescue_case(NP[dtype])
    x, tr = torch.from_numpy(x), torch.from_numpy(tr)
    best = plain._gpu_one_shot(x, tr, lex, lm, None, ALL, INF, 1.0, 0.0, 0.0)
    narrow = plain._gpu_one_shot(x, tr, lex, lm, None, 1, INF, 1.0, 0.0, 0.0)
    assert best["words"][0, 0] == 1 and narrow["words"][0, 0] == 0 and narrow["scores"][0] < best["scores"][0]
    for order in (1, 2):
        s = Both(tr, lex, lm, A.WordLookahead(lex, lm, order), 1, 3, 1, INF, 1.0, 0.0, 0.0)
        s.feed(x, torch.tensor([3]), [0, 1, 2, 3], check="rescue")
        got = s.check("rescue")[True]
        assert all(z == 1 for z in s.ref.sizes()[0])
        _same(got, best, "rescue order=%d" % order, ONE)


# ---------------------------------------------------------------------------------------------------------------- 4. ends
@DTYPES
def test_dead_ends_are_pruned_on_entry_and_every_kind_of_end_final_and_prefix(dtype):
    A = _asg()
    lex, lm = hand_case()                                  # the nodes [3] and [3, 0] have no word below them that the LM knows
    x, tr = _normal(7, 4, 5, 37, dtype)
    x[:, :, 3] += 2.0                                      # acoustics like the dead branch
    il = torch.tensor([7, 4, 1, 0])
    for order in (1, 2, 3):
        for K in (2, 8, ALL):
            s = Both(tr, lex, lm, A.WordLookahead(lex, lm, order), 4, 7, K)
            s.feed(x, il, [0, 1, 4, 7], check="dead order=%d K=%d" % (order, K))
            got = s.check("dead order=%d K=%d" % (order, K))
            assert s.ref.dead > 0 and (got[True]["states"] < 5).all() and (got[False]["states"] < 5).all()
    # word 0 = [0] is unknown to the LM, word 1 = [0, 1] known: slot 0 stays in the node of word 0 (its end is rejected), slot 1
    # comes back to it behind a separator (rejected), slot 2 goes on into the node of word 1 (an end in a word-end node)
    lex2 = A.Lexicon([[0], [0, 1]], 3, 2)
    lm2 = A.WordLM(2, [0, 1], [1], [-0.5], [0], [-1], [0.0], 0, [-1.0])
    tr2 = torch.zeros(3, 3, dtype=dtype)
    x2 = torch.full((5, 3, 3), -9.0, dtype=dtype)
    for b, labs in enumerate(([0, 0, 0, 0, 0], [0, 1, 2, 0, 0], [0, 1, 2, 0, 1])):
        for t, lab in enumerate(labs):
            x2[t, b, lab] = 0.0
    s = Both(tr2, lex2, lm2, A.WordLookahead(lex2, lm2, 2), 3, 5, 1, INF, 1.0, 0.0, 0.0)
    s.feed(x2, torch.tensor([5, 5, 5]), [0, 2, 3, 5], check="ends")
    got = s.check("ends")
    assert [len(k[-1]) for k in s.ref.kept()] == [1, 1, 1]
    assert got[True]["scores"][0] == -np.inf and got[True]["scores"][1] == -np.inf and got[True]["scores"][2] > -np.inf
    assert got[True]["words"][2].tolist() == [1, 1, -1, -1, -1] and got[True]["states"][2, -1] == 2
    assert (got[False]["scores"] > -np.inf).all() and got[False]["words"][2].tolist() == [1, -1, -1, -1, -1]
    # the prefix rule's own case: the mid-word pair holds the largest value, the pair at the root the best prefix
    lex3, lm3, x3, tr3, ws = prefix_case(NP[dtype])
    for order in (1, 2):
        s = Both(torch.from_numpy(tr3), lex3, lm3, A.WordLookahead(lex3, lm3, order), 1, 4, ALL, INF, 1.0, ws, 0.0)
        s.feed(torch.from_numpy(x3), torch.tensor([4]), [0, 3, 4], check="prefix")
        (hv, qv), vmax = min(s.ref.slots[0].A, key=lambda it: (-it[1], it[0]))
        got = s.check("prefix")[False]
        assert s.ref.state[qv] != 0 and got["states"][0, 3] == 0 and got["scores"][0] == vmax - 1.0
        p = plain.Both(torch.from_numpy(tr3), lex3, lm3, 1, 4, ALL, INF, 1.0, ws, 0.0)
        p.feed(torch.from_numpy(x3), torch.tensor([4]), [0, 3, 4])
        _same(got, p.check("prefix, no look-ahead")[False], "an unpruned prefix is the plain stream's")


# ---------------------------------------------------------------------------------------------------------------- 5. wide
def test_wide_beam_strips_the_workgroup_and_loads_the_table():
    lex, lm = wide_lexicon_and_lm()
    la = _asg().WordLookahead(lex, lm, 2)
    x, tr = _normal(6, 2, 40, 33, torch.float32)
    s = Both(tr * 0.25, lex, lm, la, 2, 6, 1200, INF, 0.5, -0.2, 0.1)
    s.feed(x * 0.25, torch.tensor([6, 5]), [0, 1, 3, 6])   # flat emissions: many pairs stay close
    assert max(max(c) for c in s.ref.cands()) > 1024 and max(max(z) for z in s.ref.sizes()) > 1024
    got = s.check("wide")[True]
    _same_as_one_shot(got, _gpu_one_shot(x * 0.25, tr * 0.25, lex, lm, la, torch.tensor([6, 5]), 1200, INF, 0.5, -0.2, 0.1), 6, "wide")


# ---------------------------------------------------------------------------------------------------------------- 6. layouts
@pytest.mark.parametrize("N", [141, 142], ids=["transitions-in-lds", "transitions-in-global-memory"])
def test_both_transition_layouts(N):
    """float64, K = 8: 4096 + 8 * 16 + N * N * 8 bytes is within the 160 KiB of LDS for N = 141 and beyond them for N = 142."""
    A = _asg()
    K = 8
    assert (4096 + K * 16 + N * N * 8 <= 160 * 1024) == (N == 141)
    lex = A.Lexicon([[3, 7], [3, 100, 5], [N - 2]], N, N - 1)
    lm = plain.arpa_lm(3, 2, 73)
    x, tr = _normal(6, 2, N, 37, torch.float64)
    for t, lab in enumerate([3, 7, N - 1, N - 2, N - 1, 3]):
        x[t, 0, lab] += 6.0
    s = Both(tr, lex, lm, A.WordLookahead(lex, lm, 2), 2, 6, K, INF)
    s.feed(x, torch.tensor([6, 4]), [0, 2, 6], check="N=%d" % N)
    got = s.check("N=%d" % N)
    assert got[True]["word_lengths"][0] >= 2 and max(max(z) for z in s.ref.sizes()) > 1


# ---------------------------------------------------------------------------------------------------------------- 7. empty
@DTYPES
def test_a_beam_that_empties_inside_a_chunk(dtype):
    lex, lm, x, tr, _ = grid_case(2, dtype, T=9)
    x = x[:, :3].clone()
    x[4, 0] = -INF                                         # chunks [3, 3, 3]: inside the second chunk,
    x[3, 1] = -INF                                         # on its first frame,
    x[5, 2] = -INF                                         # on its last
    s = Both(tr, lex, lm, _asg().WordLookahead(lex, lm, 2), 3, 12, 6, 4.0)
    s.feed(x, torch.tensor([9, 9, 9]), [0, 3, 6, 9], check="empty")
    sizes = s.ref.sizes()
    for b, t0 in enumerate((4, 3, 5)):
        assert all(z > 0 for z in sizes[b][:t0]) and all(z == 0 for z in sizes[b][t0:]) and len(sizes[b]) == 9
    got = s.check("empty")
    for final in (False, True):
        assert (got[final]["scores"] == -np.inf).all() and got[final]["frames"].tolist() == [9, 9, 9]
        assert (got[final]["path"] == -1).all() and not got[final]["status"].any()


# ---------------------------------------------------------------------------------------------------------------- 8. plumbing
def test_masked_reset_mid_stream():
    lex, lm, x, tr, _ = grid_case(3, torch.float32)
    la = _asg().WordLookahead(lex, lm, 2)
    y, _ = _normal(12, 4, 5, 40, torch.float32)
    s = Both(tr, lex, lm, la, 4, 12, 5, 5.0)
    s.advance(x[:6])
    s.reset(torch.tensor([False, True, False, True]))
    mixed = x[6:].clone()
    mixed[:, 1], mixed[:, 3] = y[:6, 1], y[:6, 3]          # slots 1 and 3 start a new utterance, the others go on
    s.advance(mixed)
    got = s.check("masked reset")[True]
    assert got["frames"].tolist() == [12, 6, 12, 6] and not got["status"].any()
    want_x = _gpu_one_shot(x, tr, lex, lm, la, None, 5, 5.0)
    want_y = _gpu_one_shot(y[:6], tr, lex, lm, la, None, 5, 5.0)
    for b in range(4):
        want, L = (want_x, 12) if b % 2 == 0 else (want_y, 6)
        _same_as_one_shot({n: got[n][b:b + 1] for n in ONE}, {n: want[n][b:b + 1] for n in ONE}, L, "slot %d" % b)
    s.reset()
    assert s.check("full reset")[True]["frames"].tolist() == [0, 0, 0, 0]


def test_capture_of_advance_and_result_with_three_replays():
    lex, lm, _, tr, _ = grid_case(3, torch.float32)
    la = _asg().WordLookahead(lex, lm, 2)
    Tc, B, K, theta = 4, 3, 12, 6.0
    T = 3 * Tc
    x, _ = _normal(T, B, 5, 41, torch.float32)
    il = torch.tensor([T, 9, T - 2])
    s = Both(tr, lex, lm, la, B, T, K, theta)
    buf = torch.zeros(Tc, B, 5, device=DEV)
    n = torch.zeros(B, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.dev.advance(buf, n)                              # warm-up; n = 0: the state stays as it is
        s.dev.result(False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        s.dev.advance(buf, n)
        out = s.dev.result(False)
    s.dev.reset()                                          # (the capture itself ran nothing)
    for c in range(3):
        buf.copy_(x[c * Tc:(c + 1) * Tc])
        n.copy_((il - c * Tc).clamp(0, Tc))
        gr.replay()
        torch.cuda.synchronize()
        s.ref.advance(x[c * Tc:(c + 1) * Tc].numpy(), (il - c * Tc).clamp(0, Tc).numpy())
        _same({k: o.cpu().numpy() for k, o in zip(NAMES, out)}, s.ref.result(False), "replay %d" % c)
    got = s.check("three replays")[True]
    _same_as_one_shot(got, _gpu_one_shot(x, tr, lex, lm, la, il, K, theta), T, "three replays")


def test_two_streams_give_identical_bits_and_the_state_has_the_plain_size():
    A = _asg()
    lex, lm = wide_lexicon_and_lm()
    la = A.WordLookahead(lex, lm, 2)
    x, tr = _normal(12, 6, 40, 36, torch.float32)
    xd, trd = (x * 0.25).to(DEV), tr.to(DEV)
    il = torch.tensor([12, 3, 0, 1, 11, 7])
    runs = []
    for _ in range(2):
        s = A.BeamWordStream(trd, lex, lm, 6, 12, 300, 6.0, 0.5, -0.2, 0.1, lookahead=la)
        for t0, t1 in ((0, 5), (5, 6), (6, 12)):
            s.advance(xd[t0:t1], (il - t0).clamp(0, t1 - t0).to(DEV))
        runs.append((_res(s, True), _res(s, False)))
    for u, v in zip(runs[0], runs[1]):
        _same(u, v, "two streams")
    _same_as_one_shot(runs[0][0], _gpu_one_shot(x * 0.25, tr, lex, lm, la, il, 300, 6.0, 0.5, -0.2, 0.1), 12, "wide, one shot")
    p = A.BeamWordStream(trd, lex, lm, 6, 12, 300, 6.0, 0.5, -0.2, 0.1)
    assert p._state.numel() == s._state.numel() and p.lookahead is None and s.lookahead is la
    with pytest.raises(NotImplementedError):
        s.result_nbest(2)
    assert p.result_nbest(2).scores.shape == (6, 2)


@DTYPES
def test_no_look_ahead_is_the_stream_as_it_was(dtype):
    A = _asg()
    lex, lm, x, tr, il = grid_case(3, dtype)
    xd, trd = x.to(DEV), tr.to(DEV)
    for K, theta in ((2, INF), (16, 3.0)):
        a = A.BeamWordStream(trd, lex, lm, 4, 12, K, theta, LW, WS, TS, dtype)
        b = A.BeamWordStream(trd, lex, lm, 4, 12, K, theta, LW, WS, TS, dtype, lookahead=None)
        c = A.ASGLoss(5).to(DEV).to(dtype)
        with torch.no_grad():
            c.transition.copy_(trd)
        c = c.beam_word_stream(lex, lm, 4, 12, K, theta, LW, WS, TS, lookahead=None)
        ref = BeamWordStreamRef(tr.numpy(), lex, lm, 4, 12, K, theta, LW, WS, TS, NP[dtype])
        for t0, t1 in ((0, 5), (5, 12)):
            n = (il - t0).clamp(0, t1 - t0)
            for s in (a, b, c):
                s.advance(xd[t0:t1], n.to(DEV))
            ref.advance(x[t0:t1].numpy(), n.numpy())
            for final in (False, True):
                want = ref.result(final)
                for s in (a, b, c):
                    _same(_res(s, final), want, "lookahead=None K=%d final=%s" % (K, final))


def test_the_plain_decoders_are_unchanged_right_after_look_ahead_stream_calls():
    A = _asg()
    lex, lm, x, tr, il = grid_case(3, torch.float32)
    la = A.WordLookahead(lex, lm, 2)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)

    def older():
        w = A.BeamWordStream(trd, lex, lm, 4, 12, 6, 4.0, LW, WS, TS)
        w.advance(xd[:5], ild.clamp(max=5))
        w.advance(xd[5:], (ild - 5).clamp(0, 7))
        win = A.BeamWordWindowStream(trd, lex, lm, 4, 8, 2, 6, 4.0, LW, WS, TS)
        outs = list(win.advance(xd, ild)) + list(win.result(True)) + list(w.result(True)) + list(w.result(False))
        outs += list(A.beam_decode_words(xd, trd, lex, lm, ild, 6, 4.0, LW, WS, TS))
        outs += list(A.beam_decode_words(xd, trd, lex, lm, ild, 6, 4.0, LW, WS, TS, lookahead=la))
        return [o.cpu() for o in outs]
    before = older()
    s = A.BeamWordStream(trd, lex, lm, 4, 12, 6, 4.0, LW, WS, TS, lookahead=la)
    s.advance(xd[:7], ild.clamp(max=7))
    _res(s, False)
    after = older()
    s.advance(xd[7:], (ild - 7).clamp(0, 5))
    _res(s, True)
    again = older()
    for u, v, w in zip(before, after, again):
        assert torch.equal(u, v) and torch.equal(u, w)
    p = BeamWordStreamRef(tr.numpy(), lex, lm, 4, 12, 6, 4.0, LW, WS, TS)
    p.advance(x.numpy(), il.numpy())
    for final, outs in ((True, before[19:29]), (False, before[29:39])):
        for n, o in zip(NAMES, outs):
            assert o.numpy().tobytes() == p.result(final)[n].tobytes(), (n, final)
