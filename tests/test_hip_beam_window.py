"""GPU tests (-m gpu) of windowed streaming beam decoding (`torch_asg_amd.BeamWindowStream`, csrc/asg_beam_window.hip): every
output of every call -- what each `advance` commits, the tail, `frames` / `committed` / `status` of `result` -- is, byte for byte,
that of the restatement (tests/beam_window_ref.py), over windows, commit periods, beams, thresholds, dtypes and chunkings; forced
commits on an automaton of two components; dozens of wraps of the ring; a beam that empties after a commit; both transition
layouts; the lane groups of the expansion; mark sets wider than one stride of the workgroup; the device's own one-shot decoder and
unbounded stream; masked reset; capture and replay; determinism; errors; and the older beam routes after window calls."""
import numpy as np
import pytest
import torch

from beam_decode_ref import beam_decode_ref
from beam_stream_ref import BeamStreamRef
from beam_window_ref import BeamWindowRef, chain_automaton, two_component_emissions, two_components_automaton

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
LW, TS = 0.8, -0.5
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
NP = {torch.float32: np.float32, torch.float64: np.float64}


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _ngram(N, order, seed, holes=False):
    rng = np.random.default_rng(seed)
    lp = np.log(rng.dirichlet(np.ones(N + 1), size=(N + 1,) * (order - 1))) if order > 1 else np.log(rng.dirichlet(np.ones(N + 1)))
    if holes:
        lp[rng.random(size=lp.shape) < 0.2] = -np.inf
    return _asg().TokenGraph.from_ngram(lp)


def _case(T, B, N, seed, dtype=torch.float32, integer=False):
    g = torch.Generator().manual_seed(seed)
    if integer:
        x = torch.randint(-2, 3, (T, B, N), generator=g).to(dtype)
        tr = torch.randint(-1, 2, (N, N), generator=g).to(dtype)
    else:
        x = torch.log_softmax(torch.randn(T, B, N, generator=g, dtype=torch.float64), -1).to(dtype)
        tr = torch.randn(N, N, generator=g, dtype=torch.float64).to(dtype)
    il = torch.randint(2, T + 1, (B,), generator=g)
    il[0] = T
    if B > 1:
        il[1] = 0
    if B > 2:
        il[2] = 1
    return x, tr, il


def _Q(graph):
    return graph.compile_host(np.float32, LW, TS)["Q"]


def _one_shot(x, tr, graph, il, K, theta):
    return beam_decode_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start,
                           None if il is None else il.numpy(), K, theta, LW, TS)


def _pair(tr, graph, B, W, P, K, theta=INF):
    """The device's stream and the restatement, side by side."""
    s = _asg().BeamWindowStream(tr.to(DEV), graph, B, W, P, K, theta, LW, TS, dtype=tr.dtype)
    ref = BeamWindowRef(tr.numpy(), graph.next, graph.weight, graph.final, graph.start, B, W, P, K, theta, LW, TS, NP[tr.dtype])
    return s, ref


def _same(got, want, what):
    """Every array bit for bit (array_equal would let -0 pass for +0)."""
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (i, what)
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), "output %d %s" % (i, what)


def _advance(s, ref, chunk, n, what):
    """One call on both; every output compared."""
    out = s.advance(chunk.to(DEV), None if n is None else n.to(DEV))
    assert type(out).__name__ == "BeamWindowCommit"
    want = ref.advance(chunk.numpy(), None if n is None else n.numpy())
    got = [o.cpu().numpy() for o in (out.path, out.states, out.tokens, out.frames, out.token_lengths)]
    _same(got, want, what)
    return got


def _results(s, ref, what):
    for final in (False, True):
        out = s.result(final)
        assert type(out).__name__ == "BeamWindowResult"
        _same([o.cpu().numpy() for o in out], ref.result(final), "%s final=%s" % (what, final))


def _feed(s, ref, x, il, cuts, what, results=False):
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        _advance(s, ref, x[t0:t1], None if il is None else (il - t0).clamp(0, t1 - t0), "%s chunk %d:%d" % (what, t0, t1))
        if results:
            _results(s, ref, "%s after %d" % (what, t1))
    _results(s, ref, what)


def _feed_ragged(s, ref, x, il, Tc, seed, what):
    """Calls that each offer Tc frames of which every slot takes a number of its own: the slots drift apart inside one shape."""
    T, B, N = x.shape
    g = torch.Generator().manual_seed(seed)
    pad = torch.cat([x, torch.zeros(Tc, B, N, dtype=x.dtype)])
    pos = torch.zeros_like(il)
    while bool((pos < il).any()):
        n = torch.minimum(torch.randint(0, Tc + 1, (B,), generator=g), il - pos)
        chunk = torch.stack([pad[int(pos[b]):int(pos[b]) + Tc, b] for b in range(B)], 1)
        _advance(s, ref, chunk, n, "%s ragged at %s" % (what, pos.tolist()))
        pos = pos + n
    _results(s, ref, what)


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "random"])
@DTYPES
def test_every_output_of_every_call_equals_the_restatement(dtype, integer):
    graph = _ngram(6, 3, 3, holes=True)
    Q = _Q(graph)
    T, B, N = 40, 5, 6
    x, tr, il = _case(T, B, N, 11, dtype, integer)
    assert il[0] == T and il[1] == 0 and il[2] == 1
    turn = forced = exact = 0
    for K in (1, 3, 8, Q):
        for theta in (INF, 2.0, 0.0):
            one = _one_shot(x, tr, graph, il, K, theta)
            for W in (4, 8, 16):
                for P in (1, 3, W):
                    cuts = {0: list(range(T + 1)), 1: [0, T], 2: [0, 1, 8, 8, 24, 40],
                            3: None,                                            # per-slot lengths inside one Tc
                            4: list(range(0, T, 3 * P + 1)) + [T],              # a chunk spans several commit attempts
                            5: [0, 0, 20, 20, 40, 40]}[turn % 6]                # chunks of no frames
                    what = "K=%d theta=%s W=%d P=%d chunking %d" % (K, theta, W, P, turn % 6)
                    turn += 1
                    s, ref = _pair(tr, graph, B, W, P, K, theta)
                    if cuts is None:
                        _feed_ragged(s, ref, x, il, 7, turn, what)
                    else:
                        _feed(s, ref, x, il, cuts, what)
                    res = ref.result(True)
                    assert res[0].tobytes() == one[0].tobytes() and res[5].tolist() == il.tolist(), what
                    forced += int((res[7] & 1).sum())
                    exact += int(((res[7] & 1) == 0).sum())
    assert forced > 0 and exact > 0 and turn >= 6


@pytest.mark.parametrize("K", [2, 4])
def test_forced_commits_on_two_components(K):
    graph = _asg().TokenGraph(*two_components_automaton(), start=0)
    T, B, W, P = 30, 2, 8, 2
    x = torch.from_numpy(two_component_emissions(T, B, graph.N, np.float64))
    tr = torch.zeros(graph.N, graph.N, dtype=torch.float64)
    il = torch.tensor([T, T - 3])
    s, ref = _pair(tr, graph, B, W, P, K)
    _feed(s, ref, x, il, [0, 5, 6, 17, 30], "two components", results=True)
    for v in ref.slots:                                             # the regime: nothing converged, every full window forced
        assert v.status == 1 and all(c is None for _, _, c, _ in v.attempts) and v.base == v.pos // P * P - (W - P)


def test_dozens_of_wraps_with_one_slot():
    graph = _ngram(6, 2, 7)
    T, B, W = 300, 2, 8
    x, tr, _ = _case(T, B, 6, 13)
    il = torch.tensor([T, T - 5])
    for P in (1, 8):
        s, ref = _pair(tr, graph, B, W, P, 1)
        _feed(s, ref, x, il, list(range(0, T, 37)) + [T], "K=1 P=%d" % P)
        assert all(v.status == 0 and v.pos > 30 * W and v.base == v.pos // P * P for v in ref.slots)
        one = _one_shot(x, tr, graph, il, 1, INF)
        assert ref.result(True)[0].tobytes() == one[0].tobytes() and (one[0] > -INF).all()


@DTYPES
def test_a_beam_that_empties_inside_a_chunk_after_a_commit(dtype):
    graph = _ngram(6, 2, 7)
    T, B, K, W, P = 14, 2, 3, 4, 2
    x, tr, _ = _case(T, B, 6, 17, dtype)
    x[9] = -INF                                                     # nothing survives frame 9
    il = torch.tensor([T, 8])
    for cuts in ([0, 6, 12, 14], [0, 9, 10, 14], [0, 10, 14]):
        s, ref = _pair(tr, graph, B, W, P, K)
        _feed(s, ref, x, il, cuts, str(cuts), results=True)
        v = ref.slots[0]
        assert v.base > 0 and v.aq.size == 0 and v.pos == T and ref.result()[7].tolist()[0] & 2


def test_both_transition_layouts():
    """The transitions sit in LDS while they fit beside the beam and the mark sets (4096 + 16 + K*(e+4) + 8 + N*N*e <= 160 KiB)
    and are read from global memory beyond: float64 and K = 8 put the last N in LDS at 141."""
    lds = lambda N, K=8, e=8: 4096 + 16 + K * (e + 4) + 8 + N * N * e
    assert lds(141) <= 160 * 1024 < lds(142) and lds(141) > 64 * 1024
    for N in (141, 142):
        graph = _ngram(N, 2, N)
        T, B = 6, 2
        x, tr, il = _case(T, B, N, 23, torch.float64)
        il[1] = 3
        s, ref = _pair(tr, graph, B, 4, 2, 8, 3.0)
        _feed(s, ref, x, il, [0, 1, 4, 6], "N=%d" % N)
        assert (ref.result(True)[0] > -INF).all()


def test_lanes_per_state():
    """K = 1: 64 lanes share a state's outgoing row; K >= 1024: one lane per state, and a strip of 1024 states per pass."""
    graph = _ngram(32, 3, 9)
    Q = _Q(graph)
    assert 1024 < Q < 1100
    T, B = 8, 2
    x, tr, il = _case(T, B, 32, 29)
    il[1] = 5
    for K, theta in ((1, INF), (1024, INF), (1024, 6.0)):
        s, ref = _pair(tr, graph, B, 4, 2, K, theta)
        _feed(s, ref, x, il, [0, 3, 4, 8], "K=%d theta=%s" % (K, theta))


def test_mark_sets_wider_than_one_stride():
    graph = _ngram(45, 3, 19)
    Q, K = _Q(graph), 2048
    assert K < Q < 2200
    T, B = 12, 2
    x, tr, il = _case(T, B, 45, 31)
    il[1] = 9
    un = BeamStreamRef(tr.numpy(), graph.next, graph.weight, graph.final, graph.start, B, T, K, INF, LW, TS, np.float32)
    un.advance(x.numpy(), il.numpy())
    assert 1024 < min(un.sizes()[0][1:]) <= K                       # slots beyond the first 1024 lanes are marked in every scan
    for W, P in ((4, 2), (8, 3)):
        s, ref = _pair(tr, graph, B, W, P, K)
        _feed(s, ref, x, il, [0, 5, 12], "W=%d" % W)
        assert any(c is not None or F for v in ref.slots for _, _, c, F in v.attempts)


@DTYPES
def test_against_the_devices_own_decoders(dtype):
    A = _asg()
    graph = _ngram(12, 3, 21, holes=True)
    T, B = 40, 6
    x, tr, il = _case(T, B, 12, 47, dtype)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    loss = A.ASGLoss(12).to(DEV).to(dtype)
    with torch.no_grad():
        loss.transition.copy_(trd)
    cuts = [0, 8, 16, 17, 40]
    for K, theta in ((16, INF), (64, 4.0)):
        want = A.beam_decode_graph(xd, trd, graph, ild, K, theta, LW, TS)
        s = loss.beam_window_stream(graph, B, 8, 2, K, theta, LW, TS)            # the module method
        un = loss.beam_stream(graph, B, T, K, theta, LW, TS)
        assert s.window == 8 and s.commit_every == 2
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            n = (ild - t0).clamp(0, t1 - t0)
            s.advance(xd[t0:t1], n)
            un.advance(xd[t0:t1], n)
            assert s.result(False).scores.cpu().numpy().tobytes() == un.result(False).scores.cpu().numpy().tobytes()
        assert s.result(True).scores.cpu().numpy().tobytes() == want[0].cpu().numpy().tobytes()
    if dtype == torch.float32:
        s = A.BeamWindowStream(trd, graph, B, 8)                                 # commit_every defaults to window // 4
        r = A.BeamWindowStream(trd, graph, B, 8, 2)
        assert s.commit_every == 2
        a = s.advance(xd[:9].to(torch.bfloat16), ild.clamp(max=9))              # half precision chunks are widened
        b = r.advance(xd[:9].to(torch.bfloat16).float().transpose(0, 1).contiguous().transpose(0, 1), ild.clamp(max=9))
        _same([o.cpu().numpy() for o in a], [o.cpu().numpy() for o in b], "bfloat16 / strided")


def test_masked_reset_mid_stream():
    graph = _ngram(6, 3, 3, holes=True)
    T, B, K, theta = 14, 2, 4, 5.0
    x, tr, _ = _case(T, B, 6, 43)
    y, _, _ = _case(T, B, 6, 44)
    s, ref = _pair(tr, graph, B, 4, 2, K, theta)
    _advance(s, ref, x[:6], None, "before the reset")
    mask = torch.tensor([False, True])
    s.reset(mask.to(DEV))
    ref.reset(mask.numpy())
    _results(s, ref, "after the masked reset")
    mixed = x[6:].clone()
    mixed[:, 1] = y[:T - 6, 1]                                       # slot 1 starts a new utterance, slot 0 goes on
    _advance(s, ref, mixed, None, "after the reset")
    _results(s, ref, "the end")
    res = ref.result(True)
    assert res[5].tolist() == [T, T - 6]
    assert res[0][0].tobytes() == _one_shot(x, tr, graph, None, K, theta)[0][0].tobytes()
    assert res[0][1].tobytes() == _one_shot(y[:T - 6], tr, graph, None, K, theta)[0][1].tobytes()
    s.reset(torch.tensor([1, 0], dtype=torch.int32))                 # an integer mask from the host
    out = s.result()
    assert out.frames.tolist() == [0, T - 6] and out.committed.tolist()[0] == 0 and out.status.tolist()[0] == 0


def test_masked_reset_of_a_used_slot_beyond_one_pass_of_the_reset():
    """The reset shares the Q entries of val / arg among 64 workgroups of 256 threads: 16384 per pass.  A chain of Q a little
    above that, walked down from its last state, keeps the search in the product states of the SECOND pass.  Slot 0 decodes,
    is reset under a mask and decodes other emissions; every output of every call against the restatement, byte for byte.
    What this can and cannot see: a frame empties the entries it touched, so val / arg of a used slot are empty before the
    masked reset as well, and a reset that skipped the second pass would pass the second half.  The constructor's reset of
    the freshly allocated (poisoned) state is the part that fails when entries >= 16384 are not cleared or the clearing lands
    at a wrong offset; the masked reset is checked for its header and for leaving slot 1 alone."""
    S, N = 3290, 5
    graph = _asg().TokenGraph(*chain_automaton(S, N))
    h = graph.compile_host(np.float32, LW, TS)
    T, B, K, W, P = 6, 2, 4, 4, 1
    assert 16384 < h["Q"] < 16384 + 128 and np.nonzero(h["state"] >= S - 1 - T)[0].min() >= 16384
    x, tr, _ = _case(T, B, N, 61)
    y, _, _ = _case(T, B, N, 62)
    s, ref = _pair(tr, graph, B, W, P, K)
    _feed(s, ref, x, None, [0, 2, T], "the first utterance")
    st = ref.result(True)[4]
    assert (ref.result(True)[0] > -INF).all() and st[st >= 0].min() >= S - 1 - T        # the states the search used
    mask = torch.tensor([True, False])
    s.reset(mask.to(DEV))
    ref.reset(mask.numpy())
    _results(s, ref, "after the masked reset")
    _feed(s, ref, y, None, [0, 2, T], "the second utterance")      # slot 0 from its start, slot 1 goes on down the chain
    assert ref.result(True)[5].tolist() == [T, 2 * T]


def test_capture_and_replay():
    graph = _ngram(8, 3, 9)
    Tc, B, N, K, theta, W, P = 4, 3, 8, 12, 6.0, 6, 3
    T = 6 * Tc
    x, tr, _ = _case(T, B, N, 53)
    il = torch.tensor([T, 9, T - 2])
    s, ref = _pair(tr, graph, B, W, P, K, theta)
    buf = torch.zeros(Tc, B, N, device=DEV)
    n = torch.zeros(B, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.advance(buf, n)                                            # warm-up; n = 0: the state stays as it is
        s.result()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        new = s.advance(buf, n)
        tail = s.result(True)
    s.reset()                                                        # (the capture itself ran nothing)
    for c in range(6):
        buf.copy_(x[c * Tc:(c + 1) * Tc])
        cn = (il - c * Tc).clamp(0, Tc)
        n.copy_(cn)
        gr.replay()
        torch.cuda.synchronize()
        want = ref.advance(x[c * Tc:(c + 1) * Tc].numpy(), cn.numpy())
        _same([o.cpu().numpy() for o in (new.path, new.states, new.tokens, new.frames, new.token_lengths)], want, "replay %d" % c)
        _same([o.cpu().numpy() for o in tail], ref.result(True), "result of replay %d" % c)
    assert ref.result()[5].tolist() == il.tolist() and ref.result()[6].max() > 0


def test_two_runs_give_identical_bits():
    graph = _ngram(12, 3, 3, holes=True)
    T, B = 48, 8
    x, tr, il = _case(T, B, 12, 59)
    xd = x.to(DEV)
    runs = []
    for _ in range(2):
        s = _asg().BeamWindowStream(tr.to(DEV), graph, B, 8, 2, 50, 8.0, LW, TS)
        outs = []
        for t0 in (0, 16, 32):
            outs += [o.cpu().numpy() for o in s.advance(xd[t0:t0 + 16], (il - t0).clamp(0, 16).to(DEV))]
        runs.append(outs + [o.cpu().numpy() for o in s.result(True)] + [o.cpu().numpy() for o in s.result(False)])
    _same(runs[0], runs[1], "two runs")


def test_errors():
    A = _asg()
    graph = _ngram(5, 2, 10)
    tr = torch.randn(5, 5, device=DEV)
    s = A.BeamWindowStream(tr, graph, 2, 6, 2, 4)
    x = torch.randn(3, 2, 5, device=DEV)
    with pytest.raises(RuntimeError):
        s.advance(x.cpu())
    with pytest.raises(RuntimeError):
        s.advance(torch.randn(3, 2, 6, device=DEV))                  # another alphabet
    with pytest.raises(RuntimeError):
        s.advance(torch.randn(3, 3, 5, device=DEV))                  # another batch
    with pytest.raises(RuntimeError):
        s.advance(x.double())
    with pytest.raises(RuntimeError):
        s.advance(x, torch.tensor([3, 3], dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        s.advance(x, torch.tensor([3], device=DEV))
    with pytest.raises(RuntimeError):
        s.reset(torch.tensor([1, 0, 1], device=DEV))
    with pytest.raises(RuntimeError):
        A.BeamWindowStream(tr.double(), graph, 2, 6)                 # not the stream's dtype
    with pytest.raises(RuntimeError):
        A.BeamWindowStream(torch.randn(6, 6, device=DEV), graph, 2, 6)
    for W, P in ((0, None), (4, 0), (4, 5)):
        with pytest.raises(ValueError):
            A.BeamWindowStream(tr, graph, 2, W, P)
    s.beam_threshold = -1.0
    with pytest.raises(ValueError):
        s.advance(x)
    s.beam_threshold = INF
    assert s.result().frames.tolist() == [0, 0]                      # nothing above reached the state
    for _ in range(5):                                               # no bound on the frames
        s.advance(x)
    out = s.advance(x[:0])                                           # a chunk of no frames: the empty outputs
    assert tuple(out.path.shape) == (2, 6) and bool((out.path == -1).all()) and out.frames.tolist() == [0, 0]
    res = s.result()
    assert res.frames.tolist() == [15, 15] and min(res.committed.tolist()) >= 15 - 6
    s.reset()
    s.advance(x)
    assert s.result().frames.tolist() == [3, 3]


def test_the_older_beam_routes_are_unchanged_after_window_calls():
    from beam_loss_cases import _compare, _full, _ref
    from beam_nbest_ref import beam_nbest_ref
    A = _asg()
    graph = _ngram(6, 3, 3, holes=True)
    T, B = 16, 4
    x, tr, il = _case(T, B, 6, 61)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    s, ref = _pair(tr, graph, B, 4, 2, 5, 4.0)
    _feed(s, ref, x, il, [0, 7, 16], "the window stream")
    one = _one_shot(x, tr, graph, il, 5, 4.0)
    got = [o.cpu().numpy() for o in A.beam_decode_graph(xd, trd, graph, ild, 5, 4.0, LW, TS)]
    _same(got, one, "5i after window calls")
    nb = A.beam_decode_graph_nbest(xd, trd, graph, ild, 5, 3, 4.0, LW, TS, return_alignments=True)
    want = beam_nbest_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start, il.numpy(), 5, 3, 4.0, LW, TS)
    _same([o.cpu().numpy() for o in nb], want, "5k after window calls")
    un = A.BeamStream(trd, graph, B, T, 5, 4.0, LW, TS)
    un.advance(xd[:7], ild.clamp(max=7))
    un.advance(xd[7:], (ild - 7).clamp(min=0))
    r = [o.cpu().numpy() for o in un.result(True)]
    assert r[0].tobytes() == one[0].tobytes() and np.array_equal(r[1], one[1]) and np.array_equal(r[2], one[2])
    xs, trs = x.double(), tr.double()
    rf = _ref(xs, trs, graph, il, 5, 4.0, LW, TS)
    _compare(_full(xs, trs, graph, il, 5, 4.0, LW, TS), rf, torch.float64, "5j after window calls")
    _results(s, ref, "the window stream after the older routes")
