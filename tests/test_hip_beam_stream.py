"""GPU tests (-m gpu) of streaming beam decoding (`torch_asg_amd.BeamStream`, csrc/asg_beam_stream.hip): for every way of
cutting utterances into chunks the final result is, bit for bit, the one-shot decode of the restatement
(tests/beam_decode_ref.py) and of the device's own `beam_decode_graph`; beams that empty inside a chunk and at a chunk
boundary; both transition layouts; the lane groups of the expansion; the frame blocks of the token collapse; partial results
against the streaming restatement (tests/beam_stream_ref.py); the clamp at max_frames; masked reset; capture and replay;
determinism; errors; and the older beam routes after streaming calls."""
import numpy as np
import pytest
import torch

from beam_decode_ref import beam_decode_ref
from beam_stream_ref import BeamStreamRef
from beam_window_ref import chain_automaton

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


def _one_shot(x, tr, graph, il, K, theta, sizes=None):
    return beam_decode_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start,
                           None if il is None else il.numpy(), K, theta, LW, TS, sizes=sizes)


def _stream(tr, graph, B, M, K, theta=INF):
    return _asg().BeamStream(tr.to(DEV), graph, B, M, K, theta, LW, TS, dtype=tr.dtype)


def _ref_stream(tr, graph, B, M, K, theta=INF):
    return BeamStreamRef(tr.numpy(), graph.next, graph.weight, graph.final, graph.start, B, M, K, theta, LW, TS, NP[tr.dtype])


def _feed(s, xd, il, cuts):
    """Advance by the chunks x[t0:t1] of consecutive cuts; slot b takes the frames below il[b]."""
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        s.advance(xd[t0:t1], None if il is None else (il - t0).clamp(0, t1 - t0).to(DEV))


def _ragged_schedule(il, Tc, seed):
    """Calls that each offer Tc frames of which every slot takes a number of its own, until slot b has taken il[b] frames."""
    g = torch.Generator().manual_seed(seed)
    pos, calls = torch.zeros_like(il), []
    while bool((pos < il).any()):
        n = torch.minimum(torch.randint(0, Tc + 1, (il.numel(),), generator=g), il - pos)
        calls.append((pos.clone(), n))
        pos = pos + n
    return calls


def _feed_ragged(s, x, calls, Tc):
    """The slots drift apart inside one chunk shape: slot b's part of a chunk starts at its own frame."""
    T, B, N = x.shape
    pad = torch.cat([x, torch.zeros(Tc, B, N, dtype=x.dtype)])
    for pos, n in calls:
        chunk = torch.stack([pad[int(pos[b]):int(pos[b]) + Tc, b] for b in range(B)], 1)
        s.advance(chunk.to(DEV), n.to(DEV))


def _res(s, final=True):
    out = s.result(final)
    torch.cuda.synchronize()
    assert type(out).__name__ == "BeamStreamResult"
    return [o.cpu().numpy() for o in out]


def _same(got, want, what):
    """Every array bit for bit (array_equal would let -0 pass for +0)."""
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (i, what)
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), "output %d %s" % (i, what)


def _same_as_one_shot(res, one, T, what):
    """res over max_frames >= T columns against the one-shot decode over T columns."""
    assert res[0].dtype == one[0].dtype and res[0].tobytes() == one[0].tobytes(), "scores " + what
    assert res[3].dtype == np.int64 and res[3].tobytes() == one[3].tobytes(), "token_lengths " + what
    for i in (1, 2, 4):
        assert res[i].dtype == np.int64 and res[i].shape[1] >= T, what
        assert np.array_equal(res[i][:, :T], one[i]) and (res[i][:, T:] == -1).all(), "output %d %s" % (i, what)


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "random"])
@DTYPES
def test_any_chunking_equals_the_one_shot_decode(dtype, integer):
    graph = _ngram(6, 3, 3, holes=True)
    Q = _Q(graph)
    T, B, N = 24, 5, 6
    x, tr, il = _case(T, B, N, 11, dtype, integer)
    assert il[0] == T and il[1] == 0 and il[2] == 1
    xd = x.to(DEV)
    cuts = {"ones": list(range(T + 1)), "whole": [0, T], "1-7-0-16": [0, 1, 8, 8, 24]}
    ragged = _ragged_schedule(il, 7, 5)
    assert len(ragged) > 3 and any(len(set(n.tolist())) > 2 for _, n in ragged)
    for K in (1, 3, 8, Q):
        for theta in (INF, 2.0, 0.0):
            one = _one_shot(x, tr, graph, il, K, theta)
            for name in list(cuts) + ["ragged"]:
                # (the host counts the Tc it was offered, not the frames a slot took: the ragged calls need that much room)
                s = _stream(tr, graph, B, max(T + 2, 7 * len(ragged)) if name == "ragged" else T + 2, K, theta)
                if name == "ragged":
                    _feed_ragged(s, x, ragged, 7)
                else:
                    _feed(s, xd, il, cuts[name])
                res = _res(s)
                what = "K=%d theta=%s %s" % (K, theta, name)
                _same_as_one_shot(res, one, T, what)
                assert np.array_equal(res[5], il.numpy()) and not res[6].any(), what
    s = _stream(tr, graph, B, T, 8)                                 # chunk_lengths None: every slot takes the whole chunk
    _feed(s, xd, None, [0, 5, 24])
    _same_as_one_shot(_res(s), _one_shot(x, tr, graph, None, 8, INF), T, "no lengths")


@DTYPES
def test_a_beam_that_empties_inside_a_chunk_and_at_a_boundary(dtype):
    graph = _ngram(6, 2, 7)
    T, B, N, K = 12, 2, 6, 3
    x, tr, _ = _case(T, B, N, 17, dtype)
    x[5] = -INF                                                     # nothing survives frame 5
    il = torch.tensor([T, 4])
    ref = _ref_stream(tr, graph, B, T, K)
    ref.advance(x.numpy(), il.numpy())
    assert ref.sizes()[0][4] > 0 and ref.sizes()[0][5:] == [0] * 7 and min(ref.sizes()[1]) > 0
    one = _one_shot(x, tr, graph, il, K, INF)
    assert one[0][0] == -INF and one[0][1] > -INF
    xd = x.to(DEV)
    for cuts in ([0, 3, 9, 12],                                     # frame 5 inside the chunk 3..9
                 [0, 5, 6, 12],                                     # ... the first frame of a chunk, the set full at the boundary
                 [0, 6, 12]):                                       # ... the last frame of a chunk, the set empty at the boundary
        s = _stream(tr, graph, B, T, K)
        _feed(s, xd, il, cuts)
        res = _res(s)
        _same_as_one_shot(res, one, T, str(cuts))
        assert res[5].tolist() == [T, 4]                            # the frames behind the empty set are consumed all the same
        _same(_res(s, final=False), ref.result(False), str(cuts))


def test_both_transition_layouts():
    """The transitions sit in LDS while they fit beside the beam (4096 + K*(e+4) + 8 + N*N*e <= 160 KiB) and are read from
    global memory beyond: float64 and K = 8 put the last N in LDS at 141."""
    lds = lambda N, K=8, e=8: 4096 + K * (e + 4) + 8 + N * N * e
    assert lds(141) <= 160 * 1024 < lds(142) and lds(141) > 64 * 1024
    for N in (141, 142):
        graph = _ngram(N, 2, N)
        T, B = 6, 2
        x, tr, il = _case(T, B, N, 23, torch.float64)
        il[1] = 3
        one = _one_shot(x, tr, graph, il, 8, 3.0)
        assert (one[0] > -INF).all()
        s = _stream(tr, graph, B, T, 8, 3.0)
        _feed(s, x.to(DEV), il, [0, 1, 4, 6])
        _same_as_one_shot(_res(s), one, T, "N=%d" % N)


def test_lanes_per_state():
    """K = 1: 64 lanes share a state's outgoing row; K >= 1024: one lane per state, and a strip of 1024 states per pass."""
    graph = _ngram(32, 3, 9)
    Q = _Q(graph)
    assert 1024 < Q < 1100
    T, B = 8, 2
    x, tr, il = _case(T, B, 32, 29)
    il[1] = 5
    xd = x.to(DEV)
    for K, theta in ((1, INF), (1024, INF), (1024, 6.0)):
        sizes = []
        one = _one_shot(x, tr, graph, il, K, theta, sizes)
        if K == 1024 and theta == INF:
            assert max(sizes[0]) == 1024                            # the beam is full and cuts
        s = _stream(tr, graph, B, T, K, theta)
        _feed(s, xd, il, [0, 3, 4, 8])
        _same_as_one_shot(_res(s), one, T, "K=%d theta=%s" % (K, theta))


def test_collapse_over_frame_blocks():
    graph = _ngram(6, 2, 12)
    M, B = 130, 4
    x, tr, _ = _case(M, B, 6, 31)
    tr = torch.zeros_like(tr)                                       # nothing holds a label: tokens change all along the blocks
    il = torch.tensor([63, 64, 65, 129])
    one = _one_shot(x, tr, graph, il, 4, INF)
    p = one[1][3]
    assert (one[3] >= 9).all() and (p[1:64] != p[:63]).any() and (p[65:128] != p[64:127]).any()      # tokens in every block
    s = _stream(tr, graph, B, M, 4)
    _feed(s, x.to(DEV), il, [0, 40, 64, 65, 130])
    res = _res(s)
    _same_as_one_shot(res, one, M, "blocks of 64 frames")
    assert res[5].tolist() == il.tolist()


@DTYPES
def test_partial_results_after_every_chunk(dtype):
    graph = _ngram(6, 3, 3, holes=True)
    T, B, K, theta = 18, 3, 4, 3.0
    x, tr, il = _case(T, B, 6, 37, dtype)
    il = torch.tensor([T, 7, 12])
    s, ref = _stream(tr, graph, B, T, K, theta), _ref_stream(tr, graph, B, T, K, theta)
    _same(_res(s, False), ref.result(False), "before the first frame")
    cuts = [0, 1, 2, 6, 6, 11, 18]
    xd = x.to(DEV)
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        n = (il - t0).clamp(0, t1 - t0)
        s.advance(xd[t0:t1], n.to(DEV))
        ref.advance(x[t0:t1].numpy(), n.numpy())
        for final in (False, True, False):                           # a result changes nothing
            _same(_res(s, final), ref.result(final), "after frame %d final=%s" % (t1, final))
    _same_as_one_shot(_res(s), _one_shot(x, tr, graph, il, K, theta), T, "the end")


def test_max_frames_reached_exactly_then_one_more_frame():
    """The host refuses chunks beyond max_frames (test_errors), but it does not see the replays of a captured advance: there
    the device's clamp and `status` are the guarantee.  M + 1 replays of a one-frame advance: slot 0 takes a frame at every
    replay -- one too many --, slot 1 skips the first and reaches max_frames exactly."""
    graph = _ngram(6, 2, 13)
    M, B, N, K = 9, 2, 6, 3
    x, tr, _ = _case(M + 1, B, N, 41)
    s = _stream(tr, graph, B, M, K)
    buf = torch.zeros(1, B, N, device=DEV)
    n = torch.zeros(B, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.advance(buf, n)                                            # warm-up; n = 0: the state stays as it is
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        s.advance(buf, n)
    for t in range(M + 1):
        buf.copy_(x[t:t + 1])
        n.copy_(torch.tensor([1, 1 if t >= 1 else 0]))
        gr.replay()
        if t == M - 1:
            res = _res(s)
            assert res[5].tolist() == [M, M - 1] and res[6].tolist() == [0, 0]
    res = _res(s)
    assert res[5].tolist() == [M, M] and res[6].tolist() == [1, 0]
    for b, utt in enumerate((x[:M], x[1:M + 1])):                    # slot 0: its first max_frames frames
        one = _one_shot(utt[:, b:b + 1], tr, graph, None, K, INF)
        _same_as_one_shot([r[b:b + 1] for r in res[:5]], one, M, "slot %d" % b)
    s.reset(torch.tensor([True, False], device=DEV))
    assert _res(s)[6].tolist() == [0, 0]


def test_masked_reset_mid_stream():
    graph = _ngram(6, 3, 3, holes=True)
    T, B, K, theta = 14, 2, 4, 5.0
    x, tr, _ = _case(T, B, 6, 43)
    y, _, _ = _case(T, B, 6, 44)
    s = _stream(tr, graph, B, T, K, theta)
    s.advance(x[:6].to(DEV))
    s.reset(torch.tensor([False, True], device=DEV))
    mixed = x[6:].clone()
    mixed[:, 1] = y[:T - 6, 1]                                       # slot 1 starts a new utterance, slot 0 goes on
    s.advance(mixed.to(DEV))
    res = _res(s)
    assert res[5].tolist() == [T, T - 6] and res[6].tolist() == [0, 0]
    want_x = _one_shot(x, tr, graph, None, K, theta)
    want_y = _one_shot(y[:T - 6], tr, graph, None, K, theta)
    for b, (want, L) in enumerate(((want_x, T), (want_y, T - 6))):
        _same_as_one_shot([r[b:b + 1] for r in res[:5]], [w[b:b + 1] for w in want], L, "slot %d" % b)
    s.reset(torch.tensor([1, 0], dtype=torch.int32))                 # an integer mask from the host
    res = _res(s)
    assert res[5].tolist() == [0, T - 6] and res[0][0] == -INF and res[0][1] > -INF
    s.reset()
    assert _res(s)[5].tolist() == [0, 0]


def test_masked_reset_of_a_used_slot_beyond_one_pass_of_the_reset():
    """The reset shares the Q entries of val / arg among 64 workgroups of 256 threads: 16384 per pass.  A chain of Q a little
    above that, walked down from its last state, keeps the search in the product states of the SECOND pass.  Slot 0 decodes,
    is reset under a mask and decodes other emissions; every output of every call against the streaming restatement
    (tests/beam_stream_ref.py), byte for byte.  A frame empties the entries it touched, so what fails when entries >= 16384
    are not cleared (or are cleared at a wrong offset) is the constructor's reset of the freshly allocated, poisoned state;
    the masked reset of the used slot is checked for its header and for leaving slot 1 alone."""
    S, N = 3290, 5
    graph = _asg().TokenGraph(*chain_automaton(S, N))
    h = graph.compile_host(np.float32, LW, TS)
    T, B, K = 6, 2, 4
    assert 16384 < h["Q"] < 16384 + 128 and np.nonzero(h["state"] >= S - 1 - T)[0].min() >= 16384
    x, tr, _ = _case(T, B, N, 61)
    y, _, _ = _case(T, B, N, 62)
    s, ref = _stream(tr, graph, B, 2 * T, K), _ref_stream(tr, graph, B, 2 * T, K)

    def both(z, what):
        for t0, t1 in ((0, 2), (2, T)):
            s.advance(z[t0:t1].to(DEV))
            ref.advance(z[t0:t1].numpy())
            for final in (False, True):
                _same(_res(s, final), ref.result(final), "%s after frame %d final=%s" % (what, t1, final))
    both(x, "the first utterance")
    st = ref.result(True)[4]
    assert (ref.result(True)[0] > -INF).all() and st[st >= 0].min() >= S - 1 - T        # the states the search used
    mask = torch.tensor([True, False])
    s.reset(mask.to(DEV))
    ref.reset(mask.numpy())
    for final in (False, True):
        _same(_res(s, final), ref.result(final), "after the masked reset final=%s" % final)
    both(y, "the second utterance")                                  # slot 0 from its start, slot 1 goes on down the chain
    assert ref.result(True)[5].tolist() == [T, 2 * T]


@DTYPES
def test_against_the_devices_own_one_shot_decoder(dtype):
    A = _asg()
    graph = _ngram(12, 3, 21, holes=True)
    T, B = 40, 6
    x, tr, il = _case(T, B, 12, 47, dtype)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    loss = A.ASGLoss(12).to(DEV).to(dtype)
    with torch.no_grad():
        loss.transition.copy_(trd)
    for K, theta in ((16, INF), (64, 4.0)):
        want = [o.cpu().numpy() for o in A.beam_decode_graph(xd, trd, graph, ild, K, theta, LW, TS)]
        s = loss.beam_stream(graph, B, T, K, theta, LW, TS)           # the module method
        _feed(s, xd, il, [0, 8, 16, 17, 40])
        _same_as_one_shot(_res(s), want, T, "K=%d" % K)
    # half precision chunks are widened to the transition's dtype
    if dtype == torch.float32:
        s, r = _stream(tr, graph, B, T, 16), _stream(tr, graph, B, T, 16)
        s.advance(xd[:9].to(torch.bfloat16), ild.clamp(max=9))
        r.advance(xd[:9].to(torch.bfloat16).float(), ild.clamp(max=9))
        _same(_res(s), _res(r), "bfloat16")
        # a strided chunk
        s.reset()
        s.advance(xd.transpose(0, 1).contiguous().transpose(0, 1), ild)
        want = [o.cpu().numpy() for o in A.beam_decode_graph(xd, trd, graph, ild, 16, INF, LW, TS)]
        _same_as_one_shot(_res(s), want, T, "strided")


def test_capture_and_replay():
    graph = _ngram(8, 3, 9)
    Tc, B, N, K, theta = 4, 3, 8, 12, 6.0
    T = 6 * Tc
    x, tr, _ = _case(T, B, N, 53)
    il = torch.tensor([T, 9, T - 2])
    s = _stream(tr, graph, B, T, K, theta)
    buf = torch.zeros(Tc, B, N, device=DEV)
    n = torch.zeros(B, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.advance(buf, n)                                            # warm-up; n = 0: the state stays as it is
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        s.advance(buf, n)
    s.reset()                                                        # (the capture itself ran nothing)
    for c in range(6):
        buf.copy_(x[c * Tc:(c + 1) * Tc])
        n.copy_((il - c * Tc).clamp(0, Tc))
        gr.replay()
    res = _res(s)
    _same_as_one_shot(res, _one_shot(x, tr, graph, il, K, theta), T, "six replays")
    assert res[5].tolist() == il.tolist() and not res[6].any()


def test_two_runs_give_identical_bits():
    graph = _ngram(12, 3, 3, holes=True)
    T, B = 48, 8
    x, tr, il = _case(T, B, 12, 59)
    xd = x.to(DEV)
    runs = []
    for _ in range(2):
        s = _stream(tr, graph, B, T, 50, 8.0)
        _feed(s, xd, il, [0, 16, 32, 48])
        runs.append(_res(s) + _res(s, False))
    _same(runs[0], runs[1], "two runs")


def test_errors():
    A = _asg()
    graph = _ngram(5, 2, 10)
    tr = torch.randn(5, 5, device=DEV)
    s = A.BeamStream(tr, graph, 2, 6, 4)
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
        A.BeamStream(tr.double(), graph, 2, 6, 4)                    # not the stream's dtype
    with pytest.raises(RuntimeError):
        A.BeamStream(torch.randn(6, 6, device=DEV), graph, 2, 6, 4)
    s.beam_threshold = -1.0
    with pytest.raises(ValueError):
        s.advance(x)
    s.beam_threshold = INF
    assert _res(s)[5].tolist() == [0, 0]                             # nothing above reached the state
    s.advance(x)
    s.advance(x)
    with pytest.raises(ValueError, match="max_frames"):
        s.advance(x[:1])
    s.advance(x[:0])                                                 # a chunk of no frames is fine
    res = _res(s)
    assert res[5].tolist() == [6, 6] and not res[6].any()
    s.reset()
    s.advance(x)
    assert _res(s)[5].tolist() == [3, 3]


def test_the_older_beam_routes_are_unchanged_after_streaming_calls():
    from beam_loss_cases import _compare, _full, _ref
    from beam_nbest_ref import beam_nbest_ref
    A = _asg()
    graph = _ngram(6, 3, 3, holes=True)
    T, B = 16, 4
    x, tr, il = _case(T, B, 6, 61)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    s = _stream(tr, graph, B, T, 5, 4.0)
    _feed(s, xd, il, [0, 7, 16])
    _res(s)
    one = _one_shot(x, tr, graph, il, 5, 4.0)
    got = [o.cpu().numpy() for o in A.beam_decode_graph(xd, trd, graph, ild, 5, 4.0, LW, TS)]
    _same(got, one, "5i after streaming")
    nb = A.beam_decode_graph_nbest(xd, trd, graph, ild, 5, 3, 4.0, LW, TS, return_alignments=True)
    want = beam_nbest_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start, il.numpy(), 5, 3, 4.0, LW, TS)
    _same([o.cpu().numpy() for o in nb], want, "5k after streaming")
    xs, trs = x.double(), tr.double()
    ref = _ref(xs, trs, graph, il, 5, 4.0, LW, TS)
    _compare(_full(xs, trs, graph, il, 5, 4.0, LW, TS), ref, torch.float64, "5j after streaming")
    _same_as_one_shot(_res(s), one, T, "the stream after the older routes")
