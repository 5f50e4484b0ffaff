"""GPU tests (-m gpu) of the n best hypotheses of the two token-graph beam streams (`BeamStream.result_nbest`,
`BeamWindowStream.result_nbest`, csrc/asg_beam_nbest.hip over a state): for every way of cutting utterances into chunks the final
list is, bit for bit, the device's own `beam_decode_graph_nbest` and the restatement's (tests/beam_stream_nbest_ref.py), the
prefix list the restatement's after every chunk; the sort's padding, the walker's strips, the collapse's frame blocks; beams that
empty, the clamp at max_frames, masked reset; the window's tails through a ring that wraps, with an empty tail, after forced
commits and at their longest; capture and replay; determinism; the state and the older routes left as they were.  Bytes are
compared everywhere: the same adds in the same order."""
import numpy as np
import pytest
import torch

from beam_stream_nbest_ref import stream_nbest, window_nbest
from beam_stream_ref import BeamStreamRef
from beam_window_ref import BeamWindowRef, chain_automaton, two_component_emissions, two_components_automaton
from test_hip_beam_stream import _Q, _case, _ngram, _ragged_schedule, _ref_stream, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
LW, TS = 0.8, -0.5
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
NP = {torch.float32: np.float32, torch.float64: np.float64}
STREAM = ("scores", "graph_scores", "tokens", "token_lengths", "num_hyps", "path", "states", "frames", "status")
WINDOW = ("scores", "tokens", "token_lengths", "num_hyps", "path", "states", "frames", "committed", "status")


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _nb(s, nbest, final, align=True):
    out = s.result_nbest(nbest, final, align)
    torch.cuda.synchronize()
    assert type(out).__name__ == ("BeamStreamNbest" if isinstance(s, _asg().BeamStream) else "BeamWindowNbest")
    return out._fields, [None if o is None else o.cpu().numpy() for o in out]


def _same(got, want, what, align=True):
    """Every array bit for bit (array_equal would let -0 pass for +0)."""
    names, got = got
    assert names in (STREAM, WINDOW) and len(got) == len(want) == 9
    for n, g, w in zip(names, got, want):
        if n in ("path", "states") and not align:
            assert g is None, (n, what)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (n, what)
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), "%s %s" % (n, what)


def _same_as_one_shot(got, one, T, what):
    """The stream's final list over max_frames >= T columns against beam_decode_graph_nbest's over T columns."""
    names, got = got
    got, one = dict(zip(names, got)), dict(zip(one._fields, [o.cpu().numpy() for o in one]))
    for n in ("scores", "graph_scores", "token_lengths", "num_hyps"):
        assert got[n].dtype == one[n].dtype and got[n].tobytes() == one[n].tobytes(), "%s %s" % (n, what)
    for n in ("tokens", "path", "states"):
        assert got[n].dtype == np.int64 and got[n].shape[-1] >= T, what
        assert np.array_equal(got[n][..., :T], one[n]) and (got[n][..., T:] == -1).all(), "%s %s" % (n, what)


def _chunks(name, x, il, ragged):
    """The (chunk, lengths) of a chunking, on the host: cuts of the utterances, or calls of 7 frames of which every slot takes
    a number of its own."""
    T, B, N = x.shape
    if name == "ragged":
        pad = torch.cat([x, torch.zeros(7, B, N, dtype=x.dtype)])
        for pos, n in ragged:
            yield torch.stack([pad[int(pos[b]):int(pos[b]) + 7, b] for b in range(B)], 1), n
    else:
        cuts = {"ones": list(range(T + 1)), "whole": [0, T], "1-7-0-16": [0, 1, 8, 8, 24]}[name]
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            yield x[t0:t1], (il - t0).clamp(0, t1 - t0)


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "random"])
@DTYPES
def test_any_chunking_against_the_one_shot_nbest_and_every_prefix_list(dtype, integer):
    A = _asg()
    # integer scores over equal weights (every edge costs token_score alone): the ends tie, and the rows are in q order
    graph = A.TokenGraph.from_ngram(np.zeros((7, 7))) if integer else _ngram(6, 3, 3, holes=True)
    Q = _Q(graph)
    T, B, N = 24, 5, 6
    x, tr, il = _case(T, B, N, 11, dtype, integer)
    assert il[0] == T and il[1] == 0 and il[2] == 1
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    ragged = _ragged_schedule(il, 7, 5)
    assert len(ragged) > 3 and any(len(set(n.tolist())) > 2 for _, n in ragged)
    most, padded, tied, fewer = 0, False, 0, 0
    for K in (1, 3, 8, Q):
        nbests = sorted({1, 2, K, K + 5})
        for theta in (INF, 2.0, 0.0):
            ones = {nb: A.beam_decode_graph_nbest(xd, trd, graph, ild, K, nb, theta, LW, TS, return_alignments=True) for nb in nbests}
            for name in ("ones", "whole", "1-7-0-16", "ragged"):
                M = max(T + 2, 7 * len(ragged)) if name == "ragged" else T + 2      # (the host counts the Tc it was offered)
                s, ref = _stream(tr, graph, B, M, K, theta), _ref_stream(tr, graph, B, M, K, theta)
                for chunk, n in _chunks(name, x, il, ragged):
                    s.advance(chunk.to(DEV), n.to(DEV))
                    ref.advance(chunk.numpy(), n.numpy())
                    for nb in nbests:                                # the n best prefixes after every chunk
                        want = stream_nbest(ref, nb, False)
                        _same(_nb(s, nb, False), want, "prefix K=%d theta=%s nbest=%d %s" % (K, theta, nb, name))
                        fewer += int((stream_nbest(ref, nb, True)[4] < want[4]).sum())
                for nb in nbests:
                    what = "final K=%d theta=%s nbest=%d %s" % (K, theta, nb, name)
                    want = stream_nbest(ref, nb, True)
                    sc, nh = want[0], want[4]
                    assert nh[1] == 0 and (nh <= min(nb, K)).all() and np.array_equal(want[7], il.numpy()), what
                    most, padded = max(most, int(nh.max())), padded or bool((nh < nb).any())
                    tied += sum(int((sc[b, 1:nh[b]] == sc[b, :max(nh[b] - 1, 0)]).sum()) for b in range(B))
                    got = _nb(s, nb, True)
                    _same(got, want, what)
                    _same_as_one_shot(got, ones[nb], T, what)
    # the regime, from the restatement: lists of several rows, padding rows, fewer final rows than prefixes, and ties
    assert most > 2 and padded and (tied > 10 if integer else fewer > 0)


@DTYPES
@pytest.mark.parametrize("n", [63, 64, 65])
def test_sort_padding(n, dtype):
    """A dense bigram over n tokens has n product states, all accepting: the stored set holds n candidates, one below, at and
    one above the power of two the sort pads to (the construction of tests/test_hip_beam_nbest.py)."""
    A = _asg()
    graph = _ngram(n, 2, 20 + n)
    x, tr, _ = _case(4, 2, n, 21, dtype)
    il = torch.tensor([4, 3])
    s, ref = _stream(tr, graph, 2, 5, n), _ref_stream(tr, graph, 2, 5, n)
    for t0, t1 in ((0, 1), (1, 4)):
        nn = (il - t0).clamp(0, t1 - t0)
        s.advance(x[t0:t1].to(DEV), nn.to(DEV))
        ref.advance(x[t0:t1].numpy(), nn.numpy())
    for final in (False, True):
        want = stream_nbest(ref, n, final)
        assert (want[4] == n).all()                                  # the regime: exactly n candidates
        _same(_nb(s, n, final), want, "sort padding final=%s" % final)
        _same(_nb(s, n, final, align=False), want, "sort padding, no alignments", align=False)
    one = A.beam_decode_graph_nbest(x.to(DEV), tr.to(DEV), graph, il.to(DEV), n, n, INF, LW, TS, return_alignments=True)
    _same_as_one_shot(_nb(s, n, True), one, 4, "sort padding")


def test_walker_strips():
    """More hypotheses than the workgroup has threads: the walk runs in strips of lanes."""
    A = _asg()
    graph = _ngram(11, 4, 5)
    assert graph.compile_host(np.float32, LW, TS)["Q"] == 1463
    x, tr, _ = _case(4, 2, 11, 23)
    il = torch.tensor([4, 3])
    s, ref = _stream(tr, graph, 2, 4, 1300), _ref_stream(tr, graph, 2, 4, 1300)
    for t0, t1 in ((0, 2), (2, 4)):
        nn = (il - t0).clamp(0, t1 - t0)
        s.advance(x[t0:t1].to(DEV), nn.to(DEV))
        ref.advance(x[t0:t1].numpy(), nn.numpy())
    want = stream_nbest(ref, 1300, True)
    assert (want[4] > 1024).all()
    got = _nb(s, 1300, True)
    _same(got, want, "strips")
    one = A.beam_decode_graph_nbest(x.to(DEV), tr.to(DEV), graph, il.to(DEV), 1300, 1300, INF, LW, TS, return_alignments=True)
    _same_as_one_shot(got, one, 4, "strips")
    _same(_nb(s, 1300, False), stream_nbest(ref, 1300, False), "strips, prefixes")


@DTYPES
def test_frame_blocks(dtype):
    """max_frames = 130 with 63 / 64 / 65 / 129 frames: the collapse works in blocks of 64 frames."""
    graph = _ngram(6, 2, 12)
    M, B = 130, 4
    x, tr, _ = _case(M, B, 6, 31, dtype)
    tr = torch.zeros_like(tr)                                        # nothing holds a label: tokens change all along the blocks
    il = torch.tensor([63, 64, 65, 129])
    s, ref = _stream(tr, graph, B, M, 4), _ref_stream(tr, graph, B, M, 4)
    for t0, t1 in ((0, 40), (40, 64), (64, 65), (65, 130)):
        nn = (il - t0).clamp(0, t1 - t0)
        s.advance(x[t0:t1].to(DEV), nn.to(DEV))
        ref.advance(x[t0:t1].numpy(), nn.numpy())
    for final in (True, False):
        want = stream_nbest(ref, 4, final)
        last = want[5][3]                                            # (paths whose tokens begin behind the first block)
        assert (want[4] == 4).all() and want[7].tolist() == il.tolist() and (last[:, 65:129] != last[:, 64:128]).any()
        _same(_nb(s, 4, final), want, "frame blocks final=%s" % final)
        _same(_nb(s, 4, final, align=False), want, "frame blocks, no alignments", align=False)


@DTYPES
def test_a_beam_that_empties_inside_a_chunk(dtype):
    graph = _ngram(6, 2, 7)
    T, B, K = 12, 2, 3
    x, tr, _ = _case(T, B, 6, 17, dtype)
    x[5] = -INF                                                      # nothing survives frame 5
    il = torch.tensor([T, 4])
    s, ref = _stream(tr, graph, B, T, K), _ref_stream(tr, graph, B, T, K)
    for t0, t1 in ((0, 3), (3, 9), (9, 12)):
        nn = (il - t0).clamp(0, t1 - t0)
        s.advance(x[t0:t1].to(DEV), nn.to(DEV))
        ref.advance(x[t0:t1].numpy(), nn.numpy())
        for final in (False, True):
            _same(_nb(s, 4, final), stream_nbest(ref, 4, final), "after frame %d final=%s" % (t1, final))
    want = stream_nbest(ref, 4, False)
    assert want[4].tolist() == [0, K] and want[7].tolist() == [T, 4] and (want[0][0] == -INF).all()


def test_frames_beyond_max_frames_through_replays_and_a_masked_reset():
    """The host refuses chunks beyond max_frames, but not the replays of a captured advance: M + 1 replays of a one-frame advance
    overflow slot 0 (status 1) while slot 1, which skipped the first, reaches max_frames exactly.  Then a masked reset in
    mid-stream.  The state is byte-equal before and after every result_nbest."""
    graph = _ngram(6, 2, 13)
    M, B, N, K = 9, 2, 6, 3
    x, tr, _ = _case(M + 1, B, N, 41)
    s, ref = _stream(tr, graph, B, M, K), _ref_stream(tr, graph, B, M, K)
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
        take = torch.tensor([1, 1 if t >= 1 else 0])
        buf.copy_(x[t:t + 1])
        n.copy_(take)
        gr.replay()
        ref.advance(x[t:t + 1].numpy(), take.numpy())
    for final in (False, True):
        want = stream_nbest(ref, 5, final)
        assert want[7].tolist() == [M, M] and want[8].tolist() == [1, 0]
        before = s._state.clone()
        _same(_nb(s, 5, final), want, "overflow final=%s" % final)
        torch.cuda.synchronize()
        assert torch.equal(before, s._state), "result_nbest wrote to the state"
    mask = torch.tensor([False, True])
    s.reset(mask.to(DEV))
    ref.reset(mask.numpy())
    want = stream_nbest(ref, 5, False)
    assert want[7].tolist() == [M, 0] and want[4][1] == 0 and want[8].tolist() == [1, 0]
    _same(_nb(s, 5, False), want, "after the masked reset")
    s.advance(x[:3].to(DEV), torch.tensor([0, 3], device=DEV))      # slot 1 starts a new utterance
    ref.advance(x[:3].numpy(), np.array([0, 3]))
    for final in (False, True):
        _same(_nb(s, 5, final), stream_nbest(ref, 5, final), "the new utterance final=%s" % final)


# ---- the window
def _win(nxt, w, f, start, tr, B, W, P, K, ts=TS):
    graph = _asg().TokenGraph(nxt, w, f, start=start)
    s = _asg().BeamWindowStream(tr.to(DEV), graph, B, W, P, K, INF, LW, ts, dtype=tr.dtype)
    ref = BeamWindowRef(tr.numpy(), nxt, w, f, start, B, W, P, K, INF, LW, ts, NP[tr.dtype])
    plain = _asg().BeamStream(tr.to(DEV), graph, B, 64, K, INF, LW, ts, dtype=tr.dtype)
    return s, ref, plain


def _window_cases(T, B, dtype):
    g = _ngram(6, 2, 12)
    x, tr, _ = _case(T, B, 6, 71, dtype)
    yield "bigram", (g.next, g.weight, g.final, g.start), x, tr, 4, TS
    x, tr, _ = _case(T, B, 5, 72, dtype)
    yield "chain", chain_automaton(T + 2, 5), x, tr, 1, TS          # K = 1: every attempt commits up to pos - 1
    x = torch.from_numpy(two_component_emissions(T, B, 6, NP[dtype]))
    yield "two", two_components_automaton(6) + (0,), x, torch.zeros(6, 6, dtype=dtype), 4, -1.0


@DTYPES
@pytest.mark.parametrize("WP", [(8, 2), (16, 4), (5, 5)])
def test_window_tails_after_every_chunk(WP, dtype):
    """pos far beyond W, so that the tail wraps the end of the ring; a tail that is empty (the chain with K = 1); rows after
    forced commits (the two components); scores equal to a BeamStream fed the same chunks; the state left alone."""
    W, P = WP
    T, B, nb = 64, 3, 6
    cuts = [0, 1, 7, 7, 16, 24, 29, 30, 47, 64]
    seen = dict(wrapped=0, empty_tail=0, forced=0, clear=0, rows=0)
    for name, auto, x, tr, K, ts in _window_cases(T, B, dtype):
        s, ref, plain = _win(*auto, tr, B, W, P, K, ts)
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            s.advance(x[t0:t1].to(DEV))
            plain.advance(x[t0:t1].to(DEV))
            ref.advance(x[t0:t1].numpy())
            for final in (False, True):
                what = "%s W=%d P=%d after frame %d final=%s" % (name, W, P, t1, final)
                want = window_nbest(ref, nb, final)
                for b, v in enumerate(ref.slots):                    # the regime, from the restatement
                    if want[3][b]:
                        seen["wrapped"] += int(v.base % W > (v.pos - 1) % W and v.pos > v.base)
                        seen["empty_tail"] += int(v.base == v.pos)
                        seen["forced" if v.status & 1 else "clear"] += 1
                        seen["rows"] += int(want[3][b] > 1)
                before = s._state.clone()
                got = _nb(s, nb, final)
                _same(got, want, what)
                _same(_nb(s, nb, final, align=False), want, what, align=False)
                assert torch.equal(before, s._state), "result_nbest wrote to the state"
                sc = plain.result_nbest(nb, final).scores.cpu().numpy()
                assert got[1][0].tobytes() == sc.tobytes(), "scores of the stream " + what
        if name == "chain":
            assert seen["empty_tail"] > 0
        if name == "two":
            assert seen["forced"] > 0
    # (with P == W every attempt commits everything, base is a multiple of W and a tail never passes the end of the ring)
    assert all(v > 0 for k, v in seen.items() if k != "wrapped" or P < W), seen


@DTYPES
@pytest.mark.parametrize("W", [64, 65, 66])
def test_the_longest_tail(W, dtype):
    """P = 1 and two components that never converge: after every attempt pos - base <= W - P, and no frame follows before the
    next one, so W - 1 frames -- 63, 64, 65: below, at and above a block of the collapse -- is the longest tail a call can meet
    (a tail of exactly W frames exists only inside advance, between a frame and its attempt)."""
    T, B = W + 9, 2
    x = torch.from_numpy(two_component_emissions(T, B, 6, NP[dtype]))
    s, ref, _ = _win(*two_components_automaton(6), 0, torch.zeros(6, 6, dtype=dtype), B, W, 1, 4, -1.0)
    for t0, t1 in ((0, W - 1), (W - 1, W), (W, T)):
        s.advance(x[t0:t1].to(DEV))
        ref.advance(x[t0:t1].numpy())
        assert all(v.pos - v.base == W - 1 for v in ref.slots)
        for final in (False, True):
            want = window_nbest(ref, 4, final)
            assert (want[3] >= 2).all()
            _same(_nb(s, 4, final), want, "W=%d after frame %d final=%s" % (W, t1, final))


# ---- both streams
def _replayed(s, ref, want_of, x, Tc, final):
    """Capture result_nbest once; three times: advance on a fresh chunk (captured too the first time round, eager after), replay
    the result, and compare what the captured call left in its outputs with the restatement."""
    B, N = x.shape[1], x.shape[2]
    buf = torch.zeros(Tc, B, N, device=DEV, dtype=x.dtype)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.advance(buf[:0])                                           # warm-ups: no frame, and the scratch of nbest = 3
        s.result_nbest(3, final, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ga, gr = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(ga):
        s.advance(buf)
    with torch.cuda.graph(gr):
        out = s.result_nbest(3, final, True)
    s.reset()                                                        # (the captures themselves ran nothing)
    for c in range(3):
        chunk = x[c * Tc:(c + 1) * Tc]
        if c == 0:
            buf.copy_(chunk)
            ga.replay()
        else:
            s.advance(chunk.to(DEV))
        ref.advance(chunk.numpy())
        gr.replay()
        torch.cuda.synchronize()
        _same((out._fields, [o.cpu().numpy() for o in out]), want_of(ref, 3, final), "replay %d final=%s" % (c, final))


@pytest.mark.parametrize("final", [False, True])
def test_capture_and_replay(final):
    graph = _ngram(8, 3, 9)
    Tc, B, K, theta = 4, 3, 12, 6.0
    x, tr, _ = _case(3 * Tc, B, 8, 53)
    _replayed(_stream(tr, graph, B, 3 * Tc, K, theta), _ref_stream(tr, graph, B, 3 * Tc, K, theta), stream_nbest, x, Tc, final)
    s = _asg().BeamWindowStream(tr.to(DEV), graph, B, 6, 2, K, theta, LW, TS)
    ref = BeamWindowRef(tr.numpy(), graph.next, graph.weight, graph.final, graph.start, B, 6, 2, K, theta, LW, TS, np.float32)
    _replayed(s, ref, window_nbest, x, Tc, final)


def test_two_runs_give_identical_bits_and_the_older_routes_are_unchanged():
    A = _asg()
    graph = _ngram(6, 3, 3, holes=True)
    T, B = 16, 4
    x, tr, il = _case(T, B, 6, 61)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)

    def older(s, w):
        outs = list(s.result(True)) + list(w.result(False)) + list(A.beam_decode_graph(xd, trd, graph, ild, 5, 4.0, LW, TS))
        outs += list(A.beam_decode_graph_nbest(xd, trd, graph, ild, 5, 3, 4.0, LW, TS, return_alignments=True))
        outs += [o for o in A.beam_decode_graph_nbest_confidence(xd, trd, graph, ild, 5, 3, 4.0, LW, TS, True, 1) if o is not None]
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]
    runs = []
    for _ in range(2):
        s = _stream(tr, graph, B, T, 5, 4.0)
        w = A.BeamWindowStream(trd, graph, B, 8, 2, 5, 4.0, LW, TS)
        for t0, t1 in ((0, 7), (7, 16)):
            nn = (il - t0).clamp(0, t1 - t0).to(DEV)
            s.advance(xd[t0:t1], nn)
            w.advance(xd[t0:t1], nn)
        before = older(s, w)
        mine = [o for z in (s, w) for final in (False, True) for o in _nb(z, 4, final)[1]]
        after = older(s, w)
        assert len(before) == len(after) and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        runs.append(mine)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    ref = _ref_stream(tr, graph, B, T, 5, 4.0)
    ref.advance(x.numpy(), il.numpy())
    for final, at in ((False, 0), (True, 9)):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][at:at + 9], stream_nbest(ref, 4, final)))
