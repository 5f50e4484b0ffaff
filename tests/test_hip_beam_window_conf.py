"""GPU tests (-m gpu) of the lattice-keeping window stream (`torch_asg_amd.BeamWindowStream(..., keep_lattice=True)`;
csrc/asg_beam_conf_window.hip).  The five plain outputs of `advance`, `result`, `result_nbest` and `reset` are
held BYTE FOR BYTE to a plain `BeamWindowStream` fed the same chunks; the start frames and confidences of the committed tokens
BIT FOR BIT to the device's own `BeamStream(keep_lattice=True)`, advanced frame by frame and asked at every multiple of the commit
period, while status bit 0 is clear; every value, forced commits included, to the numpy restatement
tests/beam_window_conf_ref.py under tests/test_hip_beam_conf.py's rule (float64 rtol = atol = 1e-9, float32 util.assert_close,
frames and padding exact); the `final=True` tail with the commits to the device's `beam_decode_graph_confidence`."""
import numpy as np
import pytest
import torch

from beam_window_conf_ref import BeamWindowConfRef
from beam_window_ref import chain_automaton, two_component_emissions, two_components_automaton
from util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
LW, TS = 0.7, -0.3
NP = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _ngram(N, order, seed, holes=False):
    rng = np.random.default_rng(seed)
    lp = np.log(rng.dirichlet(np.ones(N + 1), size=(N + 1,) * (order - 1))) if order > 1 else np.log(rng.dirichlet(np.ones(N + 1)))
    if holes:
        lp[rng.random(size=lp.shape) < 0.2] = -np.inf
    return _asg().TokenGraph.from_ngram(lp)


def _case(T, B, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g, dtype=torch.float64), -1).to(dtype)
    tr = (0.5 * torch.randn(N, N, generator=g, dtype=torch.float64)).to(dtype)
    il = torch.randint(2, T + 1, (B,), generator=g)
    il[0] = T
    if B > 1:
        il[1] = 0
    if B > 2:
        il[2] = 1
    return x, tr, il


def _window(tr, graph, B, W, P, K, tol=0, C=None, theta=INF, keep=True, w=(LW, TS)):
    kw = dict(keep_lattice=True, frame_tolerance=tol, max_chunk=C) if keep else {}
    return _asg().BeamWindowStream(tr.to(DEV), graph, B, W, P, K, theta, *w, dtype=tr.dtype, **kw)


def _ref(tr, graph, B, W, P, K, tol=0, C=None, theta=INF, w=(LW, TS)):
    return BeamWindowConfRef(tr.numpy(), graph.next, graph.weight, graph.final, graph.start, B, W, P, K, theta, *w, NP[tr.dtype],
                             tol, C)


def _grow(tr, graph, B, M, K, theta=INF, w=(LW, TS)):
    return _asg().BeamStream(tr.to(DEV), graph, B, M, K, theta, *w, dtype=tr.dtype, keep_lattice=True)


def _host(r):
    return [t.cpu().numpy() for t in r]


def _bytes(r):
    return [a.tobytes() for a in _host(r)]


def _close(got, want, dtype, what):
    assert not np.isnan(got).any(), what
    if dtype == torch.float64:
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9), what
    else:
        assert_close(got, want, what=what)


def _cuts(turn, T, P):
    """5m's six chunkings (chunking 3, the ragged one, is `None`)."""
    return {0: list(range(T + 1)), 1: [0, T], 2: [0, 1, 8, 8, 24, 40], 3: None, 4: list(range(0, T, 3 * P + 1)) + [T],
            5: [0, 0, 20, 20, 40, 40]}[turn % 6]


def _calls(x, il, cuts, C, seed=0):
    """[(chunk, lengths)] for the cuts, every chunk at most C frames long (a cut longer than C is cut again); cuts None: calls
    that offer min(7, C) frames of which every slot takes a number of its own."""
    T, B, N = x.shape
    out = []
    if cuts is None:
        Tc = min(7, C)
        g = torch.Generator().manual_seed(seed)
        pad = torch.cat([x, torch.zeros(Tc, B, N, dtype=x.dtype)])
        pos = torch.zeros_like(il)
        while bool((pos < il).any()):
            n = torch.minimum(torch.randint(0, Tc + 1, (B,), generator=g), il - pos)
            out.append((torch.stack([pad[int(pos[b]):int(pos[b]) + Tc, b] for b in range(B)], 1), n))
            pos = pos + n
        return out
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        for a in list(range(t0, t1, C)) or [t0]:
            b = min(a + C, t1)
            out.append((x[a:b], (il - a).clamp(0, b - a)))
    return out


class _Grown:
    """The device's growing lattice stream fed frame by frame, asked with final=False at every position it is asked for: per
    slot and position the token_frames / token_confidences rows (computed once per case and tolerance, shared by the chunkings)."""

    def __init__(self, x, tr, il, graph, K, tol, theta=INF, w=(LW, TS)):
        T, B, _ = x.shape
        s = _grow(tr, graph, B, T, K, theta, w)
        self.at = {}
        for t in range(T):
            s.advance(x[t:t + 1].to(DEV), (il - t).clamp(0, 1).to(DEV))
            r = s.result_confidence(tol, final=False)
            self.at[t + 1] = (r.token_frames.cpu().numpy(), r.token_confidences.cpu().numpy(), r.token_lengths.cpu().numpy())


def _run(s, plain, ref, calls, dtype, what, grown=None, P=1):
    """Feed the calls to the lattice-keeping stream, a plain stream and the restatement.  -> the concatenated (frames,
    confidences) per slot, for the chunk-invariance checks."""
    B = s.batch_size
    tfs, cfs = [[] for _ in range(B)], [[] for _ in range(B)]
    ntok = [0] * B                                               # tokens committed so far, per slot
    for i, (c, n) in enumerate(calls):
        w = "%s call %d" % (what, i)
        out = s.advance(c.to(DEV), n.to(DEV))
        assert type(out).__name__ == "BeamWindowConfCommit", w
        got = _host(out)
        if plain is not None:                                    # property 1
            assert [a.tobytes() for a in got[:5]] == _bytes(plain.advance(c.to(DEV), n.to(DEV))), w
        want = ref.advance(c.numpy(), n.numpy())
        for k, (g, v) in enumerate(zip(got[:5], (want[0], want[1], want[2], want[4], want[3]))):
            assert np.array_equal(g, v), (w, k)
        tf, cf, tl = got[5], got[6], got[3]
        assert tf.dtype == np.int64 and cf.dtype == NP[dtype] and tf.shape == cf.shape == got[0].shape, w
        assert np.array_equal(tf, want[5]), w                    # frames and padding exact
        behind = np.arange(tf.shape[1])[None, :] >= tl[:, None]
        assert (tf[behind] == -1).all() and (cf[behind] == 0).all(), w
        _close(cf, want[6], dtype, w)                            # property 4 and all prefix values
        for b in range(B):
            tfs[b] += tf[b, :tl[b]].tolist()
            cfs[b] += cf[b, :tl[b]].tobytes(),
    if grown is not None:                                        # property 3, from the restatement's own status
        for b in range(B):
            cat = np.frombuffer(b"".join(cfs[b]), NP[dtype])
            k = 0                                                # (k0, k1 count inside a call; the growing stream's from frame 0)
            for p1, b0, k0, k1, status in ref.ends[b]:
                n = k1 - k0
                if not status & 1:
                    gf, gc, gl = grown.at[p1]
                    assert gl[b] >= k + n, (what, b, p1)
                    assert tfs[b][k:k + n] == gf[b, k:k + n].tolist(), (what, b, p1)
                    assert cat[k:k + n].tobytes() == np.ascontiguousarray(gc[b, k:k + n]).tobytes(), (what, b, p1)
                k += n
            assert k == len(tfs[b]), (what, b)
    return tfs, cfs


def _plain_results_equal(s, plain, what):
    for final in (False, True):
        assert _bytes(s.result(final)) == _bytes(plain.result(final)), what
        assert _bytes(s.result_nbest(3, final, True)) == _bytes(plain.result_nbest(3, final, True)), what


# ---------------------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("W", [4, 8, 16])
@DTYPES
def test_grid_against_the_plain_stream_the_growing_stream_and_the_restatement(dtype, W):
    graph = _ngram(5, 3, 3, holes=True)
    Q = graph.compile_host(np.float32, LW, TS)["Q"]
    T, B = 40, 5
    x, tr, il = _case(T, B, graph.N, 11, dtype)
    turn = forced = exact = 0
    for K in (1, 3, 8, Q):
        for tol in (0, 1, 3):
            grown = _Grown(x, tr, il, graph, K, tol)
            for P in (1, 3, W):
                C = (1, 5, 16)[turn % 3]
                calls = _calls(x, il, _cuts(turn, T, P), C, turn)
                what = "W=%d P=%d K=%d tol=%d C=%d chunking %d" % (W, P, K, tol, C, turn % 6)
                turn += 1
                s, plain, ref = _window(tr, graph, B, W, P, K, tol, C), _window(tr, graph, B, W, P, K, keep=False), \
                    _ref(tr, graph, B, W, P, K, tol, C)
                _run(s, plain, ref, calls, dtype, what, grown, P)
                _plain_results_equal(s, plain, what)
                st = ref.result(True)[7]
                forced += int((st & 1).sum())
                exact += int(((st & 1) == 0).sum())
    assert forced > 0 and exact > 0 and turn >= 6


@DTYPES
def test_chunk_invariance_and_the_final_tail_against_the_one_shot_call(dtype):
    graph = _ngram(6, 2, 5)
    T, B, W, P, K, tol = 40, 5, 16, 3, 8, 1
    x, tr, il = _case(T, B, graph.N, 17, dtype)
    one = _asg().beam_decode_graph_confidence(x.to(DEV), tr.to(DEV), graph, il.to(DEV), K, INF, LW, TS, tol)
    of, oc, ol = one.token_frames.cpu().numpy(), one.token_confidences.cpu().numpy(), one.token_lengths.cpu().numpy()
    first, clear = None, 0
    for turn in range(6):
        C = 16
        s, ref = _window(tr, graph, B, W, P, K, tol, C), _ref(tr, graph, B, W, P, K, tol, C)
        tfs, cfs = _run(s, None, ref, _calls(x, il, _cuts(turn, T, P), C, turn), dtype, "chunking %d" % turn)
        cat = [(tfs[b], b"".join(cfs[b])) for b in range(B)]
        first = first or cat
        assert cat == first, turn                                # property 2: the same bits for every chunking
        r = s.result_confidence(final=True)
        assert type(r).__name__ == "BeamWindowConfidence"
        want = ref.result_confidence(final=True)
        h = {n: getattr(r, n).cpu().numpy() for n in r._fields}
        for n in ("path", "tokens", "states", "token_lengths", "token_frames", "frames", "committed", "status"):
            assert np.array_equal(h[n], want[n]), (turn, n)
        _close(h["token_confidences"], want["token_confidences"], dtype, turn)
        assert _bytes(s.result(True)) == [h[n].tobytes() for n in ("scores", "path", "tokens", "token_lengths", "states", "frames",
                                                                    "committed", "status")]
        for b in range(B):                                       # commits + tail = the one-shot call, while bit 0 is clear
            if h["status"][b] & 1:
                continue
            clear += 1
            n, m = len(tfs[b]), int(h["token_lengths"][b])
            assert n + m == ol[b] and tfs[b] + h["token_frames"][b, :m].tolist() == of[b, :n + m].tolist(), (turn, b)
            assert h["token_confidences"][b, :m].tobytes() == np.ascontiguousarray(oc[b, n:n + m]).tobytes(), (turn, b)
            assert h["normalisers"][b].tobytes() == one.normalisers[b].cpu().numpy().tobytes(), (turn, b)
    assert clear


# ---------------------------------------------------------------------------------------------------------------- special cases
@pytest.mark.parametrize("K", [63, 64, 65])
def test_kept_sets_at_the_wavefront_edge(K):
    S, N = 70, 4
    graph = _asg().TokenGraph(*chain_automaton(S, N)[:3], start=S - 1)
    T, B, W, P = 24, 2, 8, 2
    x, tr, _ = _case(T, B, N, 23, torch.float64)
    il = torch.tensor([T, T - 3])
    ref = _ref(tr, graph, B, W, P, K, 1, 5, w=(1.0, 0.0))
    s = _window(tr, graph, B, W, P, K, 1, 5, w=(1.0, 0.0))
    plain = _window(tr, graph, B, W, P, K, keep=False, w=(1.0, 0.0))
    grown = _Grown(x, tr, il, graph, K, 1, w=(1.0, 0.0))
    _run(s, plain, ref, _calls(x, il, [0, 5, 7, 12, 24], 5), torch.float64, "K=%d" % K, grown, P)
    assert max(max(z) for z in ref.g.sizes()) == K                # the regime: a kept set of exactly K states


@DTYPES
def test_the_largest_tolerance_and_a_pull_that_stops_above_frame_zero(dtype):
    graph = _ngram(5, 2, 9)
    T, B, W, P, tol = 40, 3, 8, 2, 64
    x, tr, il = _case(T, B, graph.N, 29, dtype)
    s, plain, ref = _window(tr, graph, B, W, P, 4, tol, 7), _window(tr, graph, B, W, P, 4, keep=False), \
        _ref(tr, graph, B, W, P, 4, tol, 7)
    _run(s, plain, ref, _calls(x, il, [0, 7, 14, 21, 28, 35, 40], 7), dtype, "tol 64", _Grown(x, tr, il, graph, 4, tol), P)
    assert all(b0 - tol <= 0 for p1, b0, *_ in ref.ends[0])       # every pull reaches frame 0
    s, ref = _window(tr, graph, B, W, P, 4, 1, 7), _ref(tr, graph, B, W, P, 4, 1, 7)
    _run(s, None, ref, _calls(x, il, [0, 7, 14, 21, 28, 35, 40], 7), dtype, "tol 1", _Grown(x, tr, il, graph, 4, 1), P)
    assert any(b0 - 1 > 0 for p1, b0, *_ in ref.ends[0]) and any(b0 - 1 <= 0 for p1, b0, *_ in ref.ends[0])


@pytest.mark.parametrize("K", [2, 4])
def test_forced_commits_on_two_components(K):
    graph = _asg().TokenGraph(*two_components_automaton(), start=0)
    T, B, W, P = 30, 2, 8, 2
    x = torch.from_numpy(two_component_emissions(T, B, graph.N, np.float64))
    tr = torch.zeros(graph.N, graph.N, dtype=torch.float64)
    il = torch.tensor([T, T - 3])
    s, plain, ref = _window(tr, graph, B, W, P, K, 1, 11, w=(1.0, -0.5)), _window(tr, graph, B, W, P, K, keep=False, w=(1.0, -0.5)), \
        _ref(tr, graph, B, W, P, K, 1, 11, w=(1.0, -0.5))
    _run(s, plain, ref, _calls(x, il, [0, 5, 6, 17, 28, 30], 11), torch.float64, "two components")
    assert all(v.status == 1 for v in ref.slots) and any(st & 1 for e in ref.ends for *_, st in e)
    want = ref.result_confidence(False)
    r = s.result_confidence(False)
    assert np.array_equal(r.token_frames.cpu().numpy(), want["token_frames"])
    _close(r.token_confidences.cpu().numpy(), want["token_confidences"], torch.float64, "tail")


def test_a_convergence_and_a_forced_commit_in_one_attempt_and_a_beam_that_empties():
    graph = _ngram(5, 3, 3, holes=True)
    T, B, dtype = 40, 5, torch.float64
    x, tr, il = _case(T, B, graph.N, 11, dtype)
    both = emptied = 0
    for W, P, K in ((4, 3, 3), (4, 4, 8), (8, 8, 3)):
        ref = _ref(tr, graph, B, W, P, K, 1, 16)
        s, plain = _window(tr, graph, B, W, P, K, 1, 16), _window(tr, graph, B, W, P, K, keep=False)
        xx = x.clone()
        xx[25:, 0] = -INF                                          # slot 0's beam empties inside a chunk, after its commits
        _run(s, plain, ref, _calls(xx, il, [0, 16, 32, 40], 16), dtype, "W=%d P=%d K=%d" % (W, P, K))
        both += sum(1 for v in ref.slots for pos, b0, c, F in v.attempts if c is not None and c >= b0 and F > 0)
        emptied += int(ref.slots[0].aq.size == 0 and ref.slots[0].base > 0)
        r = s.result_confidence(False)
        assert not torch.isnan(r.token_confidences).any() and _bytes(s.result(False)) == _bytes(plain.result(False))
    assert both and emptied


def test_no_frames_a_masked_reset_and_two_runs():
    graph = _ngram(5, 2, 9)
    T, B, W, P, K, dtype = 24, 3, 8, 2, 4, torch.float32
    x, tr, il = _case(T, B, graph.N, 31, dtype)
    il[:] = T
    runs = []
    for _ in range(2):
        s, plain, ref = _window(tr, graph, B, W, P, K, 2, 8), _window(tr, graph, B, W, P, K, keep=False), \
            _ref(tr, graph, B, W, P, K, 2, 8)
        calls = _calls(x, il, [0, 8, 8, 16], 8)                    # (a call with Tc = 0 in the middle)
        out = _run(s, plain, ref, calls, dtype, "first half")
        mask = torch.tensor([0, 1, 0])
        for t in (s, plain):
            t.reset(mask.to(DEV))
        ref.reset(mask.numpy())
        _plain_results_equal(s, plain, "masked reset")
        out2 = _run(s, plain, ref, _calls(x[16:], il - 16, [0, 8], 8), dtype, "second half")   # slot 1 starts anew at frame 0
        runs.append((out, out2, _bytes(s.result_confidence(False))))
        s.reset()
        plain.reset()
        _plain_results_equal(s, plain, "reset")
    assert runs[0] == runs[1]                                      # two runs bit-equal


def test_captured_advance_and_confidence_replay_on_fresh_chunks():
    graph = _ngram(5, 2, 9)
    T, B, W, P, K, dtype, Tc = 32, 3, 8, 2, 4, torch.float32, 8
    x, tr, il = _case(T, B, graph.N, 37, dtype)
    eager = _window(tr, graph, B, W, P, K, 1, Tc)
    want = []
    for a in range(0, T, Tc):
        o = eager.advance(x[a:a + Tc].to(DEV), (il - a).clamp(0, Tc).to(DEV))
        want.append(_bytes(o) + _bytes(eager.result_confidence(False)))
    s = _window(tr, graph, B, W, P, K, 1, Tc)
    chunk, lens = x[:Tc].to(DEV).clone(), il.clamp(0, Tc).to(DEV).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        s.reset()
        with torch.cuda.graph(g, stream=side):
            o = s.advance(chunk, lens)
            r = s.result_confidence(False)
    torch.cuda.current_stream().wait_stream(side)
    s.reset()
    for i, a in enumerate(range(0, T, Tc)):                        # the first replay and three on fresh chunks
        chunk.copy_(x[a:a + Tc])
        lens.copy_((il - a).clamp(0, Tc))
        g.replay()
        torch.cuda.synchronize()
        assert _bytes(o) + _bytes(r) == want[i], i


def test_the_other_streams_are_unchanged_afterwards():
    graph = _ngram(5, 2, 9)
    T, B, dtype = 16, 2, torch.float64
    x, tr, il = _case(T, B, graph.N, 41, dtype)
    il[:] = T

    def others():
        a = _asg()
        st = a.BeamStream(tr.to(DEV), graph, B, T, 4, INF, LW, TS, dtype=dtype)
        st.advance(x.to(DEV))
        gl = _grow(tr, graph, B, T, 4)
        gl.advance(x.to(DEV))
        pw = _window(tr, graph, B, 8, 2, 4, keep=False)
        o = pw.advance(x.to(DEV))
        return (_bytes(a.beam_decode_graph(x.to(DEV), tr.to(DEV), graph, il.to(DEV), 4, INF, LW, TS)) + _bytes(st.result(True)) +
                _bytes(o) + _bytes(pw.result(True)) + _bytes(gl.result_confidence(1, True)))
    before = others()
    s = _window(tr, graph, B, 8, 2, 4, 1, 16)
    s.advance(x.to(DEV))
    s.result_confidence(True)
    assert others() == before
