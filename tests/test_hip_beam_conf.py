"""GPU tests (-m gpu) of the token confidences and start frames of the token-graph beam decoder
(`torch_asg_amd.beam_decode_graph_confidence`; csrc/asg_beam_conf.hip) against the numpy restatement tests/beam_conf_ref.py.  The
five decoder fields are byte-equal to the device's `beam_decode_graph`, `normalisers` is bit-equal to the device's
`beam_graph_full_score` without targets, `token_frames` is exact and `token_confidences` is held to tests/test_hip_beam_loss.py's
rule (float64 rtol = atol = 1e-9, float32 util.assert_close, padding exact).  Every case first asserts from the restatement that
its input is in the regime it names."""
import numpy as np
import pytest
import torch

from beam_conf_ref import beam_conf_ref, window_confidences
from beam_loss_cases import DEV, GRAPHS, INF, _asg, _lexicon, _ngram
from util import assert_close

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
W = (0.8, 0.2)                                                             # lm_weight, token_score
WF = (0.1, -0.5)                                                           # ... of the long cases: a frame adds about nothing to Z
FIVE = ("scores", "path", "tokens", "token_lengths", "states")


def _d(t):
    return None if t is None else t.to(DEV)


def _run(x, tr, graph, il, K, th=INF, tol=0, w=W, **kw):
    return _asg().beam_decode_graph_confidence(_d(x), _d(tr), graph, _d(il), K, th, *w, tol, **kw)


def _bits(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in ts]


def _want(x, tr, graph, il, K, th=INF, w=W):
    return beam_conf_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start,
                         None if il is None else il.numpy(), K, th, *w, 0)


def _close(got, want, dtype, what):
    assert not np.isnan(got).any(), what
    if dtype == torch.float64:
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9), what
    else:
        assert_close(got, want, what=what)


def _check(x, tr, graph, il, K, th=INF, tols=(0,), w=W, want=None, what=""):
    """One (beam, threshold) against the device's own neighbours and, at every tolerance, against the restatement."""
    A = _asg()
    dtype = x.dtype
    want = want or _want(x, tr, graph, il, K, th, w)
    xd, trd, ild = _d(x), _d(tr), _d(il)
    dec = A.beam_decode_graph(xd, trd, graph, ild, K, th, *w)
    Z = A.beam_graph_full_score(xd, trd, graph, ild, K, th, *w)
    for tol in tols:
        msg = "%s K=%d th=%s tol=%d %s" % (what, K, th, tol, dtype)
        got = A.beam_decode_graph_confidence(xd, trd, graph, ild, K, th, *w, tol)
        for n, a, b in zip(FIVE, got[:5], dec):
            assert a.dtype == b.dtype and _bits([a]) == _bits([b]), msg + " " + n
        assert _bits([got.normalisers]) == _bits([Z]), msg
        for n in FIVE[1:]:
            assert np.array_equal(getattr(got, n).cpu().numpy(), want[n]), msg + " " + n
        assert np.array_equal(got.token_frames.cpu().numpy(), want["token_frames"]), msg
        conf = got.token_confidences.cpu().numpy()
        ref = window_confidences(want, None if il is None else il.numpy(), tol)
        behind = np.arange(x.shape[0])[None, :] >= want["token_lengths"][:, None]
        assert (conf[behind] == 0).all(), msg                              # the padding is exact
        _close(conf, ref, dtype, msg)
        fin = np.isfinite(want["normalisers"])
        assert np.array_equal(np.isfinite(got.normalisers.cpu().numpy()), fin), msg
        _close(got.normalisers.cpu().numpy()[fin], want["normalisers"][fin], dtype, msg + " Z")
    return want


def _case(T, B, N, seed, dtype, lengths=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g, dtype=torch.float64), -1).to(dtype)
    tr = (0.5 * torch.randn(N, N, generator=g, dtype=torch.float64)).to(dtype)
    return x, tr, None if lengths is None else torch.tensor(lengths)


def _flat_case(T, B, N, seed, dtype, lengths):
    """Emissions whose best label of every frame is 0 and small transitions with an expensive stay: the running sums of a long
    utterance stay small, so that float32's rounding of alpha + beta - Z stays far below the parity rule over hundreds of frames,
    and the winning path changes its label at nearly every frame.  The callers fold the automaton with WF for the same reason:
    at W a unigram costs about 1.7 per token, |alpha| passes 400 behind 250 tokens, and half an ulp of float32 there is 1.5e-5
    per add -- measured 2.6e-4 on a confidence at T = 300, above the rule's 1e-4, while float64 agrees to 1e-9."""
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g, dtype=torch.float64), -1)
    x = x - x.max(-1, keepdim=True).values
    tr = 0.1 * torch.randn(N, N, generator=g, dtype=torch.float64) - 3.0 * torch.eye(N, dtype=torch.float64)
    return x.to(dtype), tr.to(dtype), torch.tensor(lengths)


# ---------------------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["unigram", "trigram_holes", "random", "lexicon"])
def test_grid_of_beams_thresholds_and_tolerances(name, dtype):
    graph = GRAPHS[name]()
    Q = graph.compile_host(np.float32)["Q"]
    x, tr, il = _case(12, 4, graph.N, 21, dtype, [12, 0, 1, 5])
    pruned = doubtful = 0
    for K in (1, 3, 8, Q + 5):
        for th in (INF, 2.0):
            want = _check(x, tr, graph, il, K, th, (0, 1, 3, 64), what=name)
            assert want["token_lengths"][1] == 0 and want["normalisers"][1] == -np.inf            # length 0
            if np.isfinite(want["scores"][2]):
                assert want["token_lengths"][2] == 1 and want["token_frames"][2, 0] == 0          # length 1
            pruned += any(s == K for s in want["sizes"][0]) and K < Q
            c = want["token_confidences"][0, :int(want["token_lengths"][0])]
            doubtful += bool(((c > 0.01) & (c < 0.99)).any())
    assert pruned >= 3 and doubtful >= 2


# ---------------------------------------------------------------------------------------------------------------- the shapes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [32, 33, 63, 64, 65])
def test_source_sets_around_the_subgroup_steps(K, dtype):
    graph = _ngram(70, 1, 11)
    x, tr, il = _case(6, 2, 70, 12, dtype, [6, 4])
    want = _want(x, tr, graph, il, K)
    assert all(s == K for b in range(2) for s in want["sizes"][b])         # every source set has exactly K states
    _check(x, tr, graph, il, K, INF, (0, 2), want=want, what="subgroup")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_set_above_one_workgroup_pass(dtype):
    graph = _ngram(40, 3, 13)
    assert graph.compile_host(np.float32)["Q"] == 1640
    x, tr, il = _case(4, 2, 40, 14, dtype, [4, 3])
    want = _want(x, tr, graph, il, 1200)
    assert want["sizes"][0][2] == 1200 and want["sizes"][1][1] > 1024      # source sets of more than 1024 states
    _check(x, tr, graph, il, 1200, INF, (0, 1), want=want, what="wide")


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_trie_root_whose_row_is_longer_than_the_set(dtype):
    graph = _lexicon(12, 300, 9, maxlen=3)
    h, hb = graph.compile_host(np.float64), graph.compile_beam_host(np.float64)
    assert int(np.diff(h["row"]).max()) > 64 and int(hb["max_out"]) >= 11  # in: one edge per word end; out: one per first letter
    x, tr, il = _case(12, 3, 12, 4, dtype, [12, 7, 1])
    for K in (8, 32):
        want = _want(x, tr, graph, il, K)
        assert max(want["sizes"][0]) == K < int(hb["max_out"]) * 3
        assert (want["tokens"][0, :int(want["token_lengths"][0])] == 0).any()                  # a separator: a word boundary
        _check(x, tr, graph, il, K, INF, (0, 2), want=want, what="trie")


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_utterances_around_a_wavefront_with_a_full_window(dtype):
    graph = _ngram(10, 1, 1)
    x, tr, il = _flat_case(130, 4, 10, 15, dtype, [63, 64, 65, 129])
    want = _want(x, tr, graph, il, 6, w=WF)
    s = want["token_frames"][3, :int(want["token_lengths"][3])]
    assert max(int(((s >= v - 64) & (s <= v + 64)).sum()) for v in s) >= 20                  # tokens inside one window
    assert all(int(want["token_lengths"][b]) > 32 for b in range(4))
    _check(x, tr, graph, il, 6, INF, (0, 64), WF, want=want, what="T=130")


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_ring_wraps_behind_token_256(dtype):
    graph = _ngram(10, 1, 1)
    x, tr, il = _flat_case(300, 2, 10, 16, dtype, [300, 280])
    want = _want(x, tr, graph, il, 4, w=WF)
    assert np.abs(want["normalisers"]).max() < 32                          # the running sums did stay small
    assert int(want["token_lengths"][0]) > 257 and int(want["token_lengths"][1]) > 257         # a token index above 256
    _check(x, tr, graph, il, 4, INF, (0, 64), WF, want=want, what="T=300")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_single_frame(dtype):
    graph = GRAPHS["bigram"]()
    x, tr, il = _case(1, 3, graph.N, 17, dtype)
    want = _want(x, tr, graph, il, 4)
    assert (want["token_lengths"] == 1).all() and np.isfinite(want["normalisers"]).all()
    _check(x, tr, graph, il, 4, INF, (0, 5), want=want, what="T=1")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_beam_that_empties_and_an_end_without_a_final_weight(dtype):
    A = _asg()
    ok = A.TokenGraph(np.zeros((1, 5), np.int64), np.zeros((1, 5)), np.zeros(1))
    x, tr, il = _case(8, 3, 5, 18, dtype, [8, 8, 3])
    x[4:, 0] = -INF                                                        # utterance 0: every candidate of frame 4 is -inf
    want = _want(x, tr, ok, il, 3)
    assert want["sizes"][0][3] == 3 and want["sizes"][0][4] == 0 and want["normalisers"][0] == -np.inf
    assert np.isfinite(want["normalisers"][1:]).all()
    _check(x, tr, ok, il, 3, INF, (0, 2), want=want, what="empties")
    nxt = np.array([[1, 1, 1], [2, 2, 2], [2, 2, 2]])
    fin = np.array([0.0, 0.5, -np.inf])                                    # three tokens or more end in the state that rejects
    dead = A.TokenGraph(nxt, np.zeros((3, 3)), fin)
    x, tr, il = _case(6, 2, 3, 19, dtype, [6, 1])
    x[:, 0] = torch.tensor([0.0, -9.0, -9.0, 0.0, -9.0, -9.0, -9.0, 0.0, -9.0, -9.0, -9.0, 0.0, 0.0, -9.0, -9.0, -9.0, 0.0,
                            -9.0]).reshape(6, 3).to(dtype)                 # a b c a a b: the beam of 2 holds no accepting state
    want = _want(x, tr, dead, il, 2)
    assert want["sizes"][0][5] > 0 and want["normalisers"][0] == -np.inf and np.isfinite(want["normalisers"][1])
    _check(x, tr, dead, il, 2, INF, (0, 1), want=want, what="no end")


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_two_runs_give_identical_bits_and_groups_equal_one_call():
    graph = GRAPHS["bigram"]()
    x, tr, il = _case(12, 6, graph.N, 22, torch.float32, [12, 3, 0, 1, 11, 7])
    a = _run(x, tr, graph, il, 24, 6.0, 2)
    assert torch.isfinite(a.normalisers[[0, 1, 3, 4, 5]]).all()
    assert ((a.token_confidences > 0.01) & (a.token_confidences < 0.99)).any()
    for _ in range(2):
        assert _bits(_run(x, tr, graph, il, 24, 6.0, 2)) == _bits(a)
    from torch_asg_amd.asg import native
    be = native()
    seen = []
    buf = be._buf
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    try:
        _run(x, tr, graph, il, 24, 6.0, 2)
        whole = max(seen)
        seen.clear()
        small = _run(x, tr, graph, il, 24, 6.0, 2, max_work_bytes=whole // 2)
        assert len(seen) == 1 and seen[0] < whole          # several groups of utterances through one smaller workspace
    finally:
        del be._buf
    assert _bits(small) == _bits(a)
    assert _bits(_run(x, tr, graph, il, 24, 6.0, 2, max_work_bytes=1)) == _bits(a)             # one utterance per group


def test_capture_and_three_replays_on_fresh_emissions_and_lengths():
    A = _asg()
    graph = GRAPHS["trigram_holes"]()
    T, B, N = 9, 4, graph.N
    _, tr, _ = _case(T, B, N, 23, torch.float32)
    x = torch.zeros(T, B, N, device=DEV)
    trd = tr.to(DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)

    def step():
        return A.beam_decode_graph_confidence(x, trd, graph, il, 6, 3.0, *W, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                             # warm-up: compiles and caches the graph
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = step()
    for seed in (1, 2, 3):
        gen = torch.Generator().manual_seed(seed)
        x.copy_(torch.randn(T, B, N, generator=gen))
        il.copy_(torch.tensor([T, 4 + seed % 2, 1, T - seed]))
        gr.replay()
        torch.cuda.synchronize()
        assert _bits(out) == _bits(step())
        want = beam_conf_ref(x.cpu().numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start, il.cpu().numpy(),
                             6, 3.0, *W, 1)
        assert np.array_equal(out.token_frames.cpu().numpy(), want["token_frames"])
        _close(out.token_confidences.cpu().numpy(), want["token_confidences"], torch.float32, "replay %d" % seed)


def test_the_neighbours_are_unchanged_after_a_confidence_call():
    A = _asg()
    graph = GRAPHS["random"]()
    x, tr, il = _case(9, 4, graph.N, 24, torch.float32, [9, 0, 1, 6])
    g = torch.Generator().manual_seed(3)
    tg, tl = torch.randint(0, graph.N, (4, 3), generator=g), torch.tensor([3, 0, 1, 2])
    xd, trd, ild, tgd, tld = x.to(DEV), tr.to(DEV), il.to(DEV), tg.to(DEV), tl.to(DEV)

    def others():
        out = list(A.beam_decode_graph(xd, trd, graph, ild, 6, 4.0, *W))
        out += [o for o in A.beam_decode_graph_nbest(xd, trd, graph, ild, 6, 3, 4.0, *W) if o is not None]
        xg, tg_ = xd.clone().requires_grad_(True), trd.clone().requires_grad_(True)
        loss = A.beam_graph_asg_loss(xg, tgd, tg_, graph, ild, tld, 6, 4.0, *W)
        loss[torch.isfinite(loss)].sum().backward()
        out += [loss.detach(), xg.grad, tg_.grad]
        return [o.cpu() for o in out]
    before = others()
    A.beam_decode_graph_confidence(xd, trd, graph, ild, 64, 4.0, *W, 3)
    A.ASGLoss(graph.N).to(DEV).beam_decode_graph_confidence(xd, graph, ild, 6, 4.0, *W, frame_tolerance=1)
    for u, v in zip(before, others()):
        assert torch.equal(u, v)
    for bad in (dict(frame_tolerance=65), dict(frame_tolerance=-1)):
        with pytest.raises(RuntimeError, match="asg_beam_graph_confidence"):
            A.beam_decode_graph_confidence(xd, trd, graph, ild, 6, 4.0, **bad)
