"""GPU tests (-m gpu) of the token confidences and start frames of every row of the token-graph n-best list
(`torch_asg_amd.beam_decode_graph_nbest_confidence`; csrc/asg_beam_nbest_conf.hip) against the numpy restatement
tests/beam_nbest_conf_ref.py.  In every case the eight n-best fields are byte-equal to the device's `beam_decode_graph_nbest`,
`normalisers` is bit-equal to the device's `beam_graph_full_score` without targets, row 0's frames and confidences are bit-equal
to the device's `beam_decode_graph_confidence`, rows that read one cell carry one value, `token_frames` is exact and
`token_confidences` is held to tests/test_hip_beam_loss.py's rule as tests/test_hip_beam_conf.py applies it (float64
rtol = atol = 1e-9, float32 util.assert_close, padding exactly 0).  Every case first asserts from the restatement that its input
is in the regime it names."""
import numpy as np
import pytest
import torch

from beam_loss_cases import DEV, GRAPHS, INF, _asg, _ngram
from beam_nbest_conf_ref import NAMES, beam_nbest_conf_ref, window_confidences
from test_hip_beam_conf import _case, _flat_case
from util import assert_close

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
W = (0.8, 0.2)                                                             # lm_weight, token_score
WF = (0.1, -0.5)                                                           # ... of the long cases: a frame adds about nothing to Z
WL = (0.1, -0.8)                                                           # ... of the long cases with a wide beam, for the same


def _d(t):
    return None if t is None else t.to(DEV)


def _np(t):
    return None if t is None else t.numpy()


def _run(x, tr, graph, il, K, nbest, th=INF, tol=0, w=W, align=True, **kw):
    return _asg().beam_decode_graph_nbest_confidence(_d(x), _d(tr), graph, _d(il), K, nbest, th, *w, align, tol, **kw)


def _bits(ts):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy().tobytes() for t in ts]


def _want(x, tr, graph, il, K, nbest, th=INF, w=W):
    return beam_nbest_conf_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start, _np(il), K, nbest, th, *w, 0)


def _close(got, want, dtype, what):
    assert not np.isnan(got).any(), what
    if dtype == torch.float64:
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9), what
    else:
        assert_close(got, want, what=what)


def _p2(n):
    r = 2
    while r < n:
        r *= 2
    return r


def _fits(K, dtype, nbest, tol):
    """The limit of include/asg_hip.h::asg_beam_graph_nbest_confidence (K: the beam the library uses, min(beam_size, Q))."""
    e = 8 if dtype == torch.float64 else 4
    return 16 * ((K * (e + 4) + 15) // 16) + 1024 + 12 * _p2(min(nbest, K) * (2 * tol + 2)) <= 163840


def _check(x, tr, graph, il, K, nbest, th=INF, tols=(0,), w=W, want=None, what="", align=lambda tol: True):
    """One (beam, threshold, nbest) against the device's own three neighbours and, at every tolerance, against the restatement."""
    A = _asg()
    dtype = x.dtype
    want = want or _want(x, tr, graph, il, K, nbest, th, w)
    xd, trd, ild = _d(x), _d(tr), _d(il)
    nb = {al: A.beam_decode_graph_nbest(xd, trd, graph, ild, K, nbest, th, *w, al) for al in set(align(t) for t in tols)}
    Z = A.beam_graph_full_score(xd, trd, graph, ild, K, th, *w)
    T = x.shape[0]
    for tol in tols:
        msg = "%s K=%d th=%s nbest=%d tol=%d %s" % (what, K, th, nbest, tol, dtype)
        al = align(tol)
        one = A.beam_decode_graph_confidence(xd, trd, graph, ild, K, th, *w, tol)
        got = A.beam_decode_graph_nbest_confidence(xd, trd, graph, ild, K, nbest, th, *w, al, tol)
        for n, a, b in zip(NAMES, got[:8], nb[al]):                        # the eight n-best fields, byte for byte
            assert (a is None) == (b is None) == (not al and n in ("path", "states")), msg + " " + n
            assert a is None or (a.dtype == b.dtype and a.shape == b.shape and _bits([a]) == _bits([b])), msg + " " + n
        assert _bits([got.normalisers]) == _bits([Z]) == _bits([one.normalisers]), msg
        assert _bits([got.token_frames[:, 0]]) == _bits([one.token_frames]), msg            # row 0 is the one-best call
        assert _bits([got.token_confidences[:, 0]]) == _bits([one.token_confidences]), msg
        for n in NAMES[3:] if al else NAMES[3:6]:
            assert np.array_equal(getattr(got, n).cpu().numpy(), want[n]), msg + " " + n
        frames, conf = got.token_frames.cpu().numpy(), got.token_confidences.cpu().numpy()
        assert frames.shape == conf.shape == (x.shape[1], nbest, T) and got.token_confidences.dtype == dtype
        assert np.array_equal(frames, want["token_frames"]), msg
        ref = window_confidences(want, _np(il), tol)
        behind = np.arange(T)[None, None, :] >= want["token_lengths"][:, :, None]
        assert (conf[behind] == 0).all() and (frames[behind] == -1).all(), msg                # the padding is exact
        _close(conf, ref, dtype, msg)
        tokens = want["tokens"]
        for b in range(x.shape[1]):                                        # one value per cell across the rows
            live = ~behind[b]
            key = frames[b][live] * (graph.N + 1) + tokens[b][live]
            val = conf[b][live].view(np.uint64 if dtype == torch.float64 else np.uint32)
            order = np.argsort(key, kind="stable")
            same = key[order][1:] == key[order][:-1]
            assert (val[order][1:][same] == val[order][:-1][same]).all(), msg
            assert len(set(key.tolist())) == len(want["cells"][b]), msg
        fin = np.isfinite(want["normalisers"])
        assert np.array_equal(np.isfinite(got.normalisers.cpu().numpy()), fin), msg
        _close(got.normalisers.cpu().numpy()[fin], want["normalisers"][fin], dtype, msg + " Z")
    return want


# ---------------------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["unigram", "trigram_holes", "random", "lexicon"])
def test_grid_of_beams_thresholds_lists_and_tolerances(name, dtype):
    graph = GRAPHS[name]()
    Q = graph.compile_host(np.float32)["Q"]
    x, tr, il = _case(12, 4, graph.N, 21, dtype, [12, 0, 1, 5])
    pruned = doubtful = short = 0
    for K in (1, 3, 8, Q + 5):
        for th in (INF, 2.0):
            for nbest in (1, 2, 8, 64):
                tols = tuple(t for t in (0, 1, 3, 64) if _fits(min(K, Q), dtype, nbest, t))
                assert len(tols) >= 3
                want = _check(x, tr, graph, il, K, nbest, th, tols, what=name, align=lambda tol: tol in (0, 3))
                assert want["num_hyps"][1] == 0 and want["normalisers"][1] == -np.inf               # length 0
                if want["num_hyps"][2]:
                    assert (want["token_lengths"][2, :int(want["num_hyps"][2])] == 1).all()           # length 1
                pruned += any(s == K for s in want["sizes"][0]) and K < Q
                c = want["token_confidences"][0, 1:][want["token_frames"][0, 1:] >= 0]
                doubtful += bool(((c > 0.01) & (c < 0.99)).any())
                short += bool(0 < want["num_hyps"][0] < nbest)
    assert pruned >= 3 and doubtful >= 2 and short >= 2


# ---------------------------------------------------------------------------------------------------------------- the pull
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [32, 33, 63, 64, 65])
def test_source_sets_around_the_subgroup_steps(K, dtype):
    graph = _ngram(70, 1, 11)
    x, tr, il = _case(6, 2, 70, 12, dtype, [6, 4])
    want = _want(x, tr, graph, il, K, 5)
    assert all(s == K for b in range(2) for s in want["sizes"][b])         # every source set has exactly K states
    assert (want["num_hyps"] == 5).all()
    _check(x, tr, graph, il, K, 5, INF, (0, 2), want=want, what="subgroup")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_set_above_one_workgroup_pass_and_more_rows_than_lanes(dtype):
    graph = _ngram(40, 3, 13)
    assert graph.compile_host(np.float32)["Q"] == 1640
    x, tr, il = _case(4, 2, 40, 14, dtype, [4, 3])
    want = _want(x, tr, graph, il, 1200, 1300)
    assert want["sizes"][0][2] == 1200 and want["sizes"][1][1] > 1024      # source sets of more than 1024 states
    assert want["num_hyps"][0] > 1024                                      # strips of lanes in the n-best stage, of rows in the prep
    assert want["queries"][0] > 2048 and _fits(1200, dtype, 1300, 1)
    _check(x, tr, graph, il, 1200, 1300, INF, (0, 1), want=want, what="wide", align=lambda tol: tol == 0)


# ---------------------------------------------------------------------------------------------------------------- the prep
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_three_sorts_of_the_prep_and_the_chunks_of_the_ballot_walk(dtype):
    """T = 130 with lengths 20 / 63 / 64 / 65 / 129: the queries of an utterance fit one strip of the dedupe (<= 1024), the LDS
    network with two strips (1025 .. 2048), or go through the network over the workspace (> 2048); the lengths sit around the
    64-frame chunks of the ballot walk."""
    graph = _ngram(10, 3, 3)
    x, tr, il = _flat_case(130, 5, 10, 15, dtype, [20, 63, 64, 65, 129])
    want = _want(x, tr, graph, il, 40, 30, w=WL)
    assert np.abs(want["normalisers"]).max() < 32                          # the running sums did stay small
    q = want["queries"]
    assert 0 < q[0] <= 1024 and all(1024 < v <= 2048 for v in q[1:4]) and q[4] > 2048
    assert (want["num_hyps"] == 30).all() and all(len(c) < v for c, v in zip(want["cells"], q))        # duplicates are dropped
    _check(x, tr, graph, il, 40, 30, INF, (0, 3), WL, want=want, what="prep", align=lambda tol: tol == 3)


# ---------------------------------------------------------------------------------------------------------------- the ring
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_ring_of_four_slots_wraps_many_times(dtype):
    graph = _ngram(10, 1, 1)
    x, tr, il = _flat_case(130, 2, 10, 15, dtype, [130, 120])
    want = _want(x, tr, graph, il, 6, 2, w=WF)
    assert np.abs(want["normalisers"]).max() < 32
    assert (want["num_hyps"] == 2).all() and (want["token_lengths"] > 100).all() and _p2(2 * (2 * 0 + 2)) == 4
    _check(x, tr, graph, il, 6, 2, INF, (0,), WF, want=want, what="ring 4")


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_largest_ring_of_a_beam_of_64_with_a_full_window(dtype):
    graph = _ngram(10, 3, 3)
    assert graph.compile_host(np.float32)["Q"] >= 64
    x, tr, il = _flat_case(130, 2, 10, 16, dtype, [130, 90])
    assert _fits(64, dtype, 63, 64) and not _fits(64, dtype, 64, 64) and _p2(63 * 130) == 8192
    want = _want(x, tr, graph, il, 64, 63, w=WL)
    assert np.abs(want["normalisers"]).max() < 32 and (want["num_hyps"] == 63).all()
    s = want["token_frames"][0, 5, :int(want["token_lengths"][0, 5])]
    assert max(int(((s >= v - 64) & (s <= v + 64)).sum()) for v in s) >= 20                  # tokens of one row inside one window
    _check(x, tr, graph, il, 64, 63, INF, (64,), WL, want=want, what="ring 8192", align=lambda tol: False)


# ---------------------------------------------------------------------------------------------------------------- the filter
@pytest.mark.parametrize("dtype", DTYPES)
def test_labels_that_share_a_filter_bit(dtype):
    graph = _ngram(300, 1, 17)
    x, tr, il = _case(4, 2, 300, 18, dtype, [4, 3])
    x[:, :, [5, 261, 280]] += 6.0                                          # rows through labels whose alias (mod 256) exists
    x = torch.log_softmax(x.double(), -1).to(dtype)
    want = _want(x, tr, graph, il, 300, 8)
    labels = set(c for cells in want["cells"] for _, c in cells)
    aliased = [c for c in labels if any(a != c and a % 256 == c % 256 and a not in labels for a in range(300))]
    assert aliased and max(labels) > 255                                   # events of a label in no row pass the filter
    assert all(s == 300 for s in want["sizes"][0])                         # ... and every label has events at every frame
    _check(x, tr, graph, il, 300, 8, INF, (0, 1), want=want, what="filter")


# ---------------------------------------------------------------------------------------------------------------- small inputs
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_single_frame(dtype):
    graph = GRAPHS["bigram"]()
    x, tr, il = _case(1, 3, graph.N, 17, dtype)
    want = _want(x, tr, graph, il, 4, 6)
    assert (want["num_hyps"] == 4).all() and (want["token_lengths"][:, :4] == 1).all() and np.isfinite(want["normalisers"]).all()
    _check(x, tr, graph, il, 4, 6, INF, (0, 5), want=want, what="T=1")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_beam_that_empties_and_an_end_without_a_final_weight(dtype):
    A = _asg()
    ok = A.TokenGraph(np.zeros((1, 5), np.int64), np.zeros((1, 5)), np.zeros(1))
    x, tr, il = _case(8, 3, 5, 18, dtype, [8, 8, 3])
    x[4:, 0] = -INF                                                        # utterance 0: every candidate of frame 4 is -inf
    want = _want(x, tr, ok, il, 3, 4)
    assert want["sizes"][0][3] == 3 and want["sizes"][0][4] == 0 and want["normalisers"][0] == -np.inf and want["num_hyps"][0] == 0
    assert np.isfinite(want["normalisers"][1:]).all() and (want["num_hyps"][1:] == 3).all()
    _check(x, tr, ok, il, 3, 4, INF, (0, 2), want=want, what="empties")
    nxt = np.array([[1, 1, 1], [2, 2, 2], [2, 2, 2]])
    fin = np.array([0.0, 0.5, -np.inf])                                    # three tokens or more end in the state that rejects
    dead = A.TokenGraph(nxt, np.zeros((3, 3)), fin)
    x, tr, il = _case(6, 2, 3, 19, dtype, [6, 1])
    x[:, 0] = torch.tensor([0.0, -9.0, -9.0, 0.0, -9.0, -9.0, -9.0, 0.0, -9.0, -9.0, -9.0, 0.0, 0.0, -9.0, -9.0, -9.0, 0.0,
                            -9.0]).reshape(6, 3).to(dtype)                 # a b c a a b: the beam of 2 holds no accepting state
    want = _want(x, tr, dead, il, 2, 3)
    assert want["sizes"][0][5] > 0 and want["normalisers"][0] == -np.inf and want["num_hyps"][0] == 0
    assert np.isfinite(want["normalisers"][1]) and want["num_hyps"][1] == 2
    _check(x, tr, dead, il, 2, 3, INF, (0, 1), want=want, what="no end")


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_two_runs_give_identical_bits_and_groups_equal_one_call():
    graph = GRAPHS["bigram"]()
    x, tr, il = _case(12, 6, graph.N, 22, torch.float32, [12, 3, 0, 1, 11, 7])
    a = _run(x, tr, graph, il, 24, 7, 6.0, 2)
    assert torch.isfinite(a.normalisers[[0, 1, 3, 4, 5]]).all() and (a.num_hyps[[0, 1, 3, 4, 5]] == 7).all()
    assert ((a.token_confidences[:, 1:] > 0.01) & (a.token_confidences[:, 1:] < 0.99)).any()
    for _ in range(2):
        assert _bits(_run(x, tr, graph, il, 24, 7, 6.0, 2)) == _bits(a)
    from torch_asg_amd.asg import native
    be = native()
    seen = []
    buf = be._buf
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    try:
        _run(x, tr, graph, il, 24, 7, 6.0, 2)
        whole = max(seen)
        seen.clear()
        small = _run(x, tr, graph, il, 24, 7, 6.0, 2, max_work_bytes=whole // 2)
        assert len(seen) == 1 and seen[0] < whole          # several groups of utterances through one smaller workspace
    finally:
        del be._buf
    assert _bits(small) == _bits(a)
    assert _bits(_run(x, tr, graph, il, 24, 7, 6.0, 2, max_work_bytes=1)) == _bits(a)          # one utterance per group


def test_capture_and_three_replays_on_fresh_emissions_and_lengths():
    A = _asg()
    graph = GRAPHS["trigram_holes"]()
    T, B, N = 9, 4, graph.N
    _, tr, _ = _case(T, B, N, 23, torch.float32)
    x = torch.zeros(T, B, N, device=DEV)
    trd = tr.to(DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)

    def step():
        return A.beam_decode_graph_nbest_confidence(x, trd, graph, il, 6, 4, 3.0, *W, True, 1)
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
        want = beam_nbest_conf_ref(x.cpu().numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start,
                                   il.cpu().numpy(), 6, 4, 3.0, *W, 1)
        assert np.array_equal(out.token_frames.cpu().numpy(), want["token_frames"])
        _close(out.token_confidences.cpu().numpy(), want["token_confidences"], torch.float32, "replay %d" % seed)


def test_the_neighbours_are_unchanged_after_the_call():
    A = _asg()
    graph = GRAPHS["random"]()
    x, tr, il = _case(9, 4, graph.N, 24, torch.float32, [9, 0, 1, 6])
    g = torch.Generator().manual_seed(3)
    tg, tl = torch.randint(0, graph.N, (4, 3), generator=g), torch.tensor([3, 0, 1, 2])
    xd, trd, ild, tgd, tld = x.to(DEV), tr.to(DEV), il.to(DEV), tg.to(DEV), tl.to(DEV)

    def others():
        out = list(A.beam_decode_graph(xd, trd, graph, ild, 6, 4.0, *W))
        out += [o for o in A.beam_decode_graph_nbest(xd, trd, graph, ild, 6, 3, 4.0, *W) if o is not None]
        out += list(A.beam_decode_graph_confidence(xd, trd, graph, ild, 6, 4.0, *W, 2))
        xg, tg_ = xd.clone().requires_grad_(True), trd.clone().requires_grad_(True)
        loss = A.beam_graph_asg_loss(xg, tgd, tg_, graph, ild, tld, 6, 4.0, *W)
        loss[torch.isfinite(loss)].sum().backward()
        out += [loss.detach(), xg.grad, tg_.grad]
        return [o.cpu() for o in out]
    before = others()
    A.beam_decode_graph_nbest_confidence(xd, trd, graph, ild, 64, 9, 4.0, *W, True, 3)
    got = A.ASGLoss(graph.N).to(DEV).beam_decode_graph_nbest_confidence(xd, graph, ild, 6, 3, 4.0, *W, frame_tolerance=1)
    assert got.path is None and got.states is None and got.token_confidences.shape == (4, 3, 9)
    for u, v in zip(before, others()):
        assert torch.equal(u, v)
