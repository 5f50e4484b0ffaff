"""GPU tests (-m gpu) of beam-pruned decoding with a token automaton (`torch_asg_amd.beam_decode_graph`,
csrc/asg_beam_graph.hip): every output bit-identical to the test-side numpy restatement (tests/beam_decode_ref.py), a full beam
against the GPU's own exact decoder, path scores, a lexicon automaton, input handling, grouping, capture, determinism, errors."""
import numpy as np
import pytest
import torch

from beam_decode_ref import beam_decode_ref
from graph_decode_ref import path_score_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
NAMES = ("scores", "path", "tokens", "token_lengths", "states")


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _ngram(N, order, seed, holes=False):
    rng = np.random.default_rng(seed)
    lp = np.log(rng.dirichlet(np.ones(N + 1), size=(N + 1,) * (order - 1))) if order > 1 else np.log(rng.dirichlet(np.ones(N + 1)))
    if holes:
        lp[rng.random(size=lp.shape) < 0.2] = -np.inf
    return _asg().TokenGraph.from_ngram(lp)


def _random_graph(S, N, seed):
    """A random deterministic automaton whose upper states are unreachable, with missing arcs and non-accepting states."""
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, S // 2, size=(S, N))             # states >= S/2 are never entered
    nxt[rng.random(size=(S, N)) < 0.3] = -1
    w = rng.normal(size=(S, N))
    f = rng.normal(size=S)
    f[rng.random(size=S) < 0.3] = -np.inf
    return _asg().TokenGraph(nxt, w, f, start=0)


def _case(T, B, N, seed, dtype=torch.float32, integer=False):
    g = torch.Generator().manual_seed(seed)
    if integer:
        x = torch.randint(-2, 3, (T, B, N), generator=g).to(dtype)
        tr = torch.randint(-1, 2, (N, N), generator=g).to(dtype)
    else:
        x = torch.log_softmax(torch.randn(T, B, N, generator=g, dtype=torch.float64), -1).to(dtype)
        tr = torch.randn(N, N, generator=g, dtype=torch.float64).to(dtype)
    il = torch.randint(0, T + 1, (B,), generator=g)
    il[0] = T
    if B > 1:
        il[1] = 0
    if B > 2:
        il[2] = 1
    return x, tr, il


def _gpu(x, tr, graph, il, K, theta=INF, lw=1.0, ts=0.0, **kw):
    out = _asg().beam_decode_graph(x.to(DEV), tr.to(DEV), graph, None if il is None else il.to(DEV), K, theta, lw, ts, **kw)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _check(x, tr, graph, il, K, theta=INF, lw=1.0, ts=0.0, what="", **kw):
    got = _gpu(x, tr, graph, il, K, theta, lw, ts, **kw)
    want = beam_decode_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start,
                           None if il is None else il.numpy(), K, theta, lw, ts)
    assert got[0].dtype == x.dtype and all(o.dtype == torch.int64 for o in got[1:])
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(g.numpy(), w), "%s %s K=%d theta=%s" % (name, what, K, theta)
    return got


GRAPHS = {
    "unigram40": lambda: _ngram(40, 1, 1),
    "bigram40": lambda: _ngram(40, 2, 2),
    "trigram40": lambda: _ngram(40, 3, 3, holes=True),
    "random": lambda: _random_graph(30, 12, 4),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_bit_identical_to_the_restatement(name, dtype):
    graph = GRAPHS[name]()
    Q = graph.compile_host(np.float32, 0.8, -0.5)["Q"]
    x, tr, il = _case(60, 5, graph.N, 11, dtype)
    for K in (1, 3, 8, max(1, Q // 4)):
        for theta in (INF, 4.0, 0.0):
            _check(x, tr, graph, il, K, theta, 0.8, -0.5, name)
    _check(x, tr, graph, None, 8, INF, 1.0, 0.0, name + " no lengths")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_integer_scores_tie_at_the_last_rank(dtype):
    for graph in (_asg().TokenGraph.from_ngram(np.zeros((7, 7))), _ngram(6, 3, 7, holes=True),
                  _asg().TokenGraph(np.zeros((1, 6), np.int64), np.zeros((1, 6)), np.zeros(1))):
        x, tr, il = _case(40, 5, 6, 15, dtype, integer=True)
        Q = graph.compile_host(np.float32)["Q"]
        for K in (1, 3, 8, max(1, Q // 4)):
            for theta in (INF, 4.0, 0.0):
                _check(x, tr, graph, il, K, theta, 1.0, 1.0, "ties")
    z = torch.zeros(9, 2, 6, dtype=dtype)
    _check(z, torch.zeros(6, 6, dtype=dtype), _asg().TokenGraph.from_ngram(np.zeros((7, 7))), None, 4, INF, what="all zero")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_a_full_beam_equals_the_exact_decoder(name, dtype):
    A = _asg()
    graph = GRAPHS[name]()
    Q = graph.compile_host(np.float32, 0.8, -0.5)["Q"]
    x, tr, il = _case(60, 5, graph.N, 12, dtype)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    want = A.viterbi_decode_graph(xd, trd, graph, ild, 0.8, -0.5)
    for K in (Q, Q + 100):
        got = A.beam_decode_graph(xd, trd, graph, ild, K, INF, 0.8, -0.5)
        for n, u, v in zip(NAMES, got, want):
            assert u.dtype == v.dtype and torch.equal(u, v), "%s K=%d" % (n, K)


def test_fourgram_scores_are_path_scores_and_never_above_exact():
    A = _asg()
    N = 14
    graph = _ngram(N, 4, 5)
    x, tr, il = _case(80, 8, N, 13, torch.float32)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    exact = [o.cpu() for o in A.viterbi_decode_graph(xd, trd, graph, ild, 1.3, 0.25)]
    sc, path, tok, tl, st = [o.cpu() for o in A.beam_decode_graph(xd, trd, graph, ild, 32, INF, 1.3, 0.25)]
    for b in range(8):
        L = int(il[b])
        assert sc[b].item() <= exact[0][b].item()
        if L == 0:
            assert sc[b].item() == -INF and (path[b] == -1).all() and tl[b] == 0
            continue
        assert sc[b].item() > -INF                              # a dense n-gram: the beam cannot die out
        s, sts = path_score_graph(x[:, b].numpy(), tr.numpy(), graph.next, graph.weight, graph.final, path[b, :L].numpy(),
                                  graph.start, 1.3, 0.25)
        assert s == sc[b].item() and sts == st[b, :L].tolist()
        if torch.equal(path[b], exact[1][b]):
            assert sc[b].item() == exact[0][b].item()
    _check(x, tr, graph, il, 32, INF, 1.3, 0.25, "4-gram")


def test_lexicon_automaton():
    rng = np.random.default_rng(41)
    N, sep = 28, 27
    words = []
    while len(words) < 3000:
        w = rng.integers(0, sep, size=int(rng.integers(2, 9))).tolist()
        if all(a != b for a, b in zip(w, w[1:])):
            words.append(w)
    graph = _asg().TokenGraph.from_lexicon(words, N, sep, rng.normal(size=len(words)))
    assert graph.S > 5000
    x, tr, il = _case(60, 6, N, 42, torch.float32)
    got = _check(x, tr, graph, il, 64, INF, 1.0, 0.0, "lexicon")
    _check(x, tr, graph, il, 64, 6.0, 0.7, -0.2, "lexicon, threshold")
    assert (got[0][il > 0] > -INF).any()


def test_large_beams():
    graph = _ngram(40, 3, 3, holes=True)
    x, tr, il = _case(30, 3, 40, 18)
    for K in (1024, 4096):                                     # 4096 is above Q here: the whole graph
        _check(x, tr, graph, il, K, INF, 0.8, -0.5, "large beam")
    g4 = _ngram(40, 4, 5)
    x, tr, il = _case(12, 3, 40, 19)
    _check(x, tr, g4, il, 4096, INF, what="4-gram, K = 4096")
    _check(x, tr, g4, il, 1024, 5.0, what="4-gram, K = 1024")


def test_edge_cases():
    graph = _ngram(6, 2, 7)
    T = 9
    for B in (1, 4):
        x, tr, _ = _case(T, B, 6, 14 + B)
        il = torch.tensor([T, 0, 1, T][:B])
        _check(x, tr, graph, il, 4, what="lengths B=%d" % B)
    x, tr, il = _case(T, 3, 6, 16)
    dead = [_asg().TokenGraph(graph.next, graph.weight, np.full(graph.S, -np.inf)),          # no accepting state
            _asg().TokenGraph(np.where(np.arange(graph.S)[:, None] == 0, -1, graph.next), graph.weight, graph.final),
            _asg().TokenGraph(np.full((2, 6), -1), np.zeros((2, 6)), np.zeros(2))]          # no arc at all (Q = 0)
    for g in dead:
        sc, path, tok, tl, st = _check(x, tr, g, il, 4)
        assert (sc == -np.inf).all() and (path == -1).all() and (tok == -1).all() and (tl == 0).all() and (st == -1).all()
    # a beam that dies out: -inf emissions on everything the narrow beam kept
    x, tr, il = _case(T, 2, 6, 17)
    x[4] = -INF
    sc = _check(x, tr, graph, torch.tensor([T, 3]), 3)[0]
    assert sc[0] == -INF and sc[1] > -INF


def test_input_handling():
    A = _asg()
    graph = _ngram(40, 3, 8)
    g = torch.Generator().manual_seed(17)
    T, B, N = 50, 6, 40
    x_btn = torch.randn(B, T, N, generator=g).to(DEV)
    tr = torch.randn(N, N, generator=g).to(DEV)
    il = torch.tensor([50, 3, 0, 1, 49, 20], device=DEV)
    x = x_btn.transpose(0, 1)                                           # strided [T,B,N] view
    out = A.beam_decode_graph(x, tr, graph, il, 16, 8.0, 0.6, 0.1)
    ref = A.beam_decode_graph(x.contiguous(), tr, graph, il, 16, 8.0, 0.6, 0.1)
    for u, v in zip(out, ref):
        assert torch.equal(u, v)
    want = beam_decode_ref(x.cpu().numpy(), tr.cpu().numpy(), graph.next, graph.weight, graph.final, 0, il.cpu().numpy(),
                           16, 8.0, 0.6, 0.1)
    for u, v in zip(out, want):
        assert np.array_equal(u.cpu().numpy(), v)
    # several utterance groups: the same as one call
    from torch_asg_amd.asg import native
    be = native()
    seen = []
    buf = be._buf
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    try:
        one = A.beam_decode_graph(x, tr, graph, il, 16, 8.0, 0.6, 0.1)
        per = seen[-1] // B
        small = A.beam_decode_graph(x, tr, graph, il, 16, 8.0, 0.6, 0.1, max_work_bytes=2 * per + per // 2)
        assert seen[-1] == 2 * per
    finally:
        del be._buf
    for u, v, w in zip(small, out, one):
        assert torch.equal(u, v) and torch.equal(w, v)
    # the module method
    loss = A.ASGLoss(N).to(DEV)
    with torch.no_grad():
        loss.transition.copy_(tr)
    for u, v in zip(loss.beam_decode_graph(x, graph, il, 16, 8.0, 0.6, 0.1), out):
        assert torch.equal(u, v)
    # half precision decodes as its widening to the transition's dtype
    for hd in (torch.float16, torch.bfloat16):
        xh = x.to(hd)
        for u, v in zip(A.beam_decode_graph(xh, tr, graph, il, 16), A.beam_decode_graph(xh.float(), tr, graph, il, 16)):
            assert torch.equal(u, v)
    # compile_beam is cached under its own key and leaves compile's entry alone
    c = graph.compile(DEV, torch.float32, 0.6, 0.1)
    cb = graph.compile_beam(DEV, torch.float32, 0.6, 0.1)
    assert graph.compile(DEV, torch.float32, 0.6, 0.1) is c and graph.compile_beam(DEV, torch.float32, 0.6, 0.1) is cb
    assert "orow" not in c and cb["label"] is c["label"]


def test_capture_and_replay():
    A = _asg()
    graph = _ngram(40, 3, 9)
    T, B, N = 40, 4, 40
    x = torch.zeros(T, B, N, device=DEV)
    tr = torch.randn(N, N, device=DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.beam_decode_graph(x, tr, graph, il, 24, 9.0, 0.9, 0.2)          # warm-up: compiles and caches the graph
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = A.beam_decode_graph(x, tr, graph, il, 24, 9.0, 0.9, 0.2)
    for seed in (1, 2, 3):
        gen = torch.Generator().manual_seed(seed)
        x.copy_(torch.log_softmax(torch.randn(T, B, N, generator=gen), -1))
        il.copy_(torch.tensor([T, seed, 0, T - seed]))
        gr.replay()
        torch.cuda.synchronize()
        eager = A.beam_decode_graph(x, tr, graph, il, 24, 9.0, 0.9, 0.2)
        for u, v in zip(out, eager):
            assert torch.equal(u, v)


def test_two_runs_give_identical_bits():
    A = _asg()
    graph = _ngram(40, 3, 3, holes=True)
    x, tr, il = _case(120, 16, 40, 20)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    a = A.beam_decode_graph(xd, trd, graph, ild, 100, 12.0, 0.8, -0.5)
    for _ in range(3):
        b = A.beam_decode_graph(xd, trd, graph, ild, 100, 12.0, 0.8, -0.5)
        for u, v in zip(a, b):
            assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()


def test_errors():
    A = _asg()
    graph = _ngram(5, 2, 10)
    x = torch.randn(4, 2, 5, device=DEV)
    tr = torch.randn(5, 5, device=DEV)
    with pytest.raises(RuntimeError):
        A.beam_decode_graph(x.cpu(), tr.cpu(), graph, beam_size=4)
    with pytest.raises(RuntimeError, match="tokens"):
        A.beam_decode_graph(torch.randn(4, 2, 6, device=DEV), torch.randn(6, 6, device=DEV), graph, beam_size=4)
    with pytest.raises(RuntimeError):
        A.beam_decode_graph(x, tr.double(), graph, beam_size=4)
    with pytest.raises(RuntimeError):
        A.beam_decode_graph(x.to(torch.int32), tr, graph, beam_size=4)
    with pytest.raises(RuntimeError):
        A.beam_decode_graph(x, tr, graph, torch.tensor([4, 4], dtype=torch.int32, device=DEV), beam_size=4)
    with pytest.raises(TypeError):
        A.beam_decode_graph(x, tr, None, beam_size=4)
    for kw in (dict(beam_size=0), dict(beam_size=4, beam_threshold=-1.0), dict(beam_size=4, beam_threshold=float("nan"))):
        with pytest.raises(ValueError):
            A.beam_decode_graph(x, tr, graph, **kw)
    big = _ngram(40, 4, 5)
    with pytest.raises(RuntimeError, match="unsupported|limit|support"):
        A.beam_decode_graph(torch.randn(4, 2, 40, device=DEV), torch.randn(40, 40, device=DEV), big, beam_size=10000)
