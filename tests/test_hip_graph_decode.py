"""GPU tests (-m gpu) of Viterbi decoding with a token automaton (`torch_asg_amd.viterbi_decode_graph`,
csrc/asg_decode_graph.hip): every output bit-identical to the test-side numpy restatement (tests/graph_decode_ref.py) on both
routes, the one-state automaton against `viterbi_decode`, path scores, edge cases, input handling, capture and errors."""
import numpy as np
import pytest
import torch

from graph_decode_ref import decode_graph_ref, path_score_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


def _gpu(x, tr, graph, il, lw=1.0, ts=0.0, flags=0, max_work_bytes=1 << 30):
    from torch_asg_amd.asg import native
    out = native().viterbi_decode_graph(x.to(DEV), tr.to(DEV), graph, None if il is None else il.to(DEV), lw, ts,
                                        max_work_bytes, flags)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _check(x, tr, graph, il, lw=1.0, ts=0.0, flags=0, what="", **kw):
    got = _gpu(x, tr, graph, il, lw, ts, flags, **kw)
    want = decode_graph_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start,
                            None if il is None else il.numpy(), lw, ts)
    assert got[0].dtype == x.dtype and all(o.dtype == torch.int64 for o in got[1:])
    for name, g, w in zip(("scores", "path", "tokens", "token_lengths", "states"), got, want):
        assert np.array_equal(g.numpy(), w), "%s %s" % (name, what)
    return got


STREAM, RESIDENT = 16, 32        # ASG_FLAG_DECODE_GRAPH_STREAMING, ASG_FLAG_DECODE_GRAPH_RESIDENT

GRAPHS = {
    "unigram40": lambda: _ngram(40, 1, 1),
    "bigram40": lambda: _ngram(40, 2, 2),
    "trigram40": lambda: _ngram(40, 3, 3, holes=True),
    "random": lambda: _random_graph(30, 12, 4),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_bit_identical_to_the_reference_on_both_routes(name, dtype):
    graph = GRAPHS[name]()
    x, tr, il = _case(60, 5, graph.N, 11, dtype)
    a = _check(x, tr, graph, il, 0.8, -0.5, 0, name + " default route")
    b = _check(x, tr, graph, il, 0.8, -0.5, STREAM, name + " streaming")
    c = _check(x, tr, graph, il, 0.8, -0.5, RESIDENT, name + " resident")
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)
    _check(x, tr, graph, None, 1.0, 0.0, 0, name + " no lengths")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_fourgram_takes_the_streaming_route(dtype):
    graph = _ngram(40, 4, 5)
    c = graph.compile(DEV, dtype, 1.0, 0.0)
    assert c["Q"] > 60000 and c["E"] > 2000000                # 2 * Q * e > 128 KiB: not resident
    x, tr, il = _case(12, 3, 40, 12, dtype)
    a = _check(x, tr, graph, il, 1.0, 0.0, 0, "4-gram")
    b = _gpu(x, tr, graph, il, 1.0, 0.0, STREAM)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N", [1, 2, 40, 64, 65, 128, 256])
def test_one_state_automaton_equals_viterbi_decode(N, dtype):
    graph = _asg().TokenGraph(np.zeros((1, N), np.int64), np.zeros((1, N)), np.zeros(1))
    x, tr, il = _case(80, 6, N, 100 + N, dtype)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    want = _asg().viterbi_decode(xd, trd, ild)
    for flags in (0, STREAM, RESIDENT):
        from torch_asg_amd.asg import native
        got = native().viterbi_decode_graph(xd, trd, graph, ild, 1.0, 0.0, 1 << 30, flags)
        for g, w in zip(got[:4], want):
            assert torch.equal(g, w), "N=%d flags=%d" % (N, flags)
        assert torch.equal(got[4], torch.where(got[1] >= 0, 0, -1))


def test_path_score_matches_the_returned_score():
    graph = _ngram(40, 3, 6)
    x, tr, il = _case(100, 4, 40, 13, torch.float32)
    sc, path, tok, tl, st = _check(x, tr, graph, il, 1.7, 0.25)
    for b in range(4):
        L = int(il[b])
        if L == 0:
            continue
        s, sts = path_score_graph(x[:, b].numpy(), tr.numpy(), graph.next, graph.weight, graph.final, path[b, :L].numpy(),
                                  graph.start, 1.7, 0.25)
        assert s == sc[b].item() and sts == st[b, :L].tolist()


def test_edge_cases():
    graph = _ngram(6, 2, 7)
    T = 9
    for B in (1, 4):
        x, tr, _ = _case(T, B, 6, 14 + B)
        il = torch.tensor([T, 0, 1, T][:B])
        _check(x, tr, graph, il, what="lengths B=%d" % B)
        _check(x, tr, graph, il, flags=STREAM, what="lengths B=%d streaming" % B)
        _check(_case(T, B, 40, 14)[0], _case(T, B, 40, 14)[1], _ngram(40, 3, 7), il, flags=RESIDENT, what="resident B=%d" % B)
    for dtype in (torch.float32, torch.float64):                   # integer emissions: ties everywhere
        x, tr, il = _case(40, 5, 6, 15, dtype, integer=True)
        for flags in (0, STREAM, RESIDENT):
            _check(x, tr, _asg().TokenGraph.from_ngram(np.zeros((7, 7))), il, 1.0, 1.0, flags, "ties")
            _check(x, tr, _asg().TokenGraph(np.zeros((1, 6), np.int64), np.zeros((1, 6)), np.zeros(1)), il, 0.0, 0.0, flags)
    x, tr, il = _case(T, 3, 6, 16)
    dead = [_asg().TokenGraph(graph.next, graph.weight, np.full(graph.S, -np.inf)),          # no accepting state
            _asg().TokenGraph(np.where(np.arange(graph.S)[:, None] == 0, -1, graph.next), graph.weight, graph.final),
            _asg().TokenGraph(np.full((2, 6), -1), np.zeros((2, 6)), np.zeros(2))]          # no arc at all (Q = 0)
    for g in dead:
        for flags in (0, STREAM):
            sc, path, tok, tl, st = _check(x, tr, g, il, flags=flags)
            assert (sc == -np.inf).all() and (path == -1).all() and (tok == -1).all() and (tl == 0).all() and (st == -1).all()


def test_input_handling():
    A = _asg()
    graph = _ngram(40, 3, 8)
    g = torch.Generator().manual_seed(17)
    T, B, N = 50, 6, 40
    x_btn = torch.randn(B, T, N, generator=g).to(DEV)
    tr = torch.randn(N, N, generator=g).to(DEV)
    il = torch.tensor([50, 3, 0, 1, 49, 20], device=DEV)
    x = x_btn.transpose(0, 1)                                           # strided [T,B,N] view
    out = A.viterbi_decode_graph(x, tr, graph, il, 0.6, 0.1)
    ref = A.viterbi_decode_graph(x.contiguous(), tr, graph, il, 0.6, 0.1)
    for u, v in zip(out, ref):
        assert torch.equal(u, v)
    want = decode_graph_ref(x.cpu().numpy(), tr.cpu().numpy(), graph.next, graph.weight, graph.final, 0, il.cpu().numpy(),
                            0.6, 0.1)
    for u, v in zip(out, want):
        assert np.array_equal(u.cpu().numpy(), v)
    # several utterance groups: the same as one call
    per = T * graph.compile(DEV, torch.float32, 0.6, 0.1)["Q"] * 4
    small = A.viterbi_decode_graph(x, tr, graph, il, 0.6, 0.1, max_work_bytes=2 * per + 300 * 1024)
    for u, v in zip(small, out):
        assert torch.equal(u, v)
    # the module method
    loss = A.ASGLoss(N).to(DEV)
    with torch.no_grad():
        loss.transition.copy_(tr)
    for u, v in zip(loss.viterbi_decode_graph(x, graph, il, 0.6, 0.1), out):
        assert torch.equal(u, v)
    # half precision decodes as its widening to the transition's dtype
    for hd in (torch.float16, torch.bfloat16):
        xh = x.to(hd)
        for u, v in zip(A.viterbi_decode_graph(xh, tr, graph, il), A.viterbi_decode_graph(xh.float(), tr, graph, il)):
            assert torch.equal(u, v)


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
        A.viterbi_decode_graph(x, tr, graph, il, 0.9, 0.2)             # warm-up: compiles and caches the graph
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = A.viterbi_decode_graph(x, tr, graph, il, 0.9, 0.2)
    for seed in (1, 2):
        gen = torch.Generator().manual_seed(seed)
        x.copy_(torch.log_softmax(torch.randn(T, B, N, generator=gen), -1))
        il.copy_(torch.tensor([T, seed, 0, T - seed]))
        gr.replay()
        torch.cuda.synchronize()
        eager = A.viterbi_decode_graph(x, tr, graph, il, 0.9, 0.2)
        for u, v in zip(out, eager):
            assert torch.equal(u, v)


def test_errors():
    A = _asg()
    graph = _ngram(5, 2, 10)
    x = torch.randn(4, 2, 5, device=DEV)
    tr = torch.randn(5, 5, device=DEV)
    with pytest.raises(RuntimeError):
        A.viterbi_decode_graph(x.cpu(), tr.cpu(), graph)
    with pytest.raises(RuntimeError):
        A.viterbi_decode_graph(torch.randn(4, 2, 6, device=DEV), torch.randn(6, 6, device=DEV), graph)
    with pytest.raises(RuntimeError):
        A.viterbi_decode_graph(x, tr.double(), graph)
    with pytest.raises(RuntimeError):
        A.viterbi_decode_graph(x.to(torch.int32), tr, graph)
    with pytest.raises(RuntimeError):
        A.viterbi_decode_graph(x, tr, graph, torch.tensor([4, 4], dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        A.viterbi_decode_graph(x, tr, None)
