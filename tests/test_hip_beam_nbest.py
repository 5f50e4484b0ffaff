"""GPU tests (-m gpu) of the n-best beam decoder with its score split (`torch_asg_amd.beam_decode_graph_nbest`,
csrc/asg_beam_nbest.hip): every output bit-identical to the test-side numpy restatement (tests/beam_nbest_ref.py) in float32 and
float64 -- a grid of automata, beams, list lengths and thresholds, fewer candidates than asked for and none, ties, the sizes
around the sort's padding, more hypotheses than lanes and than a strip, the frame blocks of the token collapse -- then row 0
against the GPU's own beam decoder, grouping, capture, determinism, errors, and the older routes after an n-best call."""
import numpy as np
import pytest
import torch

from beam_decode_ref import beam_decode_ref
from beam_loss_cases import _compare, _full, _ref
from beam_nbest_ref import beam_nbest_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
NAMES = ("scores", "emission_scores", "graph_scores", "tokens", "token_lengths", "num_hyps", "path", "states")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])


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
    """The random automaton of the beam decoder's tests: unreachable upper states, missing arcs, non-accepting states."""
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, S // 2, size=(S, N))
    nxt[rng.random(size=(S, N)) < 0.3] = -1
    w = rng.normal(size=(S, N))
    f = rng.normal(size=S)
    f[rng.random(size=S) < 0.3] = -np.inf
    return _asg().TokenGraph(nxt, w, f, start=0)


def _case(T, B, N, seed, dtype=torch.float32, integer=False, lengths=None):
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
    return x, tr, (il if lengths is None else torch.tensor(lengths))


def _gpu(x, tr, graph, il, K, nbest, theta=INF, lw=1.0, ts=0.0, **kw):
    out = _asg().beam_decode_graph_nbest(x.to(DEV), tr.to(DEV), graph, None if il is None else il.to(DEV), K, nbest, theta, lw,
                                         ts, **kw)
    torch.cuda.synchronize()
    return type(out)(*[None if o is None else o.cpu() for o in out])


def _want(x, tr, graph, il, K, nbest, theta=INF, lw=1.0, ts=0.0, sizes=None):
    return beam_nbest_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start,
                          None if il is None else il.numpy(), K, nbest, theta, lw, ts, sizes=sizes)


def _same(got, want, dtype, what, alignments=True):
    assert got._fields == NAMES
    for name, g, w in zip(NAMES, got, want):
        if name in ("path", "states") and not alignments:
            assert g is None, what
            continue
        assert g.dtype == (dtype if name.endswith("scores") else torch.int64), (name, what)
        assert g.shape == w.shape, (name, what)
        # bit for bit (array_equal would let -0 pass for +0 and fail on nothing else here: there is no NaN)
        assert g.numpy().tobytes() == np.ascontiguousarray(w).tobytes(), "%s %s" % (name, what)


def _check(x, tr, graph, il, K, nbest, theta=INF, lw=1.0, ts=0.0, what="", both=False, sizes=None, **kw):
    want = _want(x, tr, graph, il, K, nbest, theta, lw, ts, sizes)
    what = "%s K=%d nbest=%d theta=%s" % (what, K, nbest, theta)
    got = _gpu(x, tr, graph, il, K, nbest, theta, lw, ts, return_alignments=True, **kw)
    _same(got, want, x.dtype, what)
    if both:
        _same(_gpu(x, tr, graph, il, K, nbest, theta, lw, ts, **kw), want, x.dtype, what + " no alignments", alignments=False)
    return got, want


GRAPHS = {
    "unigram6": lambda: _ngram(6, 1, 1),
    "bigram6": lambda: _ngram(6, 2, 2),
    "trigram6": lambda: _ngram(6, 3, 3, holes=True),
    "random": lambda: _random_graph(30, 12, 4),
}


@DTYPES
@pytest.mark.parametrize("name", list(GRAPHS))
def test_bit_identical_to_the_restatement(name, dtype):
    graph = GRAPHS[name]()
    Q = graph.compile_host(np.float32, 0.8, -0.5)["Q"]
    T, B = 12, 5
    x, tr, il = _case(T, B, graph.N, 11, dtype)
    assert il[0] == T and il[1] == 0 and il[2] == 1
    most, padded = 0, False
    for K in (1, 3, 8, Q):
        for nbest in sorted({1, 2, K, K + 5}):
            for theta in (INF, 4.0, 0.0):
                _, want = _check(x, tr, graph, il, K, nbest, theta, 0.8, -0.5, name, both=True)
                nh = want[5]
                assert nh[1] == 0 and (nh <= min(nbest, K)).all()
                most = max(most, int(nh.max()))
                padded |= bool((nh < nbest).any())
    assert most > 2 or Q <= 2, "the grid never ranked more than two hypotheses"
    assert padded
    _check(x, tr, graph, None, 8, 4, INF, 1.0, 0.0, name + " no lengths")


@DTYPES
def test_fewer_candidates_than_nbest_and_none(dtype):
    """A lexicon trie: most states are inside a word and not final, so a narrow beam often ends with few accepting states or
    with none at all."""
    rng = np.random.default_rng(41)
    N, sep = 9, 0
    words = []
    while len(words) < 80:
        w = rng.integers(1, N, size=int(rng.integers(3, 8))).tolist()
        if all(a != b for a, b in zip(w, w[1:])):
            words.append(w)
    graph = _asg().TokenGraph.from_lexicon(words, N, sep, rng.normal(size=len(words)))
    final = np.isfinite(graph.final)
    assert final.sum() * 2 < graph.S                            # most states are not final
    T, B = 10, 8
    x, tr, il = _case(T, B, N, 42, dtype)
    none = few = full = 0
    for K, nbest in ((2, 4), (4, 4), (6, 3), (12, 20)):
        sizes = []
        _, want = _check(x, tr, graph, il, K, nbest, INF, 1.0, 0.0, "lexicon", both=True, sizes=sizes)
        nh = want[5]
        for b in range(B):
            last = sizes[b][-1] if sizes[b] else 0
            none += last > 0 and nh[b] == 0                     # survivors, none of them accepting
            few += 0 < nh[b] < min(nbest, last)                 # fewer candidates than survivors and than rows
            full += nh[b] == nbest
    assert none > 0 and few > 0 and full > 0, (none, few, full)


@DTYPES
def test_ties_come_out_in_ascending_product_state(dtype):
    tied = 0
    for graph in (_asg().TokenGraph.from_ngram(np.zeros((7, 7))), _ngram(6, 3, 7, holes=True),
                  _asg().TokenGraph(np.zeros((1, 6), np.int64), np.zeros((1, 6)), np.zeros(1))):
        x, tr, il = _case(12, 5, 6, 15, dtype, integer=True)
        Q = graph.compile_host(np.float32)["Q"]
        for K in (3, 8, Q):
            for theta in (INF, 4.0, 0.0):
                _, want = _check(x, tr, graph, il, K, K, theta, 1.0, 1.0, "ties")
                sc, nh = want[0], want[5]
                for b in range(5):
                    tied += int((sc[b, 1:nh[b]] == sc[b, :max(nh[b] - 1, 0)]).sum())
    assert tied > 10
    z = torch.zeros(9, 2, 6, dtype=dtype)                       # every end equal: the rows are the product states in order
    graph = _asg().TokenGraph.from_ngram(np.zeros((7, 7)))
    got, want = _check(z, torch.zeros(6, 6, dtype=dtype), graph, None, 6, 6, what="all zero")
    assert (want[5] == 6).all() and (got.path[:, :, -1] == torch.arange(6)).all()


@DTYPES
@pytest.mark.parametrize("n", [63, 64, 65])
def test_sort_padding(n, dtype):
    """A dense bigram over n tokens has n product states, all accepting: the last set holds n candidates, one below, at and
    one above the power of two the sort pads to."""
    graph = _ngram(n, 2, 20 + n)
    x, tr, il = _case(4, 2, n, 21, dtype, lengths=[4, 3])
    sizes = []
    _, want = _check(x, tr, graph, il, n, n, what="sort padding", both=True, sizes=sizes)
    assert (want[5] == n).all() and all(s[-1] == n for s in sizes)


def test_walker_strips():
    """More hypotheses than a wavefront has lanes and than the workgroup has threads: the walk runs in strips."""
    graph = _ngram(11, 4, 5)
    assert graph.compile_host(np.float32)["Q"] == 1463
    x, tr, il = _case(6, 2, 11, 23, torch.float32, lengths=[6, 5])
    _, want = _check(x, tr, graph, il, 1300, 1300, what="strips")
    assert (want[5] > 1024).all()


@DTYPES
def test_frame_blocks(dtype):
    graph = _ngram(6, 2, 2)
    T = 130
    x, tr, il = _case(T, 5, 6, 24, dtype, lengths=[1, 63, 64, 65, 129])
    _, want = _check(x, tr, graph, il, 4, 4, what="frame blocks", both=True)
    assert (want[5] == 4).all()
    last = want[6][4]                                             # tokens that begin behind the first block of 64 frames
    assert (last[:, 65:129] != last[:, 64:128]).any()


@DTYPES
def test_row_0_is_the_beam_decoder(dtype):
    A = _asg()
    for name in ("trigram6", "random"):
        graph = GRAPHS[name]()
        x, tr, il = _case(12, 5, graph.N, 12, dtype)
        xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
        for K, theta in ((1, INF), (5, INF), (8, 3.0), (1000, INF)):
            one = A.beam_decode_graph(xd, trd, graph, ild, K, theta, 0.8, -0.5)
            for nbest in (1, 7):
                nb = A.beam_decode_graph_nbest(xd, trd, graph, ild, K, nbest, theta, 0.8, -0.5, return_alignments=True)
                rows = (nb.scores, nb.path, nb.tokens, nb.token_lengths, nb.states)
                for n, u, v in zip(("scores", "path", "tokens", "token_lengths", "states"), rows, one):
                    assert u.dtype == v.dtype and u.shape[:2] == (5, nbest), n
                    assert u[:, 0].cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), (n, name, K, nbest)
                assert torch.equal(nb.num_hyps > 0, one[0] > -INF)


def test_input_handling_and_grouping():
    A = _asg()
    graph = _ngram(6, 3, 8)
    g = torch.Generator().manual_seed(17)
    T, B, N = 12, 6, 6
    x_btn = torch.randn(B, T, N, generator=g).to(DEV)
    tr = torch.randn(N, N, generator=g).to(DEV)
    il = torch.tensor([12, 3, 0, 1, 11, 7], device=DEV)
    x = x_btn.transpose(0, 1)                                           # strided [T,B,N] view
    args = (graph, il, 16, 5, 8.0, 0.6, 0.1, True)
    out = A.beam_decode_graph_nbest(x, tr, *args)
    for u, v in zip(out, A.beam_decode_graph_nbest(x.contiguous(), tr, *args)):
        assert torch.equal(u, v)
    want = beam_nbest_ref(x.cpu().numpy(), tr.cpu().numpy(), graph.next, graph.weight, graph.final, 0, il.cpu().numpy(),
                          16, 5, 8.0, 0.6, 0.1)
    for u, v in zip(out, want):
        assert np.array_equal(u.cpu().numpy(), v)
    # several utterance groups: the bits of one call
    from torch_asg_amd.asg import native
    be = native()
    seen = []
    buf = be._buf
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    try:
        one = A.beam_decode_graph_nbest(x, tr, *args)
        whole = seen[-1]
        small = A.beam_decode_graph_nbest(x, tr, *args, max_work_bytes=whole // 2 - 1)
        assert 0 < seen[-1] <= whole // 2 - 1                           # at most two of the six utterances in a group
    finally:
        del be._buf
    for u, v, w in zip(small, out, one):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()
    # the module method, and half precision as its widening
    loss = A.ASGLoss(N).to(DEV)
    with torch.no_grad():
        loss.transition.copy_(tr)
    for u, v in zip(loss.beam_decode_graph_nbest(x, *args), out):
        assert torch.equal(u, v)
    xh = x.to(torch.bfloat16)
    for u, v in zip(A.beam_decode_graph_nbest(xh, tr, graph, il, 16, 5), A.beam_decode_graph_nbest(xh.float(), tr, graph, il, 16, 5)):
        assert (u is None and v is None) or torch.equal(u, v)


def test_capture_and_replay():
    A = _asg()
    graph = _ngram(6, 3, 9)
    T, B, N = 16, 4, 6
    x = torch.zeros(T, B, N, device=DEV)
    tr = torch.randn(N, N, device=DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)
    args = (graph, il, 24, 6, 9.0, 0.9, 0.2, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.beam_decode_graph_nbest(x, tr, *args)                          # warm-up: compiles and caches the graph
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = A.beam_decode_graph_nbest(x, tr, *args)
    for seed in (1, 2, 3):
        gen = torch.Generator().manual_seed(seed)
        x.copy_(torch.log_softmax(torch.randn(T, B, N, generator=gen), -1))
        il.copy_(torch.tensor([T, seed, 0, T - seed]))
        gr.replay()
        torch.cuda.synchronize()
        eager = A.beam_decode_graph_nbest(x, tr, *args)
        for u, v in zip(out, eager):
            assert torch.equal(u, v)
        assert out.num_hyps[2] == 0 and out.num_hyps[0] > 1


def test_two_runs_give_identical_bits():
    A = _asg()
    graph = _ngram(11, 3, 3, holes=True)
    x, tr, il = _case(20, 8, 11, 20)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    a = A.beam_decode_graph_nbest(xd, trd, graph, ild, 100, 100, 12.0, 0.8, -0.5, return_alignments=True)
    assert a.num_hyps.max() > 64
    for _ in range(2):
        b = A.beam_decode_graph_nbest(xd, trd, graph, ild, 100, 100, 12.0, 0.8, -0.5, return_alignments=True)
        for u, v in zip(a, b):
            assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()


def test_errors():
    A = _asg()
    graph = _ngram(5, 2, 10)
    x = torch.randn(4, 2, 5, device=DEV)
    tr = torch.randn(5, 5, device=DEV)
    f = A.beam_decode_graph_nbest
    with pytest.raises(RuntimeError):
        f(x.cpu(), tr.cpu(), graph, beam_size=4)
    with pytest.raises(RuntimeError, match="tokens"):
        f(torch.randn(4, 2, 6, device=DEV), torch.randn(6, 6, device=DEV), graph, beam_size=4)
    with pytest.raises(RuntimeError):
        f(x, tr.double(), graph, beam_size=4)
    with pytest.raises(RuntimeError):
        f(x.to(torch.int32), tr, graph, beam_size=4)
    with pytest.raises(RuntimeError):
        f(x, tr, graph, torch.tensor([4, 4], dtype=torch.int32, device=DEV), beam_size=4)
    with pytest.raises(TypeError):
        f(x, tr, None, beam_size=4)
    for kw in (dict(beam_size=0), dict(beam_size=4, beam_threshold=-1.0), dict(beam_size=4, beam_threshold=float("nan")),
               dict(beam_size=4, nbest=0), dict(beam_size=4, nbest=-2)):
        with pytest.raises(ValueError):
            f(x, tr, graph, **kw)
    with pytest.raises(RuntimeError, match="unsupported|limit|support"):
        f(x, tr, graph, beam_size=4, nbest=8193)
    with pytest.raises(RuntimeError, match="unsupported|limit|support"):
        f(x, tr, graph, beam_size=4, nbest=10 ** 12)
    big = _ngram(21, 4, 5)
    with pytest.raises(RuntimeError, match="unsupported|limit|support"):
        f(torch.randn(4, 2, 21, device=DEV), torch.randn(21, 21, device=DEV), big, beam_size=10000)
    assert f(x, tr, graph, beam_size=4, nbest=8192).scores.shape == (2, 8192)


@DTYPES
def test_the_older_routes_after_an_nbest_call(dtype):
    """The search kernel is shared: after an n-best call the decoder and the beam-pruned loss still equal their own
    restatements (the kernel's new workspace offset at 0 is the code they always ran)."""
    A = _asg()
    graph = GRAPHS["trigram6"]()
    x, tr, il = _case(12, 5, graph.N, 31, dtype)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    for K, theta in ((3, INF), (8, 4.0)):
        A.beam_decode_graph_nbest(xd, trd, graph, ild, K, 5, theta, 0.8, -0.5)
        got = [o.cpu() for o in A.beam_decode_graph(xd, trd, graph, ild, K, theta, 0.8, -0.5)]
        want = beam_decode_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start, il.numpy(), K, theta,
                               0.8, -0.5)
        for u, v in zip(got, want):
            assert np.array_equal(u.numpy(), v)
        tg = torch.tensor([[1, 2, 2, 4], [0, 1, 2, 3], [3, 0, 0, 0], [5, 4, 3, 2], [2, 2, 1, 0]])
        tl = torch.tensor([4, 2, 1, 3, 4])
        A.beam_decode_graph_nbest(xd, trd, graph, ild, K, 5, theta, 0.8, -0.5)
        _compare(_full(x, tr, graph, il, K, theta, 0.8, -0.5, None, tg, tl), _ref(x, tr, graph, il, K, theta, 0.8, -0.5, None, tg, tl),
                 dtype, "loss after nbest K=%d" % K)
        la = A.beam_graph_asg_loss(xd, tg.to(DEV), trd, graph, ild, tl.to(DEV), K, theta, 0.8, -0.5)
        assert not torch.isnan(la).any()
