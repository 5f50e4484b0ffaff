"""GPU tests (-m gpu) of the per-final-node scores of target graphs and their gradients (csrc/asg_target_graph_final.hip)
against the float64 numpy restatement (tests/target_graph_final_ref.py): mixed batches with ignored NaN gradients, every
workgroup width, the LDS bound, the existing score / chains, the risk, capture, strides."""
import numpy as np
import pytest
import torch
import torch_asg_amd as A

from target_graph_final_ref import risk_ref, target_graph_final_ref
from test_hip_target_graph import _batch, _case, _skips, _tree
from util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NI = -np.inf
DTYPES = [torch.float64, torch.float32]


def _close(got, want, dtype, what):
    if dtype == torch.float64:
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9), what
    else:
        assert_close(got, want, what=what)


def _run(x, tr, graphs, il, g, fn=A.target_graph_final_scores):
    xd, td = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
    fs = fn(xd, td, graphs, None if il is None else il.to(DEV))
    fs.backward(g.to(DEV, fs.dtype))
    torch.cuda.synchronize()
    return fs.detach().cpu(), xd.grad.cpu(), td.grad.cpu()


def _check(x, tr, graphs, il, g, what):
    """g: float64 [B,Kmax]; NaN goes into every entry whose reference score is -inf.  -> the reference scores."""
    ref = target_graph_final_ref(x.double().numpy(), tr.double().numpy(), graphs.graphs, None if il is None else il.numpy(), g.numpy())
    g = torch.where(torch.from_numpy(ref[0] > NI), g, torch.full_like(g, float("nan")))
    got = [u.numpy() for u in _run(x, tr, graphs, il, g)]
    assert np.array_equal(got[0] == NI, ref[0] == NI) and not any(np.isnan(u).any() for u in got), what
    for name, u, v in zip((" scores", " grad_inputs", " grad_transition"), got, ref):
        _close(u, v, x.dtype, what + name)
    return ref[0], got[1]


def _mixed():
    """Graph shapes and lengths (0, 1, < T, T): empty, one node, chain, weighted tree, two branches of one label that meet again
    (two finals), a cycle with two finals, an unreachable final."""
    N, T = 6, 8
    meet = ([0, 1, 1, 2], [0.3, NI, NI, NI], [NI, 0.4, NI, -0.2], [(0, 1, 0.1), (0, 2, -0.4), (1, 3, 0.0), (2, 3, 0.7)])
    cycle = ([0, 1], [0.0, NI], [0.1, -0.3], [(0, 1, 0.5), (1, 0, -0.25)])
    specs = [([], [], [], []), ([3], [0.5], [-1.0], []), _tree([[1, 2, 0]], N), _tree([[0, 1, 2], [0, 3], [4, 1]], N, [0.0, -0.5, 0.25]),
             meet, cycle, ([0, 1], [0.0, NI], [NI, 0.0], []), _tree([[1, 2, 0]], N), cycle, meet, _tree([[5, 2, 4], [5, 1]], N)]
    return _batch(specs, N), T, N, torch.tensor([T, 1, T, 5, T, T, T, 0, 1, 6, 2])


def _grad(shape, seed):
    g = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return torch.where(torch.rand(shape, generator=torch.Generator().manual_seed(seed + 1)) < 0.2, torch.zeros_like(g), g)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_batch_against_reference(dtype):
    graphs, T, N, il = _mixed()
    x, tr, _ = _case(T, graphs.B, N, 1, dtype)
    g = _grad((graphs.B, graphs.Kmax), 4)
    fs, gx = _check(x, tr, graphs, il, g, "mixed %s" % dtype)
    assert [int((r > NI).sum()) for r in fs] == [0, 1, 1, 3, 2, 2, 0, 0, 1, 2, 1]
    if dtype == torch.float64:                    # every frame's weights sum to 1: row t holds the sum of g over the finite finals
        want = torch.where(torch.from_numpy(fs > NI), g, torch.zeros_like(g)).sum(1)
        live = torch.arange(T)[:, None] < il[None, :]
        assert np.allclose(gx.sum(2), (want[None, :] * live).numpy(), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,T,plain", [(64, 3, False), (65, 3, False), (256, 3, False), (257, 3, False), (1024, 3, False),
                                       (65, 67, True)])        # the last: a plain chain whose far end is reached (T > K)
def test_every_workgroup_width(K, T, plain, dtype):
    graphs = _batch([_skips(K, 12, K, plain), _skips(5, 12, 1)], 12)
    x, tr, _ = _case(T, 2, 12, K, dtype)
    g = torch.zeros(2, K, dtype=torch.float64)
    at = sorted({k % K for k in (0, 63, 64, K - 2, K - 1, 3)})       # finals on both sides of a wavefront and of the width
    g[0, at] = torch.linspace(-1.5, 2.0, len(at), dtype=torch.float64)
    g[1, :5] = torch.tensor([0.5, -1.0, 0.0, 2.0, -0.25], dtype=torch.float64)
    fs, _ = _check(x, tr, graphs, torch.tensor([T, 2]), g, "K=%d T=%d %s" % (K, T, dtype))
    assert (fs[0] > NI).sum() >= (1 if plain else K // 3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_count_at_the_lds_bound(dtype):
    N, K = 8, 8
    bound = int(A._lib.lib().asg_target_graph_max_edges(int(dtype == torch.float64), K))
    rng = np.random.default_rng(5)
    src = rng.integers(0, K, bound)
    dst = (src + rng.integers(1, K, bound)) % K                              # parallel edges, never a self edge
    ed = [(int(s), int(d), float(w)) for s, d, w in zip(src, dst, rng.normal(size=bound) - 7.0)]
    lab, w = list(range(K)), list(rng.normal(size=K))
    x, tr, _ = _case(2, 2, N, 6, dtype)
    g = torch.zeros(2, K, dtype=torch.float64)
    g[0, [1, 6]], g[1, 0] = torch.tensor([1.0, -2.0], dtype=torch.float64), 0.5
    _check(x, tr, _batch([(lab, w, w, ed), (lab[:2], w[:2], w[:2], [])], N), None, g, "at the bound %s" % dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_against_the_graph_score_and_the_chains_of_the_alternatives(dtype):
    T, N = 9, 6
    alts = [[[0, 1, 2, 4], [0, 1, 3], [2, 4, 2, 1, 0], [3]], [[5, 2], [5]], [[1, 0, 1, 0, 1, 0, 1]]]      # the last: longer than its utterance
    il = torch.tensor([T, 4, 6])
    graphs = A.TargetGraphs.from_alternatives(alts, N, [[0.0, -1.0, 0.5, -0.25], [0.3, 0.0], [0.0]])
    x, tr, _ = _case(T, 3, N, 11, dtype)
    ones = torch.ones(3, dtype=torch.float64)
    Z, zx, zt = _run(x, tr, graphs, il, ones, A.target_graph_score)
    fs = _run(x, tr, graphs, il, torch.zeros(3, graphs.Kmax))[0]
    _close(torch.logsumexp(fs[:2], 1).numpy(), Z[:2].numpy(), dtype, "logsumexp of the finals")
    assert Z[2] == NI and (fs[2] == NI).all()
    alt = _run(x, tr, graphs, il, torch.zeros(3, 4), A.target_graph_alternative_scores)[0]
    assert alt.shape == (3, 4) and (alt[1, 2:] == NI).all() and (alt[2] == NI).all()
    for b, a, w in ((0, 0, 0.0), (0, 1, -1.0), (0, 2, 0.5), (0, 3, -0.25), (1, 0, 0.3), (1, 1, 0.0)):
        chain = A.TargetGraphs.from_alternatives([[alts[b][a]]], N)
        one = A.target_graph_score(x[:, b:b + 1].to(DEV), tr.to(DEV), chain, il[b:b + 1].to(DEV)).cpu()
        _close(alt[b, a:a + 1].numpy(), one.numpy() + w, dtype, "alternative %d of %d" % (a, b))
    post = torch.softmax(alt.double(), 1).nan_to_num(0.0)           # d logsumexp / d score: the gradient of the graph score
    _, ax, at = _run(x, tr, graphs, il, post, A.target_graph_alternative_scores)
    _close(ax.numpy(), zx.numpy(), dtype, "grad_inputs")
    _close(at.numpy(), zt.numpy(), dtype, "grad_transition")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_risk_against_numpy(dtype, reduction):
    T, N = 7, 5
    alts = [[[0, 1, 2], [0, 3], [4, 1]], [[2]], [[1, 0, 1, 0, 1, 0, 1, 0]], [[3, 1], [3, 1, 4, 2, 0, 1, 3, 4]]]
    graphs = A.TargetGraphs.from_alternatives(alts, N)
    x, tr, _ = _case(T, 4, N, 13, dtype)
    costs = torch.tensor([[0.0, 2.0, 3.0], [1.0, 9.0, 9.0], [2.0, 9.0, 9.0], [1.0, 4.0, 9.0]], dtype=torch.float64)
    xd = x.to(DEV).requires_grad_(True)
    m = A.ASGLoss(N, reduction=reduction).to(DEV).to(dtype)
    m.transition.data.copy_(tr)
    risk = m.target_graph_risk(xd, graphs, costs.to(DEV))
    (risk.sum() if reduction == "none" else risk).backward()
    alt = target_graph_final_ref(x.double().numpy(), tr.double().numpy(), graphs.graphs, None, np.zeros((4, graphs.Kmax)))[0]
    alt = np.where(graphs.alternative_final >= 0, np.take_along_axis(alt, np.maximum(graphs.alternative_final, 0), 1), NI)
    want, dalt = risk_ref(alt, costs.numpy())
    scale = 0.25 if reduction == "mean" else 1.0
    g = np.zeros((4, graphs.Kmax))
    np.put_along_axis(g, np.maximum(graphs.alternative_final, 0), np.where(graphs.alternative_final >= 0, dalt * scale, 0.0), 1)
    _, gx, gt = target_graph_final_ref(x.double().numpy(), tr.double().numpy(), graphs.graphs, None, g)
    assert want[2] == 0 and want[3] == 1.0                            # no alignment: 0; one live alternative: its cost
    _close(risk.detach().cpu().numpy(), want if reduction == "none" else want.sum() * scale, dtype, "risk")
    _close(xd.grad.cpu().numpy(), gx, dtype, "grad_inputs")
    _close(m.transition.grad.cpu().numpy(), gt, dtype, "grad_transition")


def test_bit_identical_run_to_run_captured_and_strided():
    graphs, T, N, il = _mixed()
    x, tr, _ = _case(T, graphs.B, N, 2, torch.float32)
    g = _grad((graphs.B, graphs.Kmax), 8)
    first = _run(x, tr, graphs, il, g)
    assert all(torch.equal(u, v) for u, v in zip(first, _run(x, tr, graphs, il, g)))
    xb = x.transpose(0, 1).contiguous().to(DEV).transpose(0, 1).requires_grad_(True)          # a batch-major view
    wide = torch.zeros(N, 2 * N)
    wide[:, ::2] = tr
    tb = wide.to(DEV)[:, ::2].requires_grad_(True)
    fb = A.target_graph_final_scores(xb, tb, graphs, il.to(DEV))
    fb.backward(g.to(DEV, torch.float32))
    assert all(torch.equal(u, v.cpu()) for u, v in zip(first, (fb.detach(), xb.grad, tb.grad)))
    xs, trd = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
    ils, gd = il.to(DEV), g.to(DEV, torch.float32)

    def step():
        xs.grad = trd.grad = None
        fs = A.TargetGraphFinalScores.apply(xs, trd, graphs, ils)
        fs.backward(gd)
        return fs
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                            # warm
    torch.cuda.current_stream().wait_stream(s)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        fc = step()
    for seed in (3, 2):                                   # two replays, each against the eager bits of its data
        x2, _, _ = _case(T, graphs.B, N, seed, torch.float32)
        with torch.no_grad():
            xs.copy_(x2.to(DEV))
        cg.replay()
        torch.cuda.synchronize()
        got = (fc.detach().cpu().clone(), xs.grad.cpu().clone(), trd.grad.cpu().clone())
        assert all(torch.equal(u, v) for u, v in zip(got, _run(x2, tr, graphs, il, g)))
