"""GPU tests (-m gpu) of the ASG score over per-utterance target graphs (csrc/asg_target_graph.hip) against the float64 numpy
restatement (tests/target_graph_ref.py): mixed batches, every workgroup width, the LDS bound, chains against `FAC`, capture."""
import numpy as np
import pytest
import torch
import torch_asg_amd as A

from target_graph_ref import target_graph_ref
from util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NI = -np.inf
DTYPES = [torch.float64, torch.float32]


def _batch(specs, N):
    return A.TargetGraphs(*[[s[n] for s in specs] for n in range(4)], N)


def _tree(seqs, N, w=None):
    lab, sw, fw, src, dst, ew = A.TargetGraphs.from_alternatives([seqs], N, None if w is None else [w]).graphs[0]
    return lab, sw, fw, list(zip(src, dst, ew))


def _mixed():
    """The graph shapes and lengths (0, 1, < T, T) of one batch; the diamond repeats a label and its pairs, twice."""
    N, T = 6, 8
    diamond = ([0, 1, 1, 2], [0.3, NI, NI, NI], [NI, NI, NI, -0.2], [(0, 1, 0.1), (0, 2, -0.4), (1, 3, 0.0), (2, 3, 0.7)])
    specs = [([], [], [], []), ([3], [0.5], [-1.0], []), _tree([[1, 2, 0]], N),
             _tree([[0, 1, 2], [0, 3], [4, 1]], N, [0.0, -0.5, 0.25]),
             diamond,
             ([0, 1], [0.0, NI], [0.1, -0.3], [(0, 1, 0.5), (1, 0, -0.25)]),
             ([0, 1], [0.0, NI], [NI, 0.0], []),
             _tree([[1, 2, 0]], N), _tree([[5, 2, 4]], N), diamond]
    il = torch.tensor([T, 1, T, 5, T, T, T, 0, 2, 6])
    return _batch(specs, N), T, N, il


def _skips(K, N, seed, plain=False):
    """A chain, labels k mod N; unless `plain`, random skips of 2 or 3 nodes and start / final weights on every node."""
    rng = np.random.default_rng(seed)
    lab = [k % N for k in range(K)]
    ed = [(k, k + 1, 0.0) for k in range(K - 1)]
    if plain:
        return lab, [0.0] + [NI] * (K - 1), [NI] * (K - 1) + [0.0], ed
    ed += [(k, k + int(j), float(w)) for k, j, w in zip(range(K - 3), rng.integers(2, 4, K), rng.normal(size=K)) if rng.random() < 0.5]
    fw = rng.normal(size=K)
    fw[rng.random(K) < 0.3] = NI
    return lab, list(rng.normal(size=K)), list(fw), ed


def _case(T, B, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g, dtype=torch.float64), -1).to(dtype)
    tr = (0.5 * torch.randn(N, N, generator=g, dtype=torch.float64)).to(dtype)
    return x, tr, torch.linspace(-1.0, 2.0, B, dtype=torch.float64)


def _run(x, tr, graphs, il, gs):
    xd, td = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
    Z = A.target_graph_score(xd, td, graphs, None if il is None else il.to(DEV))
    Z.backward(gs.to(DEV, Z.dtype))
    torch.cuda.synchronize()
    return Z.detach().cpu(), xd.grad.cpu(), td.grad.cpu()


def _check(x, tr, graphs, il, gs, what):
    Z, gx, gtr = _run(x, tr, graphs, il, gs)
    Zr, gxr, gtrr = target_graph_ref(x.double().numpy(), tr.double().numpy(), graphs.graphs, None if il is None else il.numpy(),
                                     gs.numpy())
    fin = np.isfinite(Zr)
    assert (Z.numpy()[~fin] == NI).all() and not torch.isnan(gx).any() and not torch.isnan(gtr).any(), what
    assert (gx[:, torch.from_numpy(~fin)] == 0).all(), what
    for name, got, want in ((" Z", Z.numpy()[fin], Zr[fin]), (" grad_inputs", gx.numpy(), gxr), (" grad_transition", gtr.numpy(), gtrr)):
        if x.dtype == torch.float64:
            assert np.allclose(got, want, rtol=1e-9, atol=1e-9), what + name
        else:
            assert_close(got, want, what=what + name)
    return Zr


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_batch_against_reference(dtype):
    graphs, T, N, il = _mixed()
    x, tr, gs = _case(T, graphs.B, N, 1, dtype)
    assert list(np.isfinite(_check(x, tr, graphs, il, gs, "mixed %s" % dtype))) == [False, True, True, True, True, True, False, False, False, True]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,T,plain", [(64, 3, False), (65, 3, False), (256, 3, False), (257, 3, False), (1024, 3, False),
                                       (65, 67, True)])        # the last: a plain chain whose far end is reached (T > K)
def test_every_workgroup_width(K, T, plain, dtype):
    graphs = _batch([_skips(K, 12, K, plain), _skips(5, 12, 1)], 12)
    assert graphs.Kmax == K
    x, tr, gs = _case(T, 2, 12, K, dtype)
    assert np.isfinite(_check(x, tr, graphs, torch.tensor([T, 2]), gs, "K=%d T=%d %s" % (K, T, dtype))).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_count_at_the_lds_bound_and_above(dtype):
    N, K, e = 8, 8, (8 if dtype == torch.float64 else 4)
    bound = int(A._lib.lib().asg_target_graph_max_edges(int(dtype == torch.float64), K))
    assert bound == (128 * 1024 - K * (5 * e + 4)) // (2 * e + 4)          # include/asg_hip.h: what the backward keeps in LDS
    rng = np.random.default_rng(5)
    src = rng.integers(0, K, bound + 1)
    dst = (src + rng.integers(1, K, bound + 1)) % K                          # parallel edges, never a self edge
    ed = [(int(s), int(d), float(w)) for s, d, w in zip(src, dst, rng.normal(size=bound + 1) - 7.0)]
    lab, w = list(range(K)), list(rng.normal(size=K))
    x, tr, gs = _case(3, 2, N, 6, dtype)
    _check(x, tr, _batch([(lab, w, w, ed[:bound]), (lab[:2], w[:2], w[:2], ed[:0])], N), None, gs, "at the bound %s" % dtype)
    with pytest.raises(RuntimeError, match="Kmax = 8 .* Emax = %d .* at most %d" % (bound + 1, bound)):
        _run(x, tr, _batch([(lab, w, w, ed), (lab[:2], w[:2], w[:2], ed[:0])], N), None, gs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_chains_equal_the_force_aligned_path_and_module_loss(dtype):
    T, B, N = 12, 4, 7
    x, tr, gs = _case(T, B, N, 9, dtype)
    tg = torch.tensor([[1, 2, 3, 1, 0], [4, 5, 4, 0, 0], [0, 6, 2, 0, 0], [3, 1, 3, 1, 3]])
    tl, il = torch.tensor([5, 3, 3, 5]), torch.tensor([12, 9, 2, 7])      # utterance 2: tl > len (no alignment)
    graphs = A.TargetGraphs.from_targets(tg, tl, N)
    xa, ta = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
    Za = A.FAC.apply(ta, xa, tg.to(DEV), il.to(DEV), tl.to(DEV))
    fin = torch.isfinite(Za)
    torch.where(fin, Za, torch.zeros_like(Za)).mul(gs.to(DEV, dtype)).sum().backward()
    xb = x.transpose(0, 1).contiguous().to(DEV).transpose(0, 1).requires_grad_(True)      # a batch-major view
    tb = tr.to(DEV).requires_grad_(True)
    Zb = A.target_graph_score(xb, tb, graphs, il.to(DEV))
    Zb.backward(gs.to(DEV, dtype))
    assert list(fin.cpu()) == [True, True, False, True] and Zb[2] == NI
    assert_close(Zb.detach().cpu()[fin.cpu()].numpy(), Za.detach().cpu()[fin.cpu()].numpy(), what="scores")
    assert_close(xb.grad.cpu().numpy(), xa.grad.cpu().numpy(), what="grad_inputs")
    assert_close(tb.grad.cpu().numpy(), ta.grad.cpu().numpy(), what="grad_transition")
    m = A.ASGLoss(N, reduction='none').to(DEV).to(dtype)
    m.transition.data.copy_(tr)
    xa.grad = xb.grad = None
    la = m(xa, tg.to(DEV), il.to(DEV), tl.to(DEV))
    la.sum().backward()
    ga, gta = xa.grad.cpu(), m.transition.grad.cpu()
    m.transition.grad = None
    lb = m.target_graph_loss(xb, graphs, il.to(DEV))
    lb.sum().backward()
    assert lb[2] == float("inf") and la[2] == float("inf") and not torch.isnan(xb.grad).any()
    assert_close(lb.detach().cpu()[fin.cpu()].numpy(), la.detach().cpu()[fin.cpu()].numpy(), what="loss")
    assert_close(xb.grad.cpu().numpy(), ga.numpy(), what="loss grad_inputs")
    assert_close(m.transition.grad.cpu().numpy(), gta.numpy(), what="loss grad_transition")
    assert m.target_graph_loss(xb.detach().to(torch.float16), graphs, il.to(DEV)).dtype == dtype      # widened
    m.scale_mode = 'target_size'
    with pytest.raises(ValueError, match="target_size"):
        m.target_graph_loss(xb, graphs, il.to(DEV))


def test_bit_identical_run_to_run_and_captured():
    graphs, T, N, il = _mixed()
    x, tr, gs = _case(T, graphs.B, N, 2, torch.float32)
    assert all(torch.equal(u, v) for u, v in zip(_run(x, tr, graphs, il, gs), _run(x, tr, graphs, il, gs)))
    xs, trd = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
    ils, gsd = il.to(DEV), gs.to(DEV, torch.float32)

    def step():
        xs.grad = trd.grad = None
        Z = A.TargetGraphScore.apply(xs, trd, graphs, ils)
        Z.backward(gsd)
        return Z
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                            # warm
    torch.cuda.current_stream().wait_stream(s)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        Zc = step()
    for seed in (3, 2):                                   # two replays, each against the eager bits of its data
        x2, _, _ = _case(T, graphs.B, N, seed, torch.float32)
        with torch.no_grad():
            xs.copy_(x2.to(DEV))
        cg.replay()
        torch.cuda.synchronize()
        got = (Zc.detach().cpu().clone(), xs.grad.cpu().clone(), trd.grad.cpu().clone())
        assert all(torch.equal(u, v) for u, v in zip(got, _run(x2, tr, graphs, il, gs)))
