"""GPU tests (-m gpu) of the ASG loss composed with a token automaton (`torch_asg_amd.graph_full_score`, `graph_asg_loss`,
`ASGLoss.graph_loss`; csrc/asg_graph_loss.hip): scores and gradients against the float64 numpy restatement
(tests/graph_loss_ref.py) on both routes, determinism, the one-state identity against ASGLoss, normalisation, gradcheck,
infeasible utterances, strided inputs, capture and errors."""
import itertools

import numpy as np
import pytest
import torch

from graph_loss_ref import full_graph_ref, target_scores_ref
from graph_regime_cases import _ngram, _one_state       # (shared with tests/test_hip_graph_regimes.py)
from util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STREAM, RESIDENT = 128, 256        # ASG_FLAG_GRAPH_LOSS_STREAMING, ASG_FLAG_GRAPH_LOSS_RESIDENT


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _random_graph(S, N, seed):
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, S // 2, size=(S, N))             # states >= S/2 are never entered
    nxt[rng.random(size=(S, N)) < 0.3] = -1
    w = rng.normal(size=(S, N))
    f = rng.normal(size=S)
    f[rng.random(size=S) < 0.3] = -np.inf
    return _asg().TokenGraph(nxt, w, f, start=0)


GRAPHS = {
    "unigram": lambda: _ngram(10, 1, 1),
    "bigram": lambda: _ngram(10, 2, 2),
    "trigram_holes": lambda: _ngram(6, 3, 3, holes=True),
    "random": lambda: _random_graph(12, 7, 4),
}


def _case(T, B, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g, dtype=torch.float64), -1).to(dtype)
    tr = (0.5 * torch.randn(N, N, generator=g, dtype=torch.float64)).to(dtype)
    il = torch.randint(0, T + 1, (B,), generator=g)
    il[0] = T
    if B > 1:
        il[1] = 0
    if B > 2:
        il[2] = 1
    return x, tr, il


def _full(x, tr, graph, il, lw=1.0, ts=0.0, flags=0, gs=None, max_work_bytes=1 << 30):
    xd = x.to(DEV).requires_grad_(True)
    td = tr.to(DEV).requires_grad_(True)
    Z = _asg().GraphFullScore.apply(xd, td, graph, None if il is None else il.to(DEV), lw, ts, max_work_bytes, flags)
    g = torch.ones_like(Z) if gs is None else gs.to(DEV, Z.dtype)
    Z.backward(g)
    torch.cuda.synchronize()
    return Z.detach().cpu(), xd.grad.cpu(), td.grad.cpu()


def _ref(x, tr, graph, il, lw=1.0, ts=0.0, gs=None):
    dt = np.float32 if x.dtype == torch.float32 else np.float64
    return full_graph_ref(x.double().numpy(), tr.double().numpy(), graph.next, graph.weight, graph.final, graph.start,
                          None if il is None else il.numpy(), lw, ts, None if gs is None else gs.numpy(), fold_dt=dt)


def _compare(got, want, dtype, what):
    Z, gx, gtr = got
    Zr, gxr, gtrr = want
    fin = np.isfinite(Zr)
    assert (np.isfinite(Z.numpy()) == fin).all(), what
    assert (Z.numpy()[~fin] == -np.inf).all(), what
    assert not torch.isnan(gx).any() and not torch.isnan(gtr).any(), what
    if dtype == torch.float64:
        assert np.allclose(Z.numpy()[fin], Zr[fin], rtol=1e-9, atol=1e-9), what
        assert np.allclose(gx.numpy(), gxr, rtol=1e-9, atol=1e-9), what
        assert np.allclose(gtr.numpy(), gtrr, rtol=1e-9, atol=1e-9), what
    else:
        assert_close(Z.numpy()[fin], Zr[fin], what=what + " Z")
        assert_close(gx.numpy(), gxr, what=what + " grad_inputs")
        assert_close(gtr.numpy(), gtrr, what=what + " grad_transition")


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("flags", [0, STREAM, RESIDENT])
def test_full_score_and_gradients_against_reference(name, dtype, flags):
    graph = GRAPHS[name]()
    x, tr, il = _case(9, 5, graph.N, 10, dtype)
    gs = torch.linspace(-1.0, 2.0, 5, dtype=torch.float64)
    for lw, ts in ((1.0, 0.0), (0.5, -0.25)):
        got = _full(x, tr, graph, il, lw, ts, flags, gs)
        _compare(got, _ref(x, tr, graph, il, lw, ts, gs), dtype, "%s %s flags=%d lw=%s" % (name, dtype, flags, lw))


@pytest.mark.parametrize("flags", [STREAM, RESIDENT])
def test_each_route_is_bit_identical_run_to_run_and_routes_agree(flags):
    graph = GRAPHS["trigram_holes"]()
    x, tr, il = _case(12, 7, graph.N, 3, torch.float32)
    a = _full(x, tr, graph, il, flags=flags)
    b = _full(x, tr, graph, il, flags=flags)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    other = _full(x, tr, graph, il, flags=STREAM + RESIDENT - flags)
    for u, v in zip(a, other):
        assert_close(u.numpy()[np.isfinite(u.numpy())], v.numpy()[np.isfinite(v.numpy())])


@pytest.mark.parametrize("N", list(range(1, 65, 9)) + [64, 128, 256])
def test_one_state_automaton_equals_asg_loss(N):
    torch_asg_amd = _asg()
    T, B = 12, 4
    g = torch.Generator().manual_seed(N)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1)
    tr = 0.3 * torch.randn(N, N, generator=g)
    tg = torch.randint(0, N, (B, 5), generator=g)
    il = torch.tensor([12, 9, 3, 7])
    tl = torch.tensor([5, 3, 5, 1])                       # utterance 2: tl > len (infeasible)
    m = torch_asg_amd.ASGLoss(N, reduction='none').to(DEV)
    with torch.no_grad():
        m.transition.copy_(tr)
    xa = x.to(DEV).requires_grad_(True)
    la = m(xa, tg.to(DEV), il.to(DEV), tl.to(DEV))
    la.sum().backward()
    ga, gta = xa.grad.cpu(), m.transition.grad.cpu()
    m.transition.grad = None
    xb = x.to(DEV).requires_grad_(True)
    lb = m.graph_loss(xb, tg.to(DEV), _one_state(N), il.to(DEV), tl.to(DEV), lm_weight=0.7)
    lb.sum().backward()
    torch.cuda.synchronize()
    assert torch.isinf(lb[2]) and lb[2] > 0 and torch.isinf(la[2])
    fin = torch.isfinite(la).cpu()
    assert_close(lb.detach().cpu()[fin].numpy(), la.detach().cpu()[fin].numpy(), what="loss")
    assert_close(xb.grad.cpu().numpy(), ga.numpy(), what="grad_inputs")
    assert_close(m.transition.grad.cpu().numpy(), gta.numpy(), what="grad_transition")


def test_posteriors_of_all_targets_sum_to_one_on_gpu():
    torch_asg_amd = _asg()
    T, N = 4, 3
    graph = _random_graph(6, N, 8)
    x, tr, _ = _case(T, 1, N, 2, torch.float64)
    ys = [y for L in range(1, T + 1) for y in itertools.product(range(N), repeat=L)
          if all(y[i] != y[i + 1] for i in range(L - 1))]
    tg = torch.full((len(ys), T), 0, dtype=torch.int64)
    for k, y in enumerate(ys):
        tg[k, :len(y)] = torch.tensor(y)
    tl = torch.tensor([len(y) for y in ys])
    xs = x.expand(T, len(ys), N).contiguous()
    loss = torch_asg_amd.graph_asg_loss(xs.to(DEV), tg.to(DEV), tr.to(DEV), graph, None, tl.to(DEV), 0.7, 0.2)
    assert abs(float(torch.logsumexp(-loss, 0))) < 1e-9


def test_gradcheck_float64():
    torch_asg_amd = _asg()
    graph = _ngram(3, 2, 7)
    x, tr, _ = _case(4, 2, 3, 1, torch.float64)
    tg = torch.tensor([[0, 2], [1, 1]]).to(DEV)
    il = torch.tensor([4, 3]).to(DEV)

    def f(xx, tt):
        return torch_asg_amd.graph_asg_loss(xx, tg, tt, graph, il, None, 0.9, 0.1)
    assert torch.autograd.gradcheck(f, (x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)), atol=1e-7)


def test_no_grad_call_allocates_no_alpha():
    graph = _ngram(10, 2, 2)
    T, B = 300, 64
    x, tr, il = _case(T, B, 10, 1, torch.float32)
    xd, td = x.to(DEV), tr.to(DEV)
    _asg().graph_full_score(xd, td, graph)                # warm: compiled graph, library loaded
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        _asg().graph_full_score(xd, td, graph, lm_weight=1.0)
    torch.cuda.synchronize()
    Q = graph.compile(DEV, torch.float32)["Q"]
    assert torch.cuda.max_memory_allocated() - base < T * Q * B * 4 // 4


def test_four_gram_streaming_against_reference():
    graph = _ngram(40, 4, 9)                              # Q = 65640 product states
    x, tr, il = _case(4, 3, 40, 5, torch.float64)
    got = _full(x, tr, graph, il, flags=0)
    assert graph.compile(DEV, torch.float64)["Q"] == 65640
    _compare(got, _ref(x, tr, graph, il), torch.float64, "4-gram")


def test_infeasible_utterances_are_inf_without_nan():
    torch_asg_amd = _asg()
    graph = GRAPHS["random"]()
    N = graph.N
    x, tr, _ = _case(6, 5, N, 4, torch.float32)
    il = torch.tensor([6, 0, 2, 6, 6])
    tg = torch.tensor([[1, 2, 3], [1, 0, 0], [1, 2, 3], [0, 0, 0], [2, 2, 5]])
    tl = torch.tensor([3, 1, 3, 0, 3])
    xd = x.to(DEV).requires_grad_(True)
    td = tr.to(DEV).requires_grad_(True)
    loss = torch_asg_amd.graph_asg_loss(xd, tg.to(DEV), td, graph, il.to(DEV), tl.to(DEV))
    loss.sum().backward()
    torch.cuda.synchronize()
    l = loss.detach().cpu()
    assert not torch.isnan(l).any() and l[1] == float("inf") and l[2] == float("inf") and l[3] == float("inf")
    assert not torch.isnan(xd.grad).any() and not torch.isnan(td.grad).any()
    assert (xd.grad[:, 1] == 0).all()
    # a neighbour's loss does not depend on the others
    xs = x[:, [0]].to(DEV)
    l0 = torch_asg_amd.graph_asg_loss(xs, tg[[0]].to(DEV), tr.to(DEV), graph, il[[0]].to(DEV), tl[[0]].to(DEV))
    assert torch.equal(l0.cpu()[0], l[0])
    # the target walk against the reference
    walk = _asg().asg.native().graph_target_scores(x.to(DEV), tr.to(DEV), graph, tg.to(DEV), tl.to(DEV))
    want = target_scores_ref(tg.numpy(), tl.numpy(), graph.next, graph.weight, graph.final, graph.start, fold_dt=np.float32)
    assert np.array_equal(np.isfinite(walk.cpu().numpy()), np.isfinite(want))
    assert_close(walk.cpu().numpy()[np.isfinite(want)], want[np.isfinite(want)])


def test_strided_batch_major_view_equals_contiguous():
    graph = GRAPHS["bigram"]()
    x, tr, il = _case(8, 4, graph.N, 6, torch.float32)
    bt = x.transpose(0, 1).contiguous()                   # [B,T,N]
    a = _full(x, tr, graph, il)
    xd = bt.to(DEV).transpose(0, 1).requires_grad_(True)
    Z = _asg().graph_full_score(xd, tr.to(DEV), graph, il.to(DEV))
    Z.sum().backward()
    assert torch.equal(Z.detach().cpu(), a[0]) and torch.equal(xd.grad.cpu(), a[1])


def test_small_work_budget_groups_utterances():
    graph = GRAPHS["bigram"]()
    x, tr, il = _case(8, 5, graph.N, 7, torch.float64)
    a = _full(x, tr, graph, il)
    b = _full(x, tr, graph, il, max_work_bytes=1)
    for u, v in zip(a, b):
        assert torch.allclose(u, v, rtol=1e-12, atol=1e-12, equal_nan=True)


@pytest.mark.parametrize("flags", [STREAM, RESIDENT])
def test_capture_and_replay_matches_eager(flags):
    graph = GRAPHS["bigram"]()
    N = graph.N
    x, tr, il = _case(10, 4, N, 8, torch.float32)
    xs = x.to(DEV).requires_grad_(True)
    trd = tr.to(DEV).requires_grad_(True)
    ils = il.to(DEV)
    GF = _asg().GraphFullScore

    def step():
        xs.grad = None
        trd.grad = None
        Z = GF.apply(xs, trd, graph, ils, 1.0, 0.0, 1 << 30, flags)
        torch.where(torch.isfinite(Z), Z, torch.zeros_like(Z)).sum().backward()
        return Z
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                            # warm
    torch.cuda.current_stream().wait_stream(s)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        Zc = step()
    x2, _, il2 = _case(10, 4, N, 9, torch.float32)
    with torch.no_grad():
        xs.copy_(x2.to(DEV))
        ils.copy_(il2.to(DEV))
    cg.replay()
    torch.cuda.synchronize()
    got = (Zc.detach().cpu().clone(), xs.grad.cpu().clone(), trd.grad.cpu().clone())
    want = _full(x2, tr, graph, il2, flags=flags)
    for u, v in zip(got, want):
        assert torch.equal(u, v)


def test_errors():
    torch_asg_amd = _asg()
    graph = GRAPHS["bigram"]()
    N = graph.N
    x, tr, il = _case(5, 2, N, 1, torch.float32)
    with pytest.raises(RuntimeError, match="over %d tokens" % N):
        torch_asg_amd.graph_full_score(x[:, :, :N - 1].contiguous().to(DEV), tr[:N - 1, :N - 1].contiguous().to(DEV), graph)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch_asg_amd.graph_full_score(x, tr, graph)
    with pytest.raises(RuntimeError, match="Float or Double"):
        torch_asg_amd.asg.native().graph_full_forward(x.to(DEV, torch.float16), tr.to(DEV, torch.float16), graph, None)
    with pytest.raises(TypeError, match="TokenGraph"):
        torch_asg_amd.graph_full_score(x.to(DEV), tr.to(DEV), "graph")


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("scale_mode", ["none", "input_size", "target_size_sqrt"])
def test_asg_loss_graph_loss_reductions_and_scale_mode(reduction, scale_mode):
    torch_asg_amd = _asg()
    graph = GRAPHS["bigram"]()
    N = graph.N
    x, tr, _ = _case(8, 3, N, 12, torch.float64)
    il = torch.tensor([8, 6, 7])
    tg = torch.tensor([[1, 2, 3], [4, 5, 5], [0, 9, 2]])
    tl = torch.tensor([3, 2, 3])
    m = torch_asg_amd.ASGLoss(N, reduction=reduction, scale_mode=scale_mode).to(DEV).double()
    with torch.no_grad():
        m.transition.copy_(tr)
    per = torch_asg_amd.graph_asg_loss(x.to(DEV), tg.to(DEV), m.transition.detach(), graph, il.to(DEV), tl.to(DEV)).cpu()
    if scale_mode == "input_size":
        per = per / il.double()
    elif scale_mode == "target_size_sqrt":
        per = per / tl.double().sqrt()
    want = {"none": per, "sum": per.sum(), "mean": per.mean()}[reduction]
    got = m.graph_loss(x.to(DEV), tg.to(DEV), graph, il.to(DEV), tl.to(DEV)).detach().cpu()
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    # a float16 view widens to the module's dtype
    h = m.graph_loss(x.to(DEV, torch.float16), tg.to(DEV), graph, il.to(DEV), tl.to(DEV))
    assert h.dtype == torch.float64
