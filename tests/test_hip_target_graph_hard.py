"""GPU tests (-m gpu) of the Viterbi (hard) score over target graphs and its loss (csrc/asg_target_graph_hard.hip) against
the numpy restatement of the best path (tests/target_graph_viterbi_ref.py).  With small integer grad_scores every product and
sum of the gradients is exact in float32, so they are compared for equality."""
import numpy as np
import pytest
import torch
import torch_asg_amd as A

from target_graph_viterbi_ref import target_graph_viterbi_ref, tie_case
from test_hip_target_graph import DEV, DTYPES, NI, _batch, _case, _mixed, _skips
from util import assert_close

pytestmark = pytest.mark.gpu
both = pytest.mark.parametrize("dtype", DTYPES)


def _ints(B):
    return torch.tensor([1.0, 2.0, 3.0, -1.0, 0.0], dtype=torch.float64).repeat(B // 5 + 1)[:B]


def _run(x, tr, graphs, il, gs):
    xd, td = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
    Z = A.target_graph_viterbi_score(xd, td, graphs, None if il is None else il.to(DEV))
    Z.backward(gs.to(DEV, Z.dtype))
    torch.cuda.synchronize()
    return Z.detach().cpu(), xd.grad.cpu(), td.grad.cpu()


def _check(x, tr, graphs, il, gs, what, exact=True, got=None):
    """Scores against the restatement in the dtype of x, gradients against the one-hot and pair counts of its path in float64."""
    Z, gx, gtr = got or _run(x, tr, graphs, il, gs)
    T, B, N = x.shape
    scores, _, labels = target_graph_viterbi_ref(x.numpy(), tr.numpy(), graphs.graphs, None if il is None else il.numpy())[:3]
    gxr, gtrr = np.zeros((T, B, N)), np.zeros((N, N))
    for b, g in enumerate(gs.tolist()):
        n = int((labels[b] >= 0).sum())
        gxr[np.arange(n), b, labels[b, :n]] = g
        np.add.at(gtrr, (labels[b, 1:n], labels[b, :max(n - 1, 0)]), g)
    with torch.no_grad():                             # the zero-workspace route, and the path the decoder reports
        ild = None if il is None else il.to(DEV)
        Z0 = A.target_graph_viterbi_score(x.to(DEV), tr.to(DEV), graphs, ild)
        r = A.target_graph_viterbi(x.to(DEV), tr.to(DEV), graphs, ild)
    assert Z.dtype == x.dtype and np.array_equal(Z.numpy(), scores) and torch.equal(Z0.cpu(), Z) and torch.equal(r.scores.cpu(), Z), what
    assert np.array_equal(r.labels.cpu().numpy(), labels), what
    for name, g, w in ((" grad_inputs", gx.numpy(), gxr), (" grad_transition", gtr.numpy(), gtrr)):
        if exact:
            assert np.array_equal(g, w), what + name
        elif x.dtype == torch.float64:
            assert np.allclose(g, w, rtol=1e-9, atol=1e-9), what + name
        else:
            assert_close(g, w, what=what + name)
    return scores


@both
@pytest.mark.parametrize("exact", [True, False])
def test_mixed_batch_and_integer_ties(exact, dtype):
    graphs, T, N, il = _mixed()
    x, tr, gs = _case(T, graphs.B, N, 1, dtype)       # (gs: ten values from -1 to 2, no integers but the ends)
    scores = _check(x, tr, graphs, il, _ints(graphs.B) if exact else gs, "mixed", exact)
    assert list(np.isfinite(scores)) == [False, True, True, True, True, True, False, False, False, True]
    if exact:                                         # 5aj's ties: the counted path is the one target_graph_viterbi reports
        x, tr, graphs = tie_case(70, 1)
        _check(torch.from_numpy(x).to(dtype), torch.from_numpy(tr).to(dtype), graphs, None, _ints(2), "ties")


@both
@pytest.mark.parametrize("K", [64, 65, 256, 257, 1024])
def test_widths_and_staging_blocks(K, dtype):
    F = 64 if K <= 256 else 16                        # frames per staged block of that width
    il = torch.tensor([1, 2, F - 1, F, F + 1, 2 * F + 1])
    graphs = _batch([_skips(K, 12, K + b) for b in range(6)], 12)
    x, tr, _ = _case(2 * F + 1, 6, 12, K, dtype)
    assert graphs.Kmax == K and np.isfinite(_check(x, tr, graphs, il, _ints(6), "K=%d" % K)).all()


@both
@pytest.mark.parametrize("N", [1, 5, 41])
def test_parallel_edges_and_the_dense_write(N, dtype):
    """Two parallel edges 0 -> 1 of different weight (either order), and [T,B,N] of 15, 75 and 615 elements: whole 16-byte
    granules that straddle rows, and a partial last one.  One label admits only the one-node graph."""
    edges = [(0, 1, -0.3), (0, 1, 0.5), (1, 2, 0.1), (0, 2, -1.0)]
    spec = lambda ed: ([0, 1, 2], [0.0, NI, NI], [NI, -0.1, 0.2], ed) if N > 1 else ([0], [0.0], [0.2], [])
    graphs = _batch([spec(edges), spec(edges[1::-1] + edges[2:]), spec(edges[:1] + edges[2:])], N)
    x, tr, _ = _case(5, 3, N, N, dtype)
    assert np.isfinite(_check(x, tr, graphs, torch.tensor([5, 4, 2]), _ints(3), "N=%d" % N)).all()


@both
def test_edge_count_at_the_lds_bound(dtype):
    N, K = 8, 8
    bound = int(A._lib.lib().asg_target_graph_max_edges(int(dtype == torch.float64), K))
    rng = np.random.default_rng(5)
    src = rng.integers(0, K, bound)
    dst = (src + rng.integers(1, K, bound)) % K                             # parallel edges, never a self edge
    ed = [(int(s), int(d), float(w)) for s, d, w in zip(src, dst, rng.normal(size=bound) - 7.0)]
    lab, w = list(range(K)), list(rng.normal(size=K))
    x, tr, _ = _case(3, 2, N, 6, dtype)
    graphs = _batch([(lab, w, w, ed), (lab[:2], w[:2], w[:2], ed[:0])], N)
    assert graphs.Emax == bound and np.isfinite(_check(x, tr, graphs, None, _ints(2), "at the bound")).all()


@both
def test_chains_equal_viterbi_align(dtype):
    T, B, N, S = 70, 4, 7, 30
    tg = torch.from_numpy(np.cumsum(np.random.default_rng(S).integers(1, N, (B, S)), 1) % N)
    tl, il = torch.tensor([S, S - 3, S, S // 2]), torch.tensor([T, 66, S - 1, T])    # utterance 2: shorter than its targets
    x, tr, _ = _case(T, B, N, S, dtype)
    graphs = A.TargetGraphs.from_targets(tg, tl, N)
    Z, gx, _ = got = _run(x, tr, graphs, il, _ints(B))
    _check(x, tr, graphs, il, _ints(B), "chains", got=got)
    scores, pos, _ = A.viterbi_align(x.to(DEV), tg.to(DEV), tr.to(DEV), il.to(DEV), tl.to(DEV))
    lab = torch.where(pos >= 0, tg.to(DEV).gather(1, pos.clamp(min=0)), N).t().cpu()           # [T,B], N: no path here
    want = torch.nn.functional.one_hot(lab, N + 1)[:, :, :N].to(dtype) * _ints(B).to(dtype)[:, None]
    assert torch.equal(scores.cpu(), Z) and Z[2] == NI and torch.equal(gx, want)


@both
def test_loss_and_module_against_fcc_minus_score(dtype):
    graphs, T, N, il = _mixed()
    x, tr, _ = _case(T, graphs.B, N, 4, dtype)
    m = A.ASGLoss(N, reduction='mean').to(DEV).to(dtype)
    m.transition.data.copy_(tr)
    ild, fin = il.to(DEV), torch.tensor([False, True, True, True, True, True, False, False, False, True], device=DEV)
    xa, xb, xc, ta, tb = (v.to(DEV).requires_grad_(True) for v in (x, x, x, tr, tr))
    full = A.FCC.apply(ta, xa, None, ild, None)
    hard = A.target_graph_viterbi_score(xa, ta, graphs, ild)
    want = torch.where(fin, full - torch.where(fin, hard, torch.zeros_like(hard)), torch.full_like(full, float("inf")))
    loss = A.target_graph_viterbi_loss(xb, graphs, tb, ild)
    assert torch.equal(torch.isinf(loss), ~fin) and (loss[~fin] > 0).all()
    assert_close(loss[fin].detach().cpu().numpy(), want[fin].detach().cpu().numpy(), what="loss")
    (torch.where(torch.isfinite(full), full, torch.zeros_like(full)).sum() - hard[fin].sum()).backward()     # +inf rows: FCC only
    loss.sum().backward()
    assert not torch.isnan(xb.grad).any() and not torch.isnan(tb.grad).any()
    assert_close(xb.grad.cpu().numpy(), xa.grad.cpu().numpy(), what="loss grad_inputs")
    assert_close(tb.grad.cpu().numpy(), ta.grad.cpu().numpy(), what="loss grad_transition")
    assert torch.isinf(m.target_graph_viterbi_loss(xc, graphs, ild)).item()          # (one element: the mean)
    keep = torch.nonzero(fin).flatten().cpu()         # without the dead utterances the mean is finite
    sub = _batch([(f[0], f[1], f[2], list(zip(*f[3:]))) for f in (graphs.graphs[i] for i in keep)], N)
    mean = m.target_graph_viterbi_loss(xc[:, keep.to(DEV)], sub, ild[keep.to(DEV)])
    assert_close(mean.item(), want[fin].mean().item(), what="mean")


def test_strides_repeatability_and_two_replays_of_a_captured_step():
    graphs, T, N, il = _mixed()
    (x, tr, _), gs = _case(T, graphs.B, N, 2, torch.float32), _ints(graphs.B)
    first = _run(x, tr, graphs, il, gs)
    assert all(torch.equal(u, v) for u, v in zip(first, _run(x, tr, graphs, il, gs)))
    xs = torch.empty(graphs.B, T, N, device=DEV).transpose(0, 1).requires_grad_(True)      # batch-major emissions
    trd = tr.t().contiguous().to(DEV).t().requires_grad_(True)                           # a transposed transition
    ils, gsd = il.to(DEV), gs.to(DEV, torch.float32)

    def step():
        xs.grad = trd.grad = None
        Z = A.TargetGraphViterbiScore.apply(xs, trd, graphs, ils)
        Z.backward(gsd)
        return Z
    with torch.no_grad():
        xs.copy_(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Z = step()                                        # warm, and the strided route against the contiguous one
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip((Z.detach().cpu(), xs.grad.cpu(), trd.grad.cpu()), first))
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        Zc = step()
    for seed in (3, 2):                                   # two replays, each against the eager bits of its data
        x2 = _case(T, graphs.B, N, seed, torch.float32)[0]
        with torch.no_grad():
            xs.copy_(x2)
        cg.replay()
        torch.cuda.synchronize()
        got = (Zc.detach().cpu().clone(), xs.grad.cpu().clone(), trd.grad.cpu().clone())
        assert all(torch.equal(u, v) for u, v in zip(got, _run(x2, tr, graphs, il, gs)))
