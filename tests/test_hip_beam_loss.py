"""GPU tests (-m gpu) of the beam-pruned ASG loss composed with a token automaton (`torch_asg_amd.beam_graph_full_score`,
`beam_graph_asg_loss`, `ASGLoss.beam_graph_loss`; csrc/asg_beam_loss.hip) against the numpy restatement tests/beam_loss_ref.py
with the project's parity rule (util.assert_close, scaled 1e-4 in float32; 1e-9 in float64 -- BASELINE.md section 2, as
tests/test_hip_graph_loss.py): scores, gradients and losses over several automata and beams, the whole-beam identity against the
exact route, the subset relations, determinism, gradcheck, capture, the streamed 4-gram, workspace sizes and errors."""
import ctypes

import numpy as np
import pytest
import torch

from beam_loss_cases import (DEV, GRAPHS, INF, _asg, _case, _compare, _full, _lexicon, _ngram, _one_state, _ref, _targets)
from util import assert_close

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_scores_and_gradients_against_reference(name, dtype):
    graph = GRAPHS[name]()
    B = 6
    x, tr, il = _case(9, B, graph.N, 10, dtype)
    gs = torch.linspace(-1.0, 2.0, B, dtype=torch.float64)
    tg, tl = _targets(B, 4, graph.N, il, 3)
    Q = graph.compile_host(np.float32)["Q"]
    for K in (1, 3, 16, 64, Q + 5):
        for th in (INF, 2.0):
            for tgt in (None, (tg, tl)):
                a, b = tgt if tgt else (None, None)
                lw, ts = (1.0, 0.0) if K != 3 else (0.5, -0.25)
                got = _full(x, tr, graph, il, K, th, lw, ts, gs, a, b)
                want = _ref(x, tr, graph, il, K, th, lw, ts, gs, a, b)
                what = "%s %s K=%d th=%s targets=%s" % (name, dtype, K, th, tgt is not None)
                _compare(got, want, dtype, what)
                Z, gx, _ = got
                # rows: the label posteriors of a frame sum to grad_scores[b]; exact zeros behind the utterance
                for b_ in range(B):
                    L = int(il[b_])
                    assert (gx[L:, b_] == 0).all(), what
                    if np.isfinite(float(Z[b_])) and L:
                        tol = 1e-9 if dtype == torch.float64 else 1e-4
                        assert np.allclose(gx[:L, b_].sum(-1).numpy(), float(gs[b_]), rtol=tol, atol=tol), what
                    else:
                        assert (gx[:, b_] == 0).all(), what


def test_lexicon_root_is_pulled_from_both_sides():
    """The trie's root has one incoming edge per word end: with a beam below that in-degree the kernel walks U_{t-1} and
    searches the row; with the whole beam it walks the row."""
    graph = _lexicon(12, 300, 9, maxlen=3)
    h = graph.compile_host(np.float64)
    indeg = int(np.diff(h["row"]).max())
    assert indeg > 64
    x, tr, il = _case(12, 3, graph.N, 4, torch.float64)
    for K in (8, 32, h["Q"]):
        assert K < indeg or K == h["Q"]
        _compare(_full(x, tr, graph, il, K), _ref(x, tr, graph, il, K), torch.float64, "lexicon K=%d" % K)


@pytest.mark.parametrize("N", [1, 2, 7, 33, 64])
def test_whole_beam_equals_the_exact_route_one_state(N):
    A = _asg()
    graph = _one_state(N)
    x, tr, il = _case(10, 4, N, N, torch.float32)
    tg, tl = _targets(4, 3, N, il, 1)
    dv = lambda t: t.to(DEV)
    Z = A.beam_graph_full_score(dv(x), dv(tr), graph, dv(il), beam_size=N + 1)
    assert_close(Z.cpu().numpy(), A.graph_full_score(dv(x), dv(tr), graph, dv(il)).cpu().numpy())
    la = A.beam_graph_asg_loss(dv(x), dv(tg), dv(tr), graph, dv(il), dv(tl), beam_size=N)
    lb = A.graph_asg_loss(dv(x), dv(tg), dv(tr), graph, dv(il), dv(tl))
    assert torch.equal(torch.isinf(la), torch.isinf(lb)) and not torch.isnan(la).any()
    fin = torch.isfinite(lb).cpu().numpy()
    assert_close(la.cpu().numpy()[fin], lb.cpu().numpy()[fin])


@pytest.mark.parametrize("name", ["bigram", "trigram_holes"])
def test_whole_beam_equals_the_exact_route(name):
    A = _asg()
    graph = GRAPHS[name]()
    N = graph.N
    x, tr, il = _case(11, 5, N, 21, torch.float64)
    tg, tl = _targets(5, 4, N, il, 2)
    Q = graph.compile_host(np.float64)["Q"]
    dv = lambda t: t.to(DEV)
    outs = []
    for fn in (lambda a, b: A.beam_graph_asg_loss(a, dv(tg), b, graph, dv(il), dv(tl), beam_size=Q),
               lambda a, b: A.graph_asg_loss(a, dv(tg), b, graph, dv(il), dv(tl))):
        xd, td = dv(x).requires_grad_(True), dv(tr).requires_grad_(True)
        l = fn(xd, td)
        torch.where(torch.isfinite(l), l, torch.zeros_like(l)).sum().backward()
        outs.append((l.detach().cpu(), xd.grad.cpu(), td.grad.cpu()))
    (la, ga, ta), (lb, gb, tb) = outs
    assert torch.equal(torch.isinf(la), torch.isinf(lb)) and not torch.isnan(la).any()
    fin = torch.isfinite(lb)
    assert torch.allclose(la[fin], lb[fin], rtol=1e-9, atol=1e-9)
    assert torch.allclose(ga, gb, rtol=1e-9, atol=1e-9) and torch.allclose(ta, tb, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_subset_relations_and_the_sign_of_the_loss(dtype):
    A = _asg()
    graph = GRAPHS["bigram"]()
    N = graph.N
    B = 8
    x, tr, il = _case(14, B, N, 5, dtype)
    tg, tl = _targets(B, 5, N, il, 7)
    tol = 1e-4 if dtype == torch.float32 else 1e-9
    dv = lambda t: t.to(DEV)
    Zx = A.graph_full_score(dv(x), dv(tr), graph, dv(il)).cpu()
    exact = A.graph_asg_loss(dv(x), dv(tg), dv(tr), graph, dv(il), dv(tl)).cpu()
    for K in (1, 2, 4, 16):
        for th in (INF, 1.0):
            Z = A.beam_graph_full_score(dv(x), dv(tr), graph, dv(il), K, th).cpu()
            sc = A.beam_decode_graph(dv(x), dv(tr), graph, dv(il), K, th)[0].cpu()
            assert not torch.isnan(Z).any()
            scale = max(1.0, float(Zx[torch.isfinite(Zx)].abs().max()))
            assert (Z <= Zx + tol * scale).all()
            assert (Z >= sc - tol * scale).all()
            loss = A.beam_graph_asg_loss(dv(x), dv(tg), dv(tr), graph, dv(il), dv(tl), K, th).cpu()
            assert not torch.isnan(loss).any()
            assert torch.equal(torch.isinf(loss), torch.isinf(exact)) and (loss[torch.isinf(loss)] > 0).all()
            assert (loss[torch.isfinite(loss)] >= -tol * scale).all()


def test_bit_identical_run_to_run_across_groupings_and_strides():
    graph = GRAPHS["trigram_holes"]()
    x, tr, il = _case(12, 7, graph.N, 3, torch.float32)
    tg, tl = _targets(7, 4, graph.N, il, 9)
    gs = torch.linspace(0.5, 1.5, 7)
    runs = [_full(x, tr, graph, il, 5, 3.0, gs=gs, tg=tg, tl=tl) for _ in range(3)]
    runs.append(_full(x, tr, graph, il, 5, 3.0, gs=gs, tg=tg, tl=tl, max_work_bytes=1))
    per = 3 * ctypes.sizeof(ctypes.c_double) * 100000
    runs.append(_full(x, tr, graph, il, 5, 3.0, gs=gs, tg=tg, tl=tl, max_work_bytes=per))
    for r in runs[1:]:
        for u, v in zip(runs[0], r):
            assert torch.equal(u, v)
    bt = x.transpose(0, 1).contiguous()
    xd = bt.to(DEV).transpose(0, 1).requires_grad_(True)
    Z = _asg().beam_graph_full_score(xd, tr.to(DEV), graph, il.to(DEV), 5, 3.0, targets=tg.to(DEV), target_lengths=tl.to(DEV))
    Z.backward(gs.to(DEV))
    assert torch.equal(Z.detach().cpu(), runs[0][0]) and torch.equal(xd.grad.cpu(), runs[0][1])


def test_gradcheck_float64_away_from_ties():
    A = _asg()
    graph = _ngram(4, 2, 7)
    found = None
    for seed in range(50):
        x, tr, _ = _case(5, 2, 4, seed, torch.float64)
        il = torch.tensor([5, 4])
        info = {}
        _ref(x, tr, graph, il, 2, 1.5, 0.9, 0.1, info=info)
        if info["margin"] > 1e-3:
            found = (x, tr, il, info["margin"])
            break
    assert found is not None
    x, tr, il, margin = found
    assert margin > 1e-3                                   # a perturbation of 1e-6 cannot move a set
    tg = torch.tensor([[0, 2], [1, 1]]).to(DEV)
    ild = il.to(DEV)

    def f(xx, tt):
        return A.beam_graph_asg_loss(xx, tg, tt, graph, ild, None, 2, 1.5, 0.9, 0.1)
    assert torch.autograd.gradcheck(f, (x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)), atol=1e-7)


def test_capture_and_replay_matches_eager():
    graph = GRAPHS["bigram"]()
    N = graph.N
    x, tr, il = _case(10, 4, N, 8, torch.float32)
    tg, tl = _targets(4, 3, N, il, 1)
    xs = x.to(DEV).requires_grad_(True)
    trd = tr.to(DEV).requires_grad_(True)
    ils, tgs, tls = il.to(DEV), tg.to(DEV), tl.to(DEV)
    F = _asg().BeamGraphFullScore

    def step():
        xs.grad = None
        trd.grad = None
        Z = F.apply(xs, trd, graph, ils, 3, 2.0, 1.0, 0.0, tgs, tls, 1 << 30)
        torch.where(torch.isfinite(Z), Z, torch.zeros_like(Z)).sum().backward()
        return Z
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        Zc = step()
    x2, _, il2 = _case(10, 4, N, 9, torch.float32)
    tg2, tl2 = _targets(4, 3, N, il2, 5)
    with torch.no_grad():
        xs.copy_(x2.to(DEV))
        ils.copy_(il2.to(DEV))
        tgs.copy_(tg2.to(DEV))
        tls.copy_(tl2.to(DEV))
    cg.replay()
    torch.cuda.synchronize()
    got = (Zc.detach().cpu().clone(), xs.grad.cpu().clone(), trd.grad.cpu().clone())
    fin = torch.isfinite(got[0])
    want = _full(x2, tr, graph, il2, 3, 2.0, gs=fin.double(), tg=tg2, tl=tl2)
    for u, v in zip(got, want):
        assert torch.equal(u, v)


def test_four_gram_against_reference():
    graph = _ngram(40, 4, 9)                               # Q = 65640: the exact route only streams this
    T, B, K = 60, 4, 256
    x, tr, il = _case(T, B, 40, 5, torch.float32)
    il[:] = torch.tensor([T, T - 7, 0, T // 2])
    tg, tl = _targets(B, 12, 40, il, 4)
    assert graph.compile(DEV, torch.float32)["Q"] == 65640
    got = _full(x, tr, graph, il, K, tg=tg, tl=tl)
    _compare(got, _ref(x, tr, graph, il, K, tg=tg, tl=tl), torch.float32, "4-gram")


def test_workspace_is_below_the_exact_route_and_independent_of_E():
    """A pure host check: T = 400, B = 64, the 4-gram over 40 tokens, K = 256."""
    from torch_asg_amd import _lib
    L = _lib.lib()
    Q, E, N, T, B, K = 65640, 2559960, 40, 400, 64, 256
    g = _lib.AsgTokenGraph()
    g.Q, g.E, g.N, g.dtype = Q, E, N, _lib.ASG_DTYPE_F32
    for n in ("label", "state", "row", "src", "src_label", "start_w", "final_w", "edge_w"):
        setattr(g, n, 8)
    gb = _lib.AsgTokenGraphBeam()
    gb.graph = ctypes.pointer(g)
    gb.num_start, gb.max_out = 40, 39
    for n in ("orow", "oarc", "ow", "start_q"):
        setattr(gb, n, 8)
    gl = _lib.AsgTokenGraphBeamLoss()
    gl.beam, gl.S, gl.start, gl.next = ctypes.pointer(gb), 1641, 0, 8
    ex = _lib.AsgTokenGraphLoss()
    ex.graph, ex.S, ex.start = ctypes.pointer(g), 1641, 0
    for n in ("tgt", "orow", "oedge", "lrow", "lq", "pkey", "pedge", "next", "arcw", "finw"):
        setattr(ex, n, 8)
    p = _lib.AsgProblem()
    p.inputs = p.transition = p.targets = 8
    p.T, p.B, p.N, p.S, p.dtype = T, B, N, 60, _lib.ASG_DTYPE_F32

    def mine():
        return (L.asg_beam_graph_full_work_bytes(ctypes.byref(p), ctypes.byref(gl), K, 1)
                + L.asg_beam_graph_full_scratch_bytes(ctypes.byref(p), ctypes.byref(gl), K))
    exact = L.asg_graph_full_work_bytes(ctypes.byref(p), ctypes.byref(ex), 1) + L.asg_graph_full_scratch_bytes(ctypes.byref(p), ctypes.byref(ex))
    a = mine()
    assert 0 < a < exact
    g.E = 4 * E
    assert mine() == a


def test_errors():
    A = _asg()
    graph = GRAPHS["bigram"]()
    N = graph.N
    x, tr, il = _case(5, 2, N, 1, torch.float32)
    xd, td = x.to(DEV), tr.to(DEV)
    with pytest.raises(ValueError, match="beam_size"):
        A.beam_graph_full_score(xd, td, graph, beam_size=0)
    with pytest.raises(ValueError, match="beam_threshold"):
        A.beam_graph_full_score(xd, td, graph, beam_threshold=-1.0)
    with pytest.raises(ValueError, match="beam_threshold"):
        A.beam_graph_asg_loss(xd, torch.zeros(2, 2, dtype=torch.int64, device=DEV), td, graph, beam_threshold=float("nan"))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.beam_graph_full_score(x, tr, graph)
    with pytest.raises(RuntimeError, match="dtype/device"):
        A.beam_graph_full_score(xd, td.double(), graph)
    with pytest.raises(RuntimeError, match="over %d tokens" % N):
        A.beam_graph_full_score(xd[:, :, :N - 1].contiguous(), td[:N - 1, :N - 1].contiguous(), graph)
    with pytest.raises(TypeError, match="TokenGraph"):
        A.beam_graph_full_score(xd, td, "graph")
    big = _one_state(1025)
    with pytest.raises(RuntimeError, match="status 2"):
        A.beam_graph_full_score(torch.zeros(3, 1, 1025, device=DEV), torch.zeros(1025, 1025, device=DEV), big)
    # a short work buffer through the C ABI
    from torch_asg_amd import _lib, graph as G
    be = A.asg.native()
    gl = G.abi_graph_beam_loss(graph.compile_beam_loss(torch.device(DEV), torch.float32))
    p, keep = be._problem(xd, td, None, None, None)
    need = _lib.lib().asg_beam_graph_full_work_bytes(ctypes.byref(p), ctypes.byref(gl), 4, 0)
    buf = torch.empty(need, dtype=torch.uint8, device=DEV)
    sc = torch.empty(2, device=DEV)
    rc = _lib.lib().asg_beam_graph_full_forward(None, ctypes.byref(p), ctypes.byref(gl), 4, INF, buf.data_ptr(), need - 1,
                                                sc.data_ptr(), 0, None)
    assert rc == 3


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("scale_mode", ["none", "input_size", "target_size_sqrt"])
def test_asg_loss_beam_graph_loss_reductions_and_scale_mode(reduction, scale_mode):
    A = _asg()
    graph = GRAPHS["bigram"]()
    N = graph.N
    x, tr, _ = _case(8, 3, N, 12, torch.float64)
    il = torch.tensor([8, 6, 7])
    tg = torch.tensor([[1, 2, 3], [4, 5, 5], [0, 9, 2]])
    tl = torch.tensor([3, 2, 3])
    m = A.ASGLoss(N, reduction=reduction, scale_mode=scale_mode).to(DEV).double()
    with torch.no_grad():
        m.transition.copy_(tr)
    per = A.beam_graph_asg_loss(x.to(DEV), tg.to(DEV), m.transition.detach(), graph, il.to(DEV), tl.to(DEV), 4, 3.0).cpu()
    if scale_mode == "input_size":
        per = per / il.double()
    elif scale_mode == "target_size_sqrt":
        per = per / tl.double().sqrt()
    want = {"none": per, "sum": per.sum(), "mean": per.mean()}[reduction]
    got = m.beam_graph_loss(x.to(DEV), tg.to(DEV), graph, il.to(DEV), tl.to(DEV), beam_size=4, beam_threshold=3.0).detach().cpu()
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    h = m.beam_graph_loss(x.to(DEV, torch.float16), tg.to(DEV), graph, il.to(DEV), tl.to(DEV), beam_size=4)
    assert h.dtype == torch.float64
