"""CPU tests that pin the test-side reference of the beam-pruned ASG loss (tests/beam_loss_ref.py): its search against
tests/beam_decode_ref.py, Z_K against exhaustive path enumeration, its gradients against central differences with the sets
frozen, the whole-beam identity against tests/graph_loss_ref.py, the loss's sign, the target cases, and the C ABI of
asg_beam_graph_full_* (symbols, sizes, argument checks) -- no kernel is launched here."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from beam_decode_ref import beam_decode_ref
from beam_loss_ref import beam_loss_ref, forced_sets, lattice, search
from graph_decode_ref import path_score_graph
from graph_loss_ref import Composed, full_graph_ref, target_scores_ref, _lse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_automaton(rng, S, N, accept_all=False):
    nxt = rng.integers(0, S, size=(S, N))
    nxt[rng.random(size=(S, N)) < 0.2] = -1
    w = rng.normal(size=(S, N))
    f = rng.normal(size=S)
    if not accept_all:
        f[rng.random(size=S) < 0.3] = -np.inf
    return nxt, w, f


def _ngram(rng, N, order, holes=False):
    import torch_asg_amd
    lp = np.log(rng.dirichlet(np.ones(N + 1), size=(N + 1,) * (order - 1))) if order > 1 else np.log(rng.dirichlet(np.ones(N + 1)))
    if holes:
        lp[rng.random(size=lp.shape) < 0.2] = -np.inf
    g = torch_asg_amd.TokenGraph.from_ngram(lp)
    return g.next, g.weight, g.final


def _Q(nxt, w, f):
    return Composed(nxt, w, f).Q


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("seed", range(4))
def test_search_equals_beam_decode_ref(seed, dt):
    rng = np.random.default_rng(100 + seed)
    N = int(rng.integers(3, 8))
    nxt, w, f = _ngram(rng, N, 2 + seed % 2, holes=bool(seed & 1)) if seed < 2 else _random_automaton(rng, 6, N)
    T, B = 9, 4
    x = rng.normal(size=(T, B, N)).astype(dt)
    tr = rng.normal(size=(N, N)).astype(dt)
    il = np.array([T, 0, 1, 6])
    for K, th in ((1, np.inf), (3, np.inf), (5, 1.5), (1000, np.inf), (4, 0.0)):
        sizes = []
        sc, path, _, _, states = beam_decode_ref(x, tr, nxt, w, f, 0, il, K, th, 0.8, 0.1, sizes=sizes)
        info = {}
        beam_loss_ref(x, tr, nxt, w, f, 0, il, K, th, 0.8, 0.1, info=info)
        k = 0
        for b in range(B):
            r = info["search"][b]
            L = int(il[b])
            assert (r["score"] == sc[b]) or (np.isneginf(r["score"]) and np.isneginf(sc[b]))
            if L:
                assert r["sizes"] == sizes[k]
                k += 1
                assert all(len(s) == n and (np.diff(s) > 0).all() for s, n in zip(r["sets"], r["sizes"]))
            if np.isfinite(sc[b]):
                assert np.array_equal(r["path"], path[b, :L]) and np.array_equal(r["states"], states[b, :L])


def _path_states(labels, nxt, present, start, comp):
    """product state at every frame of a label path, None if the automaton has no arc for it"""
    qs, s, prev = [], start, None
    for i in labels:
        if i != prev:
            if not present[s, i]:
                return None
            s = int(nxt[s, i])
        qs.append(int(np.nonzero((comp.state == s) & (comp.label == i))[0][0]))
        prev = i
    return qs


@pytest.mark.parametrize("seed", range(6))
def test_z_is_lse_over_exactly_the_paths_inside_the_sets(seed):
    rng = np.random.default_rng(300 + seed)
    for k in range(4):
        N, T = int(rng.integers(2, 4)), int(rng.integers(1, 6))
        nxt, w, f = _random_automaton(rng, int(rng.integers(2, 4)), N)
        x = rng.normal(size=(T, 1, N))
        tr = rng.normal(size=(N, N))
        K = int(rng.integers(1, 4))
        th = [np.inf, 1.0][k % 2]
        y = rng.integers(0, N, size=(1, 2))
        tg = y if k >= 2 else None
        Z, _, _, U = beam_loss_ref(x, tr, nxt, w, f, 0, None, K, th, 0.9, 0.2, targets=tg)
        comp = Composed(nxt, w, f, 0, 0.9, 0.2)
        sc = []
        for p in itertools.product(range(N), repeat=T):
            qs = _path_states(p, nxt, comp.present, 0, comp)
            if qs is None or any(q not in U[0][t] for t, q in enumerate(qs)):
                continue
            sc.append(path_score_graph(x[:, 0], tr, nxt, w, f, p, 0, 0.9, 0.2)[0])
        want = _lse(np.array(sc)) if sc else -np.inf
        if want == -np.inf:
            assert Z[0] == -np.inf
        else:
            assert abs(Z[0] - want) <= 1e-10 * max(1.0, abs(want)), (Z[0], want)


def test_gradients_match_central_differences_with_the_sets_frozen():
    rng = np.random.default_rng(7)
    T, N = 5, 3
    nxt, w, f = _random_automaton(rng, 3, N, accept_all=True)
    x = rng.normal(size=(T, 1, N))
    tr = rng.normal(size=(N, N))
    tg = np.array([[0, 2]])
    Z, gx, gtr, U = beam_loss_ref(x, tr, nxt, w, f, 0, None, 2, np.inf, 0.8, 0.1, targets=tg, grad_scores=[0.7])
    assert np.isfinite(Z).all()
    comp = Composed(nxt, w, f, 0, 0.8, 0.1)

    def F(xx, tt):
        return 0.7 * lattice(comp, xx[:, 0], tt, T, U[0])[0]
    h = 1e-6
    for idx in itertools.product(range(T), range(1), range(N)):
        d = np.zeros_like(x)
        d[idx] = h
        assert abs((F(x + d, tr) - F(x - d, tr)) / (2 * h) - gx[idx]) < 1e-6
    for idx in itertools.product(range(N), range(N)):
        d = np.zeros_like(tr)
        d[idx] = h
        assert abs((F(x, tr + d) - F(x, tr - d)) / (2 * h) - gtr[idx]) < 1e-6
    # a frame's label posteriors sum to one
    assert np.allclose(gx[:, 0].sum(-1), 0.7)


@pytest.mark.parametrize("seed", range(4))
def test_whole_beam_equals_the_exact_reference(seed):
    rng = np.random.default_rng(500 + seed)
    N = 4
    nxt, w, f = _ngram(rng, N, 2 + seed % 2, holes=True) if seed < 2 else _random_automaton(rng, 5, N)
    T, B = 6, 3
    x = rng.normal(size=(T, B, N))
    tr = rng.normal(size=(N, N))
    il = np.array([T, 0, 3])
    gs = np.array([1.0, 0.5, -2.0])
    Q = _Q(nxt, w, f)
    got = beam_loss_ref(x, tr, nxt, w, f, 0, il, Q + 3, np.inf, 0.7, 0.2, grad_scores=gs)
    want = full_graph_ref(x, tr, nxt, w, f, 0, il, 0.7, 0.2, grad_scores=gs)
    for a, c in zip(got[:3], want):
        assert np.allclose(a, c, rtol=1e-12, atol=1e-12)
    small = beam_loss_ref(x, tr, nxt, w, f, 0, il, 2, np.inf, 0.7, 0.2)[0]
    assert (small <= want[0] + 1e-12).all()
    sc = beam_decode_ref(x, tr, nxt, w, f, 0, il, 2, np.inf, 0.7, 0.2)[0]
    assert (small >= sc - 1e-12).all()


def _loss(x, tr, nxt, w, f, il, tg, tl, K, th=np.inf, lw=0.9, ts=0.1):
    from oracle import asg_oracle as orc
    Z = beam_loss_ref(x, tr, nxt, w, f, 0, il, K, th, lw, ts, targets=tg, target_lengths=tl)[0]
    fac = orc.aligned_forward(x, tg, tr, il, tl)[0]
    a = target_scores_ref(tg, tl, nxt, w, f, 0, lw, ts)
    al = fac + a
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(al), Z - al, np.inf), Z


@pytest.mark.parametrize("seed", range(4))
def test_loss_is_nonnegative_for_any_beam_and_exact_for_the_whole_beam(seed):
    rng = np.random.default_rng(700 + seed)
    N = 5
    nxt, w, f = _ngram(rng, N, 2) if seed < 2 else _random_automaton(rng, 4, N, accept_all=True)
    T, B = 8, 4
    x = rng.normal(size=(T, B, N))
    tr = rng.normal(size=(N, N))
    il = np.array([T, 5, 7, 3])
    tg = rng.integers(0, N, size=(B, 3))
    tg[1] = [2, 2, 3]                                             # a repeat in the target
    tl = np.array([3, 3, 2, 1])
    Q = _Q(nxt, w, f)
    from oracle import asg_oracle as orc
    exact_Z = full_graph_ref(x, tr, nxt, w, f, 0, il, 0.9, 0.1)[0]
    al = orc.aligned_forward(x, tg, tr, il, tl)[0] + target_scores_ref(tg, tl, nxt, w, f, 0, 0.9, 0.1)
    exact = np.where(np.isfinite(al), exact_Z - al, np.inf)
    for K in (1, 2, 4):
        loss, Z = _loss(x, tr, nxt, w, f, il, tg, tl, K)
        fin = np.isfinite(loss)
        assert np.array_equal(fin, np.isfinite(exact))
        assert (loss[fin] >= -1e-10).all(), loss
        assert (Z <= exact_Z + 1e-10).all()
    loss, _ = _loss(x, tr, nxt, w, f, il, tg, tl, Q)
    fin = np.isfinite(exact)
    assert np.array_equal(np.isfinite(loss), fin) and np.allclose(loss[fin], exact[fin], rtol=1e-12, atol=1e-12)


def test_target_cases():
    nxt = np.array([[1, 0, -1], [1, 0, 1]])
    w = np.zeros((2, 3))
    f = np.array([-np.inf, 0.0])
    c = Composed(nxt, w, f)
    # product states sorted by (state, label): (s0,l1)=0, (s1,l0)=1, (s1,l2)=2
    assert list(zip(c.state, c.label)) == [(0, 1), (1, 0), (1, 2)]
    F = forced_sets(c, [0, 0, 2], 4)                              # merged: 0 2 -> q = 1, 2; n = 2, L = 4
    assert [list(a) for a in F] == [[1], [1, 2], [1, 2], [2]]
    assert all(a.size == 0 for a in forced_sets(c, [2], 3))       # no arc on 2 from the start
    assert all(a.size == 0 for a in forced_sets(c, [0, 1], 3))    # ends in the non-accepting state 0
    assert all(a.size == 0 for a in forced_sets(c, [0, 2, 0], 2))  # tl > len
    assert all(a.size == 0 for a in forced_sets(c, [], 3))
    assert all(a.size == 0 for a in forced_sets(c, [0, 5], 3))    # a label outside the alphabet
    assert [list(a) for a in forced_sets(c, [0], 1)] == [[1]]
    assert forced_sets(c, [0], 0) == []
    # lengths 0 and 1 through the whole reference, K = 1: the forced state joins the kept one
    rng = np.random.default_rng(1)
    x = rng.normal(size=(3, 3, 3))
    x[0, :, 1] = 5.0                                              # the search starts on label 1
    tr = rng.normal(size=(3, 3))
    Z, gx, gtr, U = beam_loss_ref(x, tr, nxt, w, f, 0, [0, 1, 3], 1, np.inf, targets=np.array([[0, 2]] * 3),
                                  target_lengths=[1, 1, 2])
    assert Z[0] == -np.inf and U[0] == [] and not gx[:, 0].any()
    assert [list(a) for a in U[1]] == [[0, 1]] and np.isfinite(Z[1])
    assert list(U[2][0]) == [0, 1] and not np.isnan(gx).any() and not np.isnan(gtr).any()


# ---- C ABI -----------------------------------------------------------------------------------------------------------

NEW = ["asg_beam_graph_full_work_bytes", "asg_beam_graph_full_scratch_bytes", "asg_beam_graph_full_forward",
       "asg_beam_graph_full_backward"]


def test_abi_declares_and_exports_the_beam_loss_entry_points():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    import torch_asg_amd
    for n in ("beam_graph_full_score", "beam_graph_asg_loss", "BeamGraphFullScore"):
        assert hasattr(torch_asg_amd, n)
    assert hasattr(torch_asg_amd.ASGLoss, "beam_graph_loss") and hasattr(torch_asg_amd.TokenGraph, "compile_beam_loss")


def _host_view(graph, dt, T, B, S=0):
    """An asg_token_graph_beam_loss over HOST arrays (sizes and validation read no array) and a problem."""
    from torch_asg_amd import _lib
    h = graph.compile_host(dt)
    hb = graph.compile_beam_host(dt)
    keep = [h, hb]
    g = _lib.AsgTokenGraph()
    g.Q, g.E, g.N = h["Q"], h["E"], graph.N
    g.dtype = _lib.ASG_DTYPE_F32 if dt == np.float32 else _lib.ASG_DTYPE_F64
    for n in ("label", "state", "row", "src", "src_label", "start_w", "final_w", "edge_w"):
        setattr(g, n, h[n].ctypes.data)
    gb = _lib.AsgTokenGraphBeam()
    gb.graph = ctypes.pointer(g)
    gb.num_start, gb.max_out = hb["num_start"], hb["max_out"]
    for n in ("orow", "oarc", "ow", "start_q"):
        setattr(gb, n, hb[n].ctypes.data)
    nx = np.ascontiguousarray(graph.next.astype(np.int32))
    keep.append(nx)
    gl = _lib.AsgTokenGraphBeamLoss()
    gl.beam = ctypes.pointer(gb)
    gl.S, gl.start, gl.next = graph.S, graph.start, nx.ctypes.data
    p = _lib.AsgProblem()
    dummy = np.zeros(8, dt)
    keep.append(dummy)
    p.inputs, p.transition = dummy.ctypes.data, dummy.ctypes.data
    p.T, p.B, p.N, p.S, p.dtype = T, B, graph.N, max(S, 1), g.dtype
    if S:
        tg = np.zeros(8, np.int64)
        keep.append(tg)
        p.targets = tg.ctypes.data
    return p, gl, (g, gb, keep)


def test_sizes_and_argument_validation_without_gpu():
    import torch_asg_amd
    from torch_asg_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(0)
    graph = torch_asg_amd.TokenGraph(*_ngram(rng, 6, 2))
    p, gl, keep = _host_view(graph, np.float32, 50, 4, S=10)
    wb = L.asg_beam_graph_full_work_bytes
    a, b = wb(ctypes.byref(p), ctypes.byref(gl), 8, 0), wb(ctypes.byref(p), ctypes.byref(gl), 8, 1)
    assert 0 < a < b
    M = min(8, graph.compile_host(np.float32)["Q"]) + 10               # K + min(S, T)
    assert b - a >= 4 * (50 - 2) * M * 4                          # alpha [T][M] instead of two rows, per utterance
    assert L.asg_beam_graph_full_scratch_bytes(ctypes.byref(p), ctypes.byref(gl), 8) >= 4 * (2 * M * 4 + 36 * 8)
    fwd, bwd = L.asg_beam_graph_full_forward, L.asg_beam_graph_full_backward
    one = ctypes.c_void_p(1)
    assert fwd(None, ctypes.byref(p), ctypes.byref(gl), 0, 1.0, one, 1 << 40, one, 0, None) == 1          # beam_size < 1
    assert fwd(None, ctypes.byref(p), ctypes.byref(gl), 8, -1.0, one, 1 << 40, one, 0, None) == 1         # negative threshold
    assert fwd(None, ctypes.byref(p), ctypes.byref(gl), 8, float("nan"), one, 1 << 40, one, 0, None) == 1
    assert fwd(None, ctypes.byref(p), None, 8, 1.0, one, 1 << 40, one, 0, None) == 1
    assert fwd(None, ctypes.byref(p), ctypes.byref(gl), 8, 1.0, one, a - 1, one, 0, None) == 3            # short buffer
    assert fwd(None, ctypes.byref(p), ctypes.byref(gl), 8, 1.0, one, a, one, 64, None) == 3               # ... for a stored alpha
    assert bwd(None, ctypes.byref(p), ctypes.byref(gl), 8, one, b, one, one, one, one, one, 0, 0, None) == 3
    p.S = 5000                                                     # min(S, T) forced states above the limit needs T too
    p.T = 5000
    assert fwd(None, ctypes.byref(p), ctypes.byref(gl), 8, 1.0, one, 1 << 40, one, 0, None) == 2
    p.S, p.T = 10, 50
    big = torch_asg_amd.TokenGraph(np.zeros((1, 1025), np.int64), np.zeros((1, 1025)), np.zeros(1))
    p2, gl2, keep2 = _host_view(big, np.float32, 5, 1)
    assert fwd(None, ctypes.byref(p2), ctypes.byref(gl2), 8, 1.0, one, 1 << 40, one, 0, None) == 2        # N > 1024
    ok = torch_asg_amd.TokenGraph(np.zeros((1, 256), np.int64), np.zeros((1, 256)), np.zeros(1))
    p3, gl3, keep3 = _host_view(ok, np.float64, 5, 1)
    assert wb(ctypes.byref(p3), ctypes.byref(gl3), 8192, 1) > 0                                              # N = 256, K = 8192 in fp64


def test_workspace_follows_the_beam_and_not_the_edges():
    """T = 400, B = 64, a 4-gram over 40 tokens, K = 256: below the exact route's alpha + scratch, and unchanged when E grows
    at fixed Q, K and max_out (the formula in include/asg_hip.h has no E in it)."""
    from torch_asg_amd import _lib
    L = _lib.lib()
    Q, E, N, T, B, K = 65640, 2559960, 40, 400, 64, 256
    g = _lib.AsgTokenGraph()
    g.Q, g.E, g.N, g.dtype = Q, E, N, _lib.ASG_DTYPE_F32
    one = 8
    for n in ("label", "state", "row", "src", "src_label", "start_w", "final_w", "edge_w"):
        setattr(g, n, one)
    gb = _lib.AsgTokenGraphBeam()
    gb.graph = ctypes.pointer(g)
    gb.num_start, gb.max_out = 40, 39
    for n in ("orow", "oarc", "ow", "start_q"):
        setattr(gb, n, one)
    gl = _lib.AsgTokenGraphBeamLoss()
    gl.beam, gl.S, gl.start, gl.next = ctypes.pointer(gb), 1641, 0, one
    p = _lib.AsgProblem()
    p.inputs = p.transition = p.targets = one
    p.T, p.B, p.N, p.S, p.dtype = T, B, N, 60, _lib.ASG_DTYPE_F32
    mine = (L.asg_beam_graph_full_work_bytes(ctypes.byref(p), ctypes.byref(gl), K, 1)
            + L.asg_beam_graph_full_scratch_bytes(ctypes.byref(p), ctypes.byref(gl), K))
    exact = T * Q * B * 4 + (2 * Q * B * 4 + (Q + E) * B * 4)        # asg_graph_full_work_bytes(store=1) + scratch, include/asg_hip.h
    assert 0 < mine < exact // 20, (mine, exact)
    g.E = 4 * E
    again = (L.asg_beam_graph_full_work_bytes(ctypes.byref(p), ctypes.byref(gl), K, 1)
             + L.asg_beam_graph_full_scratch_bytes(ctypes.byref(p), ctypes.byref(gl), K))
    assert again == mine
