"""CPU tests of the ASG loss composed with a token automaton: the test-side reference (tests/graph_loss_ref.py) against exhaustive
path enumeration, central differences, the oracle's full-lattice score and the normalisation identity, and the C ABI of
asg_graph_full_* / asg_graph_target_scores (symbols, sizes, argument checks) -- no kernel is launched here."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from graph_decode_ref import path_score_graph
from graph_loss_ref import full_graph_ref, target_scores_ref, _lse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_automaton(rng, S, N):
    nxt = rng.integers(0, S, size=(S, N))
    nxt[rng.random(size=(S, N)) < 0.25] = -1                      # missing arcs
    if S > 2:
        nxt[nxt == S - 1] = 0                                     # state S-1 is never entered
    w = rng.normal(size=(S, N))
    w[rng.random(size=(S, N)) < 0.1] = -np.inf                    # present but weighing -inf: absent too
    f = rng.normal(size=S)
    f[rng.random(size=S) < 0.3] = -np.inf                         # non-accepting states
    return nxt, w, f


def _ngram(rng, N, order, holes):
    import torch_asg_amd
    lp = np.log(rng.dirichlet(np.ones(N + 1), size=(N + 1,) * (order - 1))) if order > 1 else np.log(rng.dirichlet(np.ones(N + 1)))
    if holes:
        lp[rng.random(size=lp.shape) < 0.25] = -np.inf
    g = torch_asg_amd.TokenGraph.from_ngram(lp)
    return g.next, g.weight, g.final


FOLDS = [(1.0, 0.0), (0.5, -0.3), (2.0, 1.25)]


@pytest.mark.parametrize("seed", range(8))
def test_reference_full_score_against_exhaustive_enumeration(seed):
    rng = np.random.default_rng(900 + seed)
    for k in range(6):
        T, B, N = int(rng.integers(1, 6)), int(rng.integers(1, 4)), int(rng.integers(2, 5))
        if k % 2:
            nxt, w, f = _random_automaton(rng, int(rng.integers(1, 5)), N)
        else:
            nxt, w, f = _ngram(rng, N, int(rng.integers(1, 4)), holes=True)
        lw, ts = FOLDS[int(rng.integers(len(FOLDS)))]
        x = rng.normal(size=(T, B, N))
        tr = rng.normal(size=(N, N))
        il = rng.integers(0, T + 1, size=B)
        il[0] = T
        Z, _, _ = full_graph_ref(x, tr, nxt, w, f, 0, il, lw, ts)
        for b in range(B):
            L = int(il[b])
            if L == 0:
                assert Z[b] == -np.inf
                continue
            sc = [path_score_graph(x[:, b], tr, nxt, w, f, p, 0, lw, ts)[0] for p in itertools.product(range(N), repeat=L)]
            want = _lse(np.array(sc))
            if want == -np.inf:
                assert Z[b] == -np.inf
            else:
                assert abs(Z[b] - want) <= 1e-10 * max(1.0, abs(want)), (Z[b], want)


def test_reference_gradients_match_central_differences():
    rng = np.random.default_rng(5)
    T, B, N = 4, 2, 3
    nxt, w, f = _random_automaton(rng, 3, N)
    f[:] = 0.0
    x = rng.normal(size=(T, B, N))
    tr = rng.normal(size=(N, N))
    il = np.array([4, 3])
    gs = np.array([0.7, -1.3])
    Z, gx, gtr = full_graph_ref(x, tr, nxt, w, f, 0, il, 0.8, 0.1, grad_scores=gs)
    assert np.isfinite(Z).all()

    def F(xx, tt):
        return float(gs @ full_graph_ref(xx, tt, nxt, w, f, 0, il, 0.8, 0.1)[0])
    h = 1e-6
    for idx in itertools.product(range(T), range(B), range(N)):
        d = np.zeros_like(x)
        d[idx] = h
        assert abs((F(x + d, tr) - F(x - d, tr)) / (2 * h) - gx[idx]) < 1e-6
    for idx in itertools.product(range(N), range(N)):
        d = np.zeros_like(tr)
        d[idx] = h
        assert abs((F(x, tr + d) - F(x, tr - d)) / (2 * h) - gtr[idx]) < 1e-6


@pytest.mark.parametrize("lw", [1.0, 0.3])
def test_one_state_automaton_equals_the_oracle_full_score(lw):
    from oracle import asg_oracle as orc
    rng = np.random.default_rng(11)
    T, B, N = 7, 4, 5
    x = rng.normal(size=(T, B, N))
    tr = rng.normal(size=(N, N))
    il = np.array([7, 5, 1, 3])
    Z, gx, gtr = full_graph_ref(x, tr, np.zeros((1, N), np.int64), np.zeros((1, N)), np.zeros(1), 0, il, lw, 0.0)
    want = orc.full_forward(x, tr, il)[0]
    assert np.allclose(Z, want, rtol=1e-12, atol=1e-12)


def test_posteriors_of_all_targets_sum_to_one():
    """Targets without consecutive repeats partition the label paths: logsumexp_y(-loss(y)) = 0."""
    from oracle import asg_oracle as orc
    rng = np.random.default_rng(3)
    T, N = 4, 3
    for k in range(3):
        nxt, w, f = _random_automaton(rng, 3, N) if k else _ngram(rng, N, 2, holes=True)
        x = rng.normal(size=(T, 1, N))
        tr = rng.normal(size=(N, N))
        Z = full_graph_ref(x, tr, nxt, w, f, 0, None, 0.7, 0.2)[0][0]
        if Z == -np.inf:
            continue
        terms = []
        for L in range(1, T + 1):
            for y in itertools.product(range(N), repeat=L):
                if any(y[i] == y[i + 1] for i in range(L - 1)):
                    continue
                tg = np.array([y], np.int64)
                fac = orc.aligned_forward(x, tg, tr, np.array([T]), np.array([L]))[0][0]
                a = target_scores_ref(tg, None, nxt, w, f, 0, 0.7, 0.2)[0]
                terms.append(fac + a - Z)
        assert abs(_lse(np.array(terms))) < 1e-10


def test_target_scores_merge_repeats_and_reject():
    nxt = np.array([[1, -1], [1, 0]])
    w = np.array([[0.5, 0.0], [0.25, 2.0]])
    f = np.array([-np.inf, 1.0])
    tg = np.array([[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 1, 1]], np.int64)
    got = target_scores_ref(tg, [4, 2, 3], nxt, w, f)
    # y0 = 0 0 1 0 -> 0 1 0: 0.5 + 2.0 + 0.5 ... state 0 after 1 from state 1: then 0 from state 0 -> 1, final 1.0
    assert got[0] == 0.5 + 2.0 + 0.5 + 1.0
    assert got[1] == -np.inf                                       # no arc for 1 from the start
    assert got[2] == -np.inf                                       # ends in the non-accepting state 0


# ---- C ABI -----------------------------------------------------------------------------------------------------------

NEW = ["asg_graph_full_work_bytes", "asg_graph_full_scratch_bytes", "asg_graph_full_forward", "asg_graph_full_backward",
       "asg_graph_target_scores"]


def test_abi_declares_and_exports_the_graph_loss_entry_points():
    from torch_asg_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asg_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(L, n), n
        assert n in _lib.SYMBOLS
    assert "asg_token_graph_loss" in src
    assert _lib.FLAG_GRAPH_LOSS_KEEP_ALPHA == 64 and _lib.FLAG_GRAPH_LOSS_STREAMING == 128 and _lib.FLAG_GRAPH_LOSS_RESIDENT == 256


def _fake(Q=11, E=20, N=5, S=3, dtype=0):
    """A problem and a graph whose pointers are non-null placeholders: only sizes and checks are exercised."""
    from torch_asg_amd import _lib
    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.S, p.dtype = 7, 3, N, 2, dtype
    p.inputs = p.transition = p.targets = 256
    g = _lib.AsgTokenGraph()
    g.Q, g.E, g.N, g.dtype = Q, E, N, dtype
    for n in ("label", "state", "row", "src", "src_label", "start_w", "final_w", "edge_w"):
        setattr(g, n, 256)
    gl = _lib.AsgTokenGraphLoss()
    gl.graph = ctypes.pointer(g)
    gl.S, gl.start = S, 0
    for n in ("tgt", "orow", "oedge", "lrow", "lq", "pkey", "pedge", "next", "arcw", "finw"):
        setattr(gl, n, 256)
    return p, g, gl


def test_abi_work_bytes_and_validation_without_gpu():
    from torch_asg_amd import _lib
    L = _lib.lib()
    p, g, gl = _fake()
    P, G = ctypes.byref(p), ctypes.byref(gl)
    assert L.asg_graph_full_work_bytes(P, G, 1) == 7 * 11 * 3 * 4
    assert L.asg_graph_full_work_bytes(P, G, 0) == 2 * 11 * 3 * 4
    assert L.asg_graph_full_scratch_bytes(P, G) == (2 * 11 * 3 * 4 + 255) // 256 * 256 + (11 + 20) * 3 * 4
    p.dtype = g.dtype = 1
    assert L.asg_graph_full_work_bytes(P, G, 1) == 7 * 11 * 3 * 8
    # short buffers: rejected before anything is launched
    need = L.asg_graph_full_work_bytes(P, G, 1)
    assert L.asg_graph_full_forward(None, P, G, 256, need - 1, 256, _lib.FLAG_GRAPH_LOSS_KEEP_ALPHA, None) == 3
    assert L.asg_graph_full_backward(None, P, G, 256, need - 1, 256, 256, 256, 256, 256, 1 << 30, 0, None) == 3
    assert L.asg_graph_full_backward(None, P, G, 256, need, 256, 256, 256, 256, 256, 16, 0, None) == 3
    # null outputs / graph
    assert L.asg_graph_full_forward(None, P, G, 256, need, None, 0, None) == 1
    assert L.asg_graph_full_forward(None, P, None, 256, need, 256, 0, None) == 1
    assert L.asg_graph_target_scores(None, P, G, None, None) == 1
    # a graph over the wrong N, a dtype mismatch
    g.N = 4
    assert L.asg_graph_full_forward(None, P, G, 256, need, 256, 0, None) == 1
    assert L.asg_graph_full_work_bytes(P, G, 1) == 0
    g.N, g.dtype = 5, 0
    assert L.asg_graph_full_forward(None, P, G, 256, need, 256, 0, None) == 1
    # limits: Q, E < 2^31, N <= 2^16
    p, g, gl = _fake()
    P, G = ctypes.byref(p), ctypes.byref(gl)
    g.Q = 1 << 31
    assert L.asg_graph_full_forward(None, P, G, 256, 1 << 40, 256, 0, None) == 2
    g.Q, g.E = 11, 1 << 31
    assert L.asg_graph_full_forward(None, P, G, 256, 1 << 40, 256, 0, None) == 2
    p, g, gl = _fake(N=(1 << 16) + 1)
    assert L.asg_graph_full_forward(None, ctypes.byref(p), ctypes.byref(gl), 256, 1 << 40, 256, 0, None) == 2
    # a bad start state, missing loss arrays
    p, g, gl = _fake()
    gl.start = 3
    assert L.asg_graph_full_forward(None, ctypes.byref(p), ctypes.byref(gl), 256, 1 << 40, 256, 0, None) == 1
    p, g, gl = _fake()
    gl.oedge = None
    assert L.asg_graph_full_backward(None, ctypes.byref(p), ctypes.byref(gl), 256, 1 << 40, 256, 256, 256, 256, 256, 1 << 40,
                                     0, None) == 1


def test_compile_loss_host_arrays():
    import torch_asg_amd
    rng = np.random.default_rng(1)
    nxt, w, f = _random_automaton(rng, 4, 3)
    g = torch_asg_amd.TokenGraph(nxt, w, f)
    h = g.compile_host(np.float64, 0.5, 0.25)
    lh = g.compile_loss_host(np.float64, 0.5, 0.25)
    Q, E = h["Q"], h["E"]
    tgt = lh["tgt"].astype(np.int64)
    assert (np.repeat(np.arange(Q), np.diff(h["row"])) == tgt).all()
    oe = lh["oedge"].astype(np.int64)
    assert sorted(oe.tolist()) == list(range(E))
    pairs = list(zip(h["src"][oe], tgt[oe]))
    assert pairs == sorted(pairs)
    assert (np.diff(lh["orow"]) == np.bincount(h["src"], minlength=Q)).all()
    assert (h["label"][lh["lq"]] == np.repeat(np.arange(3), np.diff(lh["lrow"]))).all()
    pk = h["label"][tgt] * 3 + h["src_label"]
    assert (lh["pkey"] == pk[lh["pedge"]]).all() and (np.diff(lh["pkey"]) >= 0).all()
    present = (nxt >= 0) & (w != -np.inf)
    assert ((lh["next"] >= 0) == present).all() and (lh["arcw"][~present] == -np.inf).all()
