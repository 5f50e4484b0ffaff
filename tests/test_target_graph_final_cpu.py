"""CPU tests of the per-final-node scores of target graphs: the float64 reference (tests/target_graph_final_ref.py) against
facts it was not written from, the exported names, and the C entry points' refusals
(include/asg_hip.h::asg_target_graph_final_forward) -- no kernel is launched here."""
import ctypes

import numpy as np
import pytest

import torch_asg_amd as A
from oracle import asg_oracle as orc
from target_graph_final_ref import final_scores_ref, target_graph_final_ref
from target_graph_ref import target_graph_ref
from test_target_graph_viterbi_cpu import CYCLE, DIAMOND
from torch_asg_amd import TargetGraphs, _lib

NI = -np.inf
# two branches that meet again, a cycle back to the start, three finals
MESH = ([0, 1, 2, 1, 3], [0.3, NI, -0.1, NI, NI], [NI, 0.2, NI, -0.4, 0.0],
        [(0, 1, 0.1), (0, 2, -0.4), (1, 4, 0.0), (2, 3, 0.7), (3, 4, 0.2), (4, 0, -0.3), (2, 1, 0.05)])


def test_reference_sums_to_the_graph_score_and_rows_sum_to_g():
    rng = np.random.default_rng(0)
    T, N = 7, 5
    graphs = TargetGraphs(*[[s[n] for s in (MESH, DIAMOND, CYCLE)] for n in range(4)], N)
    x, tr = np.log(rng.dirichlet(np.ones(N), size=(T, 3))), 0.5 * rng.normal(size=(N, N))
    il, g = np.array([7, 2, 5]), rng.normal(size=(3, 5))
    fs, gin, gtr = target_graph_final_ref(x, tr, graphs.graphs, il, g)
    assert list(np.isfinite(fs[0])) == [False, True, False, True, True] and (fs[1] == NI).all()      # the diamond needs 3 frames
    Z = target_graph_ref(x, tr, graphs.graphs, il)[0]
    assert np.allclose(np.logaddexp.reduce(fs[[0, 2]], axis=1), Z[[0, 2]], rtol=1e-13, atol=1e-13) and Z[1] == NI
    for b in range(3):                        # every frame's weights sum to 1: a row holds the sum of g over the finite finals
        want = np.where(np.arange(T) < il[b], g[b][fs[b] > NI].sum(), 0.0) if (fs[b] > NI).any() else np.zeros(T)
        assert np.allclose(gin[:, b].sum(1), want, rtol=1e-12, atol=1e-12)


def test_reference_on_a_prefix_tree_is_the_force_aligned_score_of_each_sequence():
    rng = np.random.default_rng(1)
    T, N = 9, 5
    seqs, w = [[0, 1, 2, 4], [0, 1, 3], [2, 4, 2, 1, 0], [3], [0, 1]], np.array([0.0, -1.0, 0.5, -0.25, 0.125])
    x, tr = np.log(rng.dirichlet(np.ones(N), size=(T, 1))), 0.5 * rng.normal(size=(N, N))
    tg = np.zeros((len(seqs), 5), np.int64)
    for n, s in enumerate(seqs):
        tg[n, :len(s)] = s
    each = orc.aligned_forward(np.repeat(x, len(seqs), axis=1), tg, tr, np.full(len(seqs), T), np.array([len(s) for s in seqs]))[0]
    tree = TargetGraphs.from_alternatives([seqs], N, [w])
    fs = final_scores_ref(x, tr, tree.graphs)
    assert np.allclose(fs[0, tree.alternative_final[0]], each + w, rtol=1e-12, atol=1e-12)
    assert (fs[0, tree.final_alternative[0] < 0] == NI).all()


def test_exported_names_and_version():
    for name in ("TargetGraphFinalScores", "target_graph_final_scores", "target_graph_alternative_scores", "target_graph_risk"):
        assert name in A.__all__ and hasattr(A, name)
    for name in ("target_graph_final_scores", "target_graph_alternative_scores", "target_graph_risk"):
        assert hasattr(A.ASGLoss, name)
    for name in ("asg_target_graph_final_forward", "asg_target_graph_final_backward"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert _lib.lib().asg_hip_version() == _lib.ABI_VERSION == 230
    with pytest.raises(ValueError, match="from_alternatives"):
        A.target_graph_alternative_scores(None, None, TargetGraphs(*[[s[n] for s in (CYCLE,)] for n in range(4)], 3))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_c_entry_points_without_a_device(dt):
    L = _lib.lib()
    graphs = TargetGraphs(*[[s[n] for s in (DIAMOND, CYCLE)] for n in range(4)], 3)
    h = graphs.compile_host(dt)
    g = _lib.AsgTargetGraphs()
    g.B, g.Kmax, g.Emax, g.npairs, g.N = 2, graphs.Kmax, graphs.Emax, h["pkey"].size, 3
    g.dtype = _lib.ASG_DTYPE_F32 if dt == np.float32 else _lib.ASG_DTYPE_F64
    for n in _lib.TARGET_GRAPH_ARRAYS:
        setattr(g, n, h[n].ctypes.data)
    p, dummy = _lib.AsgProblem(), np.zeros(8, dt)
    p.inputs, p.transition = dummy.ctypes.data, dummy.ctypes.data
    p.T, p.B, p.N, p.S, p.dtype = 7, 2, 3, 1, g.dtype
    P, G, one = ctypes.byref(p), ctypes.byref(g), ctypes.c_void_p(1)
    need, sneed = L.asg_target_graph_work_bytes(P, G, 1), L.asg_target_graph_scratch_bytes(P, G)      # the score's own buffers
    assert need == 7 * 4 * 2 * np.dtype(dt).itemsize and sneed == 2 * 8 * np.dtype(dt).itemsize

    def fwd(nbytes=need, null=-1, tg=G, flags=_lib.FLAG_GRAPH_LOSS_KEEP_ALPHA):
        a = [None if i == null else one for i in range(2)]                  # work, final_scores
        return L.asg_target_graph_final_forward(None, P, tg, a[0], nbytes, a[1], flags, None)

    def bwd(nbytes=need, sbytes=sneed, null=-1, tg=G):
        a = [None if i == null else one for i in range(6)]      # work, scores, grad_scores, grad_inputs, grad_transition, scratch
        return L.asg_target_graph_final_backward(None, P, tg, a[0], nbytes, *a[1:], sbytes, 0, None)
    assert [fwd(null=i) for i in range(2)] == [1] * 2 and fwd(tg=None) == 1               # ASG_ERR_INVALID: a null pointer
    assert [bwd(null=i) for i in range(6)] == [1] * 6 and bwd(tg=None) == 1
    assert fwd(nbytes=need - 1) == 3 and bwd(nbytes=need - 1) == 3 and bwd(sbytes=sneed - 1) == 3      # ASG_ERR_WORKSPACE
    assert fwd(nbytes=0, null=1, flags=0) == 1                              # without the flag only the scores are needed, and are null
    p.B = 3
    assert fwd() == 1 and bwd() == 1                                        # p->B != tg->B
    p.B = 2
    g.Kmax = 1025
    assert fwd() == 2 and bwd() == 2                                        # ASG_ERR_UNSUPPORTED
    g.Kmax = graphs.Kmax
    g.Emax = L.asg_target_graph_max_edges(g.dtype, g.Kmax) + 1
    assert fwd() == 2 and bwd() == 2
