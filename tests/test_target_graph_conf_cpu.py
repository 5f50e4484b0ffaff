"""CPU tests of the target-graph confidences: the numpy restatement (tests/target_graph_conf_ref.py) against exhaustive
enumeration and the oracle's force-aligned scores, the C entry points' sizes and refusals, the exported names."""
import ctypes
import itertools

import numpy as np
import pytest

import torch_asg_amd
from oracle import asg_oracle as orc
from target_graph_conf_ref import target_graph_conf_ref
from target_graph_viterbi_ref import NI, target_graph_viterbi_ref
from torch_asg_amd import TargetGraphs, _lib

SEQS, WEIGHTS = [[0, 1, 2], [0, 3], [4]], [0.0, -0.5, 0.25]
DIAMOND = ([0, 1, 1, 2], [0.3, NI, NI, NI], [NI, NI, NI, -0.2], [(0, 1, 0.1), (0, 2, -0.4), (1, 3, 0.0), (2, 3, 0.7)])
CYCLE = ([0, 1], [0.0, NI], [0.1, -0.3], [(0, 1, 0.5), (1, 0, -0.25)])


def _enumerate(I, tr, graph, T, N):
    """Z, P [N,T] and the final posteriors [K], each summed directly over every node sequence of T frames."""
    lab, sw, fw, src, dst, ew = graph
    edge = {(s, d): w for s, d, w in zip(src, dst, ew)}
    seqs = list(itertools.product(range(len(lab)), repeat=T))
    sc = []
    for seq in seqs:
        sc.append(sw[seq[0]] + I[0, lab[seq[0]]] + fw[seq[-1]])
        for a, k, t in zip(seq, seq[1:], range(1, T)):
            sc[-1] += (tr[lab[k], lab[k]] if a == k else tr[lab[k], lab[a]] + edge.get((a, k), NI)) + I[t, lab[k]]
    Z = np.logaddexp.reduce(sc)
    P, post = np.zeros((N, T)), np.zeros(len(lab))
    for seq, w in zip(seqs, np.exp(np.array(sc) - Z) if Z > NI else []):
        post[seq[-1]] += w
        for t in range(T):
            if t == 0 or seq[t] != seq[t - 1]:
                P[lab[seq[t]], t] += w
    return Z, P, post


@pytest.mark.parametrize("tol", [0, 1, 5])
@pytest.mark.parametrize("T", [1, 3, 5])
def test_restatement_against_exhaustive_enumeration(T, tol):
    rng = np.random.default_rng(T)
    trees = TargetGraphs.from_alternatives([SEQS], 5, [WEIGHTS])
    tree = trees.graphs[0]
    graphs = TargetGraphs(*[[s[n] for s in ((tree[0], tree[1], tree[2], list(zip(*tree[3:]))), DIAMOND, CYCLE)] for n in range(4)], 5)
    x, tr = rng.normal(size=(T, 3, 5)), 0.5 * rng.normal(size=(5, 5))
    _, _, _, tokens, frames, lengths = target_graph_viterbi_ref(x, tr, graphs.graphs)
    Z, conf, post, P = target_graph_conf_ref(x, tr, graphs.graphs, tokens, frames, lengths, tol=tol)
    for b, g in enumerate(graphs.graphs):
        Ze, Pe, pe = _enumerate(x[:, b], tr, g, T, 5)
        if Ze == NI:                                                        # (the diamond needs three frames)
            assert Z[b] == NI and lengths[b] == 0 and not conf[b].any() and not post[b].any()
            continue
        want = [Pe[tokens[b][j], max(frames[b][j] - tol, 0):frames[b][j] + tol + 1].sum() for j in range(lengths[b])]
        assert abs(Z[b] - Ze) < 1e-12 and np.allclose(P[b], Pe, rtol=1e-12, atol=1e-12), b
        assert np.allclose(post[b, :len(pe)], pe, rtol=1e-12, atol=1e-12) and abs(pe.sum() - 1) < 1e-12, b
        assert np.allclose(conf[b, :lengths[b]], want, rtol=1e-12, atol=1e-12) and not conf[b, lengths[b]:].any(), b
        if tol == 0:
            assert (np.array(want) <= 1 + 1e-12).all()
    # the alternatives' posteriors: the softmax of the sequences' force-aligned scores plus their weights
    tg = np.array([s + [0] * (3 - len(s)) for s in SEQS])
    fac = orc.aligned_forward(np.repeat(x[:, :1], 3, 1), tg, tr, None, np.array([len(s) for s in SEQS]))[0] + WEIGHTS
    fac[np.array([len(s) for s in SEQS]) > T] = NI
    assert np.allclose(post[0][trees.alternative_final[0]], np.exp(fac - np.logaddexp.reduce(fac)), rtol=1e-10, atol=1e-12)


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
    need = L.asg_target_graph_confidence_work_bytes(P, G)
    assert need == 2 * 7 * 4 * np.dtype(dt).itemsize + 2 * 7 * 4 * 2       # alpha (a multiple of 16 here) + the back-pointers

    def call(nbytes=need, null=-1, tg=G, tol=0):
        a = [None if i == null else one for i in range(10)]                 # work and the nine outputs
        return L.asg_target_graph_confidence(None, P, tg, tol, a[0], nbytes, *a[1:], 0, None)
    assert [call(null=i) for i in range(10)] == [1] * 10 and call(tg=None) == 1          # ASG_ERR_INVALID: a null pointer
    assert call(nbytes=need - 1) == 3                                       # ASG_ERR_WORKSPACE: one byte short
    assert call(tol=-1) == 1 and call(tol=65) == 2                          # ASG_ERR_INVALID / ASG_ERR_UNSUPPORTED
    p.B = 3
    assert call() == 1                                                      # p->B != tg->B
    p.B = 2
    g.Emax = L.asg_target_graph_max_edges(g.dtype, g.Kmax) + 1
    assert call() == 2 and L.asg_target_graph_confidence_work_bytes(P, G) == 0           # ASG_ERR_UNSUPPORTED


def test_names_and_version():
    assert {"TargetGraphConfidence", "target_graph_confidence"} <= set(torch_asg_amd.__all__)
    assert torch_asg_amd.TargetGraphConfidence._fields[:7] == torch_asg_amd.TargetGraphAlignment._fields
    assert _lib.lib().asg_hip_version() == 230 == _lib.ABI_VERSION
