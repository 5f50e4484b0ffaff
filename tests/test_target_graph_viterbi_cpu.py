"""CPU tests of the best path of a target graph: the numpy restatement (tests/target_graph_viterbi_ref.py) against exhaustive
enumeration and the oracle's chain Viterbi, the tie rule, `final_alternative`, and the C entry points' refusals."""
import ctypes
import itertools

import numpy as np
import pytest

from oracle import asg_oracle as orc
from target_graph_viterbi_ref import NI, target_graph_viterbi_ref, tie_case
from torch_asg_amd import TargetGraphs, _lib

DIAMOND = ([0, 1, 1, 2], [0.3, NI, NI, NI], [NI, NI, NI, -0.2], [(0, 1, 0.1), (0, 2, -0.4), (1, 3, 0.0), (2, 3, 0.7)])
CYCLE = ([0, 1], [0.0, NI], [0.1, -0.3], [(0, 1, 0.5), (1, 0, -0.25)])


def _enumerate(I, tr, graph, T):
    """Every (path, alignment) as a node sequence, best first: (score, nodes) pairs."""
    lab, sw, fw, src, dst, ew = graph
    edge = {(s, d): w for s, d, w in zip(src, dst, ew)}
    found = []
    for seq in itertools.product(range(len(lab)), repeat=T):
        sc = sw[seq[0]] + I[0, lab[seq[0]]] + fw[seq[-1]]
        for a, k, t in zip(seq, seq[1:], range(1, T)):
            sc += (tr[lab[k], lab[k]] if a == k else tr[lab[k], lab[a]] + edge.get((a, k), NI)) + I[t, lab[k]]
        found.append((sc, seq))
    return sorted(found, reverse=True)


@pytest.mark.parametrize("T", [1, 3, 5])
def test_restatement_against_exhaustive_enumeration(T):
    rng = np.random.default_rng(T)
    tree = TargetGraphs.from_alternatives([[[0, 1, 2], [0, 3], [4]]], 5, [[0.0, -0.5, 0.25]]).graphs[0]
    specs = [(tree[0], tree[1], tree[2], list(zip(*tree[3:]))), DIAMOND, CYCLE]
    graphs = TargetGraphs(*[[s[n] for s in specs] for n in range(4)], 5)
    x, tr = rng.normal(size=(T, 3, 5)), 0.5 * rng.normal(size=(5, 5))
    scores, nodes, labels, tokens, frames, lengths = target_graph_viterbi_ref(x, tr, graphs.graphs)
    for b, g in enumerate(graphs.graphs):
        (best, seq), second = _enumerate(x[:, b], tr, g, T)[:2]
        if best == NI:                                                      # (the diamond needs three frames)
            assert scores[b] == NI and lengths[b] == 0 and (np.stack([nodes[b], labels[b], tokens[b], frames[b]]) == -1).all()
            continue
        assert best - second[0] > 1e-9 and abs(scores[b] - best) < 1e-12, b
        at = [t for t in range(T) if t == 0 or seq[t] != seq[t - 1]]
        assert list(nodes[b]) == list(seq) and list(labels[b]) == [g[0][k] for k in seq] and lengths[b] == len(at)
        assert list(frames[b]) == at + [-1] * (T - len(at)) and list(tokens[b]) == [g[0][seq[t]] for t in at] + [-1] * (T - len(at))


def test_restatement_equals_the_oracle_viterbi_on_chains():
    rng = np.random.default_rng(3)
    tg = np.array([[1, 2, 3, 1, 0], [4, 5, 4, 0, 0], [0, 5, 2, 0, 0], [3, 1, 3, 1, 3]])
    tl, il = np.array([5, 3, 3, 5]), np.array([11, 8, 2, 6])              # utterance 2: its targets do not fit its frames
    x, tr = rng.normal(size=(11, 4, 6)), rng.normal(size=(6, 6))
    graphs = TargetGraphs.from_targets(tg, tl, 6)
    scores, nodes, labels, _, _, lengths = target_graph_viterbi_ref(x, tr, graphs.graphs, il)
    want, pos = orc.viterbi(x, tg, tr, il, tl)
    assert scores[2] == NI and want[2] == NI and lengths[2] == 0
    assert np.allclose(np.delete(scores, 2), np.delete(want, 2), rtol=1e-12, atol=1e-12) and np.array_equal(nodes, pos)
    assert np.array_equal(labels, np.where(pos >= 0, np.take_along_axis(tg, np.maximum(pos, 0), 1), -1))
    assert np.array_equal(graphs.final_alternative, np.array([[-1, -1, -1, -1, 0], [-1, -1, 0, -1, -1]])[[0, 1, 1, 0]])


def test_the_tie_rule_bites_and_final_alternative_names_the_sequences():
    x, tr, graphs = tie_case(70, 1)
    strict = target_graph_viterbi_ref(x, tr, graphs.graphs)
    loose = target_graph_viterbi_ref(x, tr, graphs.graphs, edges_win_ties=True)
    assert np.array_equal(strict[0], loose[0])                              # the same maximum ...
    assert all(not np.array_equal(strict[1][b], loose[1][b]) for b in range(2))          # ... along another path
    tree = TargetGraphs.from_alternatives([[[0, 1, 2], [0, 3], [4, 1], [0]], [[2, 1]]], 5)
    assert np.array_equal(tree.final_alternative, np.array([[3, -1, 0, 1, -1, 2], [-1, 0, -1, -1, -1, -1]]))
    assert TargetGraphs([[0]], [[0.0]], [[0.0]], [[]], 2).final_alternative is None


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
    need = L.asg_target_graph_viterbi_work_bytes(P, G)
    assert need == 2 * 7 * 4 * 2                                            # B * T * Kmax * 2

    def call(nbytes=need, null=-1, tg=G):
        a = [None if i == null else one for i in range(7)]                  # work, scores and the five integer outputs
        return L.asg_target_graph_viterbi(None, P, tg, a[0], nbytes, *a[1:], 0, None)
    assert [call(null=i) for i in range(7)] == [1] * 7 and call(tg=None) == 1            # ASG_ERR_INVALID: a null pointer
    assert call(nbytes=need - 1) == 3                                       # ASG_ERR_WORKSPACE: one byte short
    p.B = 3
    assert call() == 1                                                      # p->B != tg->B
    p.B = 2
    g.Emax = L.asg_target_graph_max_edges(g.dtype, g.Kmax) + 1
    assert call() == 2 and L.asg_target_graph_viterbi_work_bytes(P, G) == 0          # ASG_ERR_UNSUPPORTED
