"""CPU tests of the n best paths of a target graph: the numpy restatement (tests/target_graph_nbest_ref.py) against exhaustive
enumeration grouped by end node, the best path's restatement and the oracle's chain Viterbi; the C entry points' refusals."""
import ctypes

import numpy as np
import pytest

import torch_asg_amd as A
from oracle import asg_oracle as orc
from target_graph_nbest_ref import target_graph_nbest_ref
from target_graph_viterbi_ref import NI, target_graph_viterbi_ref, tie_case
from test_target_graph_viterbi_cpu import CYCLE, DIAMOND, _enumerate
from torch_asg_amd import TargetGraphs, _lib


@pytest.mark.parametrize("T", [1, 3, 5])
@pytest.mark.parametrize("nbest", [1, 2, 7])
def test_restatement_against_exhaustive_enumeration(T, nbest):
    rng = np.random.default_rng(T)
    tree = TargetGraphs.from_alternatives([[[0, 1, 2], [0, 3], [4]]], 5, [[0.0, -0.5, 0.25]]).graphs[0]
    specs = [(tree[0], tree[1], tree[2], list(zip(*tree[3:]))), DIAMOND, CYCLE]
    graphs = TargetGraphs(*[[s[n] for s in specs] for n in range(4)], 5)
    x, tr = rng.normal(size=(T, 3, 5)), 0.5 * rng.normal(size=(5, 5))
    num, scores, ends, emis, tokens, frames, lengths, nodes, labels = target_graph_nbest_ref(x, tr, graphs.graphs, None, nbest)
    best = target_graph_viterbi_ref(x, tr, graphs.graphs)
    for got, want in zip((scores, nodes, labels, tokens, frames, lengths), best):
        assert np.array_equal(got[:, 0], want)                                   # row 0 is the best path, bit for bit
    for b, g in enumerate(graphs.graphs):
        per_end = {}
        for sc, seq in _enumerate(x[:, b], tr, g, T):                            # best first: the first per end node is its best
            if sc > NI and seq[-1] not in per_end:
                per_end[seq[-1]] = (sc, seq)
        want = sorted(per_end.items(), key=lambda kv: (-kv[1][0], kv[0]))[:nbest]
        assert num[b] == len(want) and (b != 0 or T < 3 or len(per_end) == 3)
        for r, (k, (sc, seq)) in enumerate(want):
            at = [t for t in range(T) if t == 0 or seq[t] != seq[t - 1]]
            lab = [g[0][n] for n in seq]
            ac = sum(x[t, b, lab[t]] for t in range(T)) + sum(tr[lab[t], lab[t - 1]] for t in range(1, T))
            assert ends[b, r] == k and abs(scores[b, r] - sc) < 1e-12 and abs(emis[b, r] - ac) < 1e-12
            assert list(nodes[b, r]) == list(seq) and list(labels[b, r]) == lab and lengths[b, r] == len(at)
            assert list(frames[b, r]) == at + [-1] * (T - len(at)) and list(tokens[b, r]) == [lab[t] for t in at] + [-1] * (T - len(at))
        pad = slice(len(want), None)
        assert (scores[b, pad] == NI).all() and (emis[b, pad] == NI).all() and (lengths[b, pad] == 0).all()
        assert all((a[b, pad] == -1).all() for a in (ends, tokens, frames, nodes, labels))


def test_ties_rank_by_node_and_trees_rank_their_alternatives_by_the_oracle_viterbi():
    x, tr, graphs = tie_case(12, 4)                                              # (few frames: a small range of integer scores)
    num, scores, ends = target_graph_nbest_ref(x, tr, graphs.graphs, None, 8)[:3]
    assert any(scores[0, r] == scores[0, r + 1] and ends[0, r] < ends[0, r + 1] for r in range(num[0] - 1))      # a real tie
    rng = np.random.default_rng(3)
    tg = np.array([[[1, 2, 3, 1], [1, 2, 0, 0], [4, 5, 4, 0]], [[0, 5, 2, 0], [3, 1, 3, 1], [3, 1, 0, 0]]])
    tl, il = np.array([[4, 2, 3], [3, 4, 2]]), np.array([9, 3])                  # utterance 1: too short for its second sequence
    x, tr = rng.normal(size=(9, 2, 6)), rng.normal(size=(6, 6))
    trees = TargetGraphs.from_alternatives([[tg[b, j, :tl[b, j]] for j in range(3)] for b in range(2)], 6)
    num, scores, ends = target_graph_nbest_ref(x, tr, trees.graphs, il, 3)[:3]
    each = np.stack([orc.viterbi(x, tg[:, j], tr, il, tl[:, j])[0] for j in range(3)], 1)           # [B, alternative]
    assert list(num) == [3, 2] and each[1, 1] == NI
    for b in range(2):
        alt = trees.final_alternative[b][ends[b, :num[b]]]
        assert list(alt) == list(np.argsort(-each[b], kind="stable")[:num[b]])
        assert np.allclose(scores[b, :num[b]], each[b, alt], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_c_entry_points_and_names_without_a_device(dt):
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
    size = lambda nb: L.asg_target_graph_nbest_work_bytes(P, G, nb)
    assert size(3) == 2 * 7 * 4 * 2 + 96 and size(1) == 112 + 32 and size(4) == size(1024) == 112 + 112       # rows = min(nbest, Kmax)
    assert size(0) == 0 and size(1025) == 0

    def call(nbest=3, null=(), nbytes=size(3)):
        a = [None if i in null else one for i in range(10)]                 # work, the seven outputs, nodes and labels
        return L.asg_target_graph_nbest(None, P, G, nbest, a[0], nbytes, *a[1:], 0, None)
    assert [call(null=(i,)) for i in range(10)] == [1] * 10                 # ASG_ERR_INVALID: a null pointer (one of nodes / labels too)
    assert call(nbytes=size(3) - 1) == 3 and call(4, nbytes=size(3)) == 3   # ASG_ERR_WORKSPACE
    assert call(0) == 1 and call(-5, null=range(10)) == 1                   # nbest < 1: ASG_ERR_INVALID, before the pointers
    assert call(1025, null=range(10)) == 2                                  # nbest > 1024: ASG_ERR_UNSUPPORTED, before the pointers
    g.Emax = L.asg_target_graph_max_edges(g.dtype, g.Kmax) + 1
    assert call(0) == 2                                                     # ... and behind the graphs
    for name in ("target_graph_nbest", "TargetGraphNBest"):
        assert name in A.__all__ and hasattr(A, name)
    assert hasattr(A.ASGLoss, "target_graph_nbest") and {"asg_target_graph_nbest_work_bytes", "asg_target_graph_nbest"} <= set(_lib.SYMBOLS)
    assert A.TargetGraphNBest._fields == ("num_hyps", "scores", "end_nodes", "emission_scores", "tokens", "token_frames",
                                          "token_lengths", "alternatives", "nodes", "labels")
