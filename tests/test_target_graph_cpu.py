"""CPU tests of `torch_asg_amd.TargetGraphs` (torch_asg_amd/target_graph.py): the packed arrays of hand-written graphs, every
refusal, and the float64 reference (tests/target_graph_ref.py) against two facts it was not written from."""
import numpy as np
import pytest
import torch

from oracle import asg_oracle as orc
from target_graph_ref import target_graph_ref
from torch_asg_amd import TargetGraphs

NI = -np.inf


def test_chain_arrays():
    h = TargetGraphs.from_targets(torch.tensor([[2, 0, 1, 1]]), torch.tensor([3]), 3).compile_host(np.float64)
    want = dict(nk=[3], label=[[2, 0, 1]], row=[[0, 0, 1, 2]], src=[[0, 1]], tgt=[[1, 2]], orow=[[0, 1, 2, 2]], oedge=[[0, 1]],
                nlab=[3], lab=[[0, 1, 2]], lrow=[[0, 1, 2, 3]], lnode=[[1, 2, 0]], start_w=[[0, NI, NI]], final_w=[[NI, NI, 0]],
                edge_w=[[0, 0]], pkey=[0, 2, 3, 4, 8], pseg=[0, 1, 2, 3, 4, 5], pslot=[1, 3, 4, 2, 0])
    assert set(h) == set(want)
    for n, w in want.items():
        assert np.array_equal(h[n], np.array(w)), n
        assert h[n].dtype == (np.float64 if n.endswith("_w") else np.int64 if n == "pkey" else np.int32), n


def test_prefix_tree_and_cycle_arrays_padded_in_one_batch():
    tree = TargetGraphs.from_alternatives([[[0, 1, 2], [0, 3]]], 4, [[0.0, -0.5]]).graphs[0]
    assert [list(a) for a in tree] == [[0, 1, 2, 3], [0, NI, NI, NI], [NI, NI, 0, -0.5], [0, 1, 0], [1, 2, 3], [0, 0, 0]]
    g = TargetGraphs([tree[0], [0, 1]], [tree[1], [0, NI]], [tree[2], [NI, 0]],
                     [list(zip(*tree[3:])), [(0, 1, 0.5), (1, 0, -0.25)]], 4)
    assert (g.Kmax, g.Emax) == (4, 3)
    h = g.compile_host(np.float32)
    want = dict(nk=[4, 2], row=[[0, 0, 1, 2, 3], [0, 1, 2, 2, 2]], orow=[[0, 2, 3, 3, 3], [0, 1, 2, 2, 2]], nlab=[4, 2],
                pkey=[0, 1, 4, 5, 9, 10, 12, 15], pseg=[0, 2, 3, 5, 7, 8, 9, 10, 11], pslot=[0, 7, 11, 4, 12, 1, 8, 5, 2, 6, 3])
    for n, w in want.items():
        assert np.array_equal(h[n], np.array(w)), n
    for n, w in dict(src=[1, 0], tgt=[0, 1], oedge=[1, 0], edge_w=[-0.25, 0.5], lab=[0, 1], lnode=[0, 1]).items():
        assert np.array_equal(h[n][1, :2], np.array(w)), n          # the cycle, in front of its padding
    assert list(h["oedge"][0]) == [0, 2, 1] and h["edge_w"].dtype == np.float32


@pytest.mark.parametrize("make", [
    lambda: TargetGraphs([[0, 1]], [[0, NI]], [[NI, 0]], [[(0, 0, 0.0)]], 3),                   # self edge
    lambda: TargetGraphs([[1, 0, 1]], [[0, NI, NI]], [[NI, NI, 0]], [[(0, 2, 0.0)]], 3),        # edge between equal labels
    lambda: TargetGraphs([[0, 1]], [[np.inf, NI]], [[NI, 0]], [[(0, 1, 0.0)]], 3),              # +inf start
    lambda: TargetGraphs([[0, 1]], [[0, NI]], [[NI, np.nan]], [[(0, 1, 0.0)]], 3),              # NaN final
    lambda: TargetGraphs([[0, 1]], [[0, NI]], [[NI, 0]], [[(0, 1, np.inf)]], 3),                # +inf edge
    lambda: TargetGraphs([[0, 1] * 513], [[0.0] * 1026], [[0.0] * 1026], [[]], 3),              # more than 1024 nodes
    lambda: TargetGraphs.from_alternatives([[[0, 1], []]], 3),                                  # empty sequence
    lambda: TargetGraphs.from_alternatives([[[0, 1, 1]]], 3),                                   # equal consecutive labels
    lambda: TargetGraphs.from_alternatives([[[0, 1], [2], [0, 1]]], 3),                         # the same sequence twice
    lambda: TargetGraphs.from_targets(torch.tensor([[0, 0]]), None, 3),                         # a chain that repeats a label
])
def test_refusals(make):
    with pytest.raises(ValueError):
        make()


def test_reference_chain_is_the_force_aligned_score_and_tree_the_logsumexp_of_its_sequences():
    rng = np.random.default_rng(0)
    T, N = 9, 5
    seqs = [[0, 1, 2, 4], [0, 1, 3], [2, 4, 2, 1, 0], [3]]
    x = np.log(rng.dirichlet(np.ones(N), size=(T, len(seqs))))          # [T, 4, N]
    tr = 0.5 * rng.normal(size=(N, N))
    tg = np.zeros((len(seqs), 5), np.int64)
    for n, s in enumerate(seqs):
        tg[n, :len(s)] = s
    tl = np.array([len(s) for s in seqs])
    il, gs = np.array([9, 7, 9, 4]), np.array([1.0, -0.5, 2.0, 0.25])
    want, alpha, beta = orc.aligned_forward(x, tg, tr, il, tl)
    wtr, win = orc.aligned_backward(gs, alpha, beta, tg, tr, il, tl, N)
    got, gin, gtr = target_graph_ref(x, tr, TargetGraphs.from_targets(tg, tl, N).graphs, il, gs)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert np.allclose(gin, win, rtol=1e-10, atol=1e-12) and np.allclose(gtr, wtr, rtol=1e-10, atol=1e-12)
    # distinct label sequences have disjoint alignments: one utterance, every sequence an alternative
    xs = np.repeat(x[:, :1], len(seqs), axis=1)
    each = orc.aligned_forward(xs, tg, tr, np.full(len(seqs), T), tl)[0]
    w = np.array([0.0, -1.0, 0.5, -0.25])
    tree = target_graph_ref(xs[:, :1], tr, TargetGraphs.from_alternatives([seqs], N, [w]).graphs)[0]
    assert abs(tree[0] - np.logaddexp.reduce(each + w)) < 1e-12
