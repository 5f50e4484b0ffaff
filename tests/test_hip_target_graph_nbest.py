"""GPU tests (-m gpu) of the n best paths of a target graph (csrc/asg_target_graph_nbest.hip): every output bit for bit against
the numpy restatement in the same dtype (tests/target_graph_nbest_ref.py) -- adds and compares only, so no tolerance -- and
row 0 against `target_graph_viterbi` on the device."""
import numpy as np
import pytest
import torch
import torch_asg_amd as A

from target_graph_nbest_ref import FIELDS, target_graph_nbest_ref
from target_graph_viterbi_ref import tie_case
from test_hip_target_graph import DEV, DTYPES, NI, _batch, _case, _mixed, _skips

pytestmark = pytest.mark.gpu
both = pytest.mark.parametrize("dtype", DTYPES)


def _check(x, tr, graphs, il, nbest, what, got=None):
    """Every output of the device call (or `got`) against the restatement in the dtype of x, row 0 against the best path of the
    device -> (result, restatement)."""
    ild = None if il is None else il.to(DEV)
    r = got or A.target_graph_nbest(x.to(DEV), tr.to(DEV), graphs, ild, nbest, True)
    want = target_graph_nbest_ref(x.numpy(), tr.numpy(), graphs.graphs, None if il is None else il.numpy(), nbest)
    for name, w in zip(FIELDS, want):
        g = getattr(r, name)
        assert g.dtype == (x.dtype if "scores" in name else torch.int64) and np.array_equal(g.cpu().numpy(), w), "%s: %s" % (what, name)
    fa = graphs.final_alternative
    assert (r.alternatives is None) == (fa is None), what
    if fa is not None:
        assert np.array_equal(r.alternatives.cpu().numpy(), np.where(want[2] >= 0, np.take_along_axis(fa, np.maximum(want[2], 0), 1), -1))
    one = A.target_graph_viterbi(x.to(DEV), tr.to(DEV), graphs, ild)
    for name in ("scores", "nodes", "labels", "tokens", "token_frames", "token_lengths"):
        assert torch.equal(getattr(r, name)[:, 0], getattr(one, name)), "%s: row 0 %s" % (what, name)
    assert torch.equal(r.num_hyps > 0, one.scores > NI) and (one.alternatives is None or torch.equal(r.alternatives[:, 0], one.alternatives))
    return r, want


def _all_final(spec):
    lab, sw, fw, ed = spec
    return lab, sw, [0.0 if w == NI else w for w in fw], ed


@both
@pytest.mark.parametrize("nbest", [1, 3, 11])                                    # 11: Kmax + 5
def test_mixed_batch(nbest, dtype):
    graphs, T, N, il = _mixed()
    r, want = _check(*_case(T, graphs.B, N, 1, dtype)[:2], graphs, il, nbest, "mixed nbest=%d" % nbest)
    assert graphs.Kmax + 5 == 11 and list(want[0]) == [min(nbest, n) for n in [0, 1, 1, 3, 1, 2, 0, 0, 0, 1]]
    assert tuple(r.tokens.shape) == (graphs.B, nbest, T) and (want[1][:, 1:][want[0] <= 1] == NI).all()
    no = A.target_graph_nbest(*(v.to(DEV) for v in _case(T, graphs.B, N, 1, dtype)[:2]), graphs, il.to(DEV), nbest)
    assert no.nodes is None and no.labels is None and all(u is None or torch.equal(u, v) for u, v in zip(no, r))


@both
@pytest.mark.parametrize("K", [64, 65, 256, 257, 1024])
def test_full_tile_at_every_width_and_staging_edge(K, dtype):
    F = 64 if K <= 256 else 16                        # frames per staged block of that width
    il = torch.tensor([1, 2, F - 1, F, F + 1, 2 * F + 1])
    graphs = _batch([_all_final(_skips(K, 12, K + b)) for b in range(6)], 12)
    want = _check(*_case(2 * F + 1, 6, 12, K, dtype)[:2], graphs, il, K, "K=%d" % K)[1]
    assert graphs.Kmax == K and want[0][0] == K and (want[0] > 0).all()          # every node starts and ends: all K walkers


@both
@pytest.mark.parametrize("T", [12, 70])
def test_ties_come_in_ascending_node_order(T, dtype):
    x, tr, graphs = tie_case(T, 4)
    flat = A.TargetGraphs(*zip(*[(lab, sw, [0.0] * len(lab), list(zip(src, dst, ew))) for lab, sw, _, src, dst, ew in graphs.graphs]), 4)
    for gr, nbest in ((graphs, 4), (flat, 11)):                                  # the given finals; every node final
        want = _check(torch.from_numpy(x).to(dtype), torch.from_numpy(tr).to(dtype), gr, None, nbest, "ties T=%d" % T)[1]
        tied = want[1][0, :-1] == want[1][0, 1:]
        assert (gr is graphs and T == 70) or (tied.any() and (want[2][0, :-1] < want[2][0, 1:])[tied].all())


@both
def test_long_chain_across_the_64_frame_chunks(dtype):
    T, S = 260, 200
    x, tr, _ = _case(T, 2, 5, T, dtype)
    r, want = _check(x, tr, A.TargetGraphs.from_targets((torch.arange(S) % 5).repeat(2, 1), None, 5), torch.tensor([T, 230]), 2, "chain")
    assert list(want[0]) == [1, 1] and list(want[6][:, 0]) == [S, S] and np.isin([63, 64, 128, 192, 255, 256], want[5][0, 0]).sum() >= 2
    assert r.alternatives.tolist() == [[0, -1], [0, -1]]


@both
def test_trees_of_four_rank_as_four_aligner_calls(dtype):
    T, B, N, S = 24, 6, 8, 6
    rng = np.random.default_rng(11)
    steps = rng.integers(1, N, (B, 4, S))
    steps[:, :, 0] = np.arange(4)                                                # four distinct sequences per utterance
    tg, tl = np.cumsum(steps, 2) % N, rng.integers(3, S + 1, (B, 4))
    x, tr, _ = _case(T, B, N, 12, dtype)
    graphs = A.TargetGraphs.from_alternatives([[tg[b, j, :tl[b, j]] for j in range(4)] for b in range(B)], N)
    r = _check(x, tr, graphs, None, 4, "trees")[0]
    each = torch.stack([A.viterbi_align(x.to(DEV), torch.from_numpy(tg[:, j]).to(DEV), tr.to(DEV), None,
                                        torch.from_numpy(tl[:, j]).to(DEV))[0] for j in range(4)], 1)
    top = each.sort(1, descending=True)
    assert (top.values[:, :-1] > top.values[:, 1:]).all() and r.num_hyps.tolist() == [4] * B
    assert torch.equal(r.scores, top.values) and torch.equal(r.alternatives, top.indices)


def test_strides_and_two_replays_of_a_captured_call():
    N, T = 6, 8
    graphs = A.TargetGraphs.from_alternatives([[[0, 1, 2], [0, 3]], [[4, 1], [2]], [[5, 0, 3, 1]]], N)
    xs = torch.empty(3, T, N, device=DEV).transpose(0, 1)                            # batch-major emissions
    trd, ils = _case(T, 3, N, 0, torch.float32)[1].to(DEV).t(), torch.zeros(3, dtype=torch.int64, device=DEV)
    m = A.ASGLoss(N).to(DEV)
    m.transition.data.copy_(trd)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.target_graph_nbest(xs, trd, graphs, ils, 3, True)   # warm
    torch.cuda.current_stream().wait_stream(s)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        rc = A.target_graph_nbest(xs, trd, graphs, ils, 3, True)
    for seed, il in ((3, [8, 5, 2]), (4, [3, 8, 8])):     # fresh emissions and lengths; [.., 2]: too short for its sequence
        x = _case(T, 3, N, seed, torch.float32)[0]
        xs.copy_(x)
        ils.copy_(torch.tensor(il))
        cg.replay()
        torch.cuda.synchronize()
        want = _check(x, trd.cpu(), graphs, torch.tensor(il), 3, "replay", rc)[1]
        eager = m.target_graph_nbest(xs, graphs, ils, 3, True)
        assert all(torch.equal(u, v) for u, v in zip(rc, eager)) and (want[0][2] == 0) == (il[2] == 2)


def test_refusals():
    graphs, T, N, il = _mixed()
    x, tr, _ = _case(T, graphs.B, N, 1, torch.float32)
    with pytest.raises(ValueError, match="nbest"):
        A.target_graph_nbest(x.to(DEV), tr.to(DEV), graphs, il.to(DEV), 0)
    with pytest.raises(RuntimeError, match="asg_target_graph_nbest"):
        A.target_graph_nbest(x.to(DEV), tr.to(DEV), graphs, il.to(DEV), 1025)
    assert A.target_graph_nbest(x.to(DEV).half(), tr.to(DEV), graphs, il.to(DEV), 2).scores.dtype == torch.float32      # widened
