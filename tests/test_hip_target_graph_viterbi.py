"""GPU tests (-m gpu) of the best path of a target graph (csrc/asg_target_graph_viterbi.hip): every output bit for bit against
the numpy restatement in the same dtype (tests/target_graph_viterbi_ref.py) -- adds and compares only, so no tolerance."""
import numpy as np
import pytest
import torch
import torch_asg_amd as A

from target_graph_viterbi_ref import target_graph_viterbi_ref, tie_case
from test_hip_target_graph import DEV, DTYPES, NI, _batch, _case, _mixed, _skips
from util import assert_close

pytestmark = pytest.mark.gpu
both = pytest.mark.parametrize("dtype", DTYPES)


def _check(x, tr, graphs, il, what, got=None):
    """The six outputs of the device call (or `got`) against the restatement in the dtype of x -> (result, restatement)."""
    r = got or A.target_graph_viterbi(x.to(DEV), tr.to(DEV), graphs, None if il is None else il.to(DEV))
    iln = None if il is None else il.numpy()
    want = target_graph_viterbi_ref(x.numpy(), tr.numpy(), graphs.graphs, iln)
    for n, (g, w) in enumerate(zip(r, want)):
        assert g.dtype == (torch.int64 if n else x.dtype) and np.array_equal(g.cpu().numpy(), w), "%s: %s" % (what, r._fields[n])
    if x.dtype == torch.float32:
        fin = np.isfinite(want[0])
        assert_close(want[0][fin], target_graph_viterbi_ref(x.double().numpy(), tr.double().numpy(), graphs.graphs, iln)[0][fin], what=what)
    return r, want


@both
def test_mixed_batch(dtype):
    graphs, T, N, il = _mixed()
    r, want = _check(*_case(T, graphs.B, N, 1, dtype)[:2], graphs, il, "mixed")
    dead = np.array([True, False, False, False, False, False, True, True, True, False])
    assert list(want[0] == NI) == list(dead) and r.alternatives is None and list(want[5] == 0) == list(dead)
    assert all((w[dead] == -1).all() and (w[~dead, 0] >= 0).all() for w in want[1:5])


@both
@pytest.mark.parametrize("K", [64, 65, 256, 257, 1024])
def test_widths_and_staging_blocks(K, dtype):
    F = 64 if K <= 256 else 16                        # frames per staged block of that width
    il = torch.tensor([1, 2, F - 1, F, F + 1, 2 * F - 1, 2 * F, 2 * F + 1])
    graphs = _batch([_skips(K, 12, K + b) for b in range(8)], 12)
    want = _check(*_case(2 * F + 1, 8, 12, K, dtype)[:2], graphs, il, "K=%d" % K)[1]
    assert graphs.Kmax == K and np.isfinite(want[0]).all()


@both
@pytest.mark.parametrize("S,T", [(3, 64), (3, 65), (3, 130), (200, 260)])
def test_compaction_chunks(S, T, dtype):
    """Chains whose tokens start on both sides of the chunk edges (64 / 256 frames) and of the wavefront edges of the scan."""
    cuts = [(1, 2), (T - 2, T - 1), (min(63, T - 2), min(64, T - 1)), (T // 2, T - 1)]
    x, tr, _ = _case(T, 4, 5, T, dtype)
    for b, (c1, c2) in enumerate(cuts if S == 3 else []):        # peaks that put the two moves of utterance b at cuts[b]
        x[:c1, b, 0] += 9; x[c1:c2, b, 1] += 9; x[c2:, b, 2] += 9
    want = _check(x, tr, A.TargetGraphs.from_targets((torch.arange(S) % 5).repeat(4, 1), None, 5), None, "S=%d T=%d" % (S, T))[1]
    assert (want[5] == S).all() and (S != 3 or [list(f[:3]) for f in want[4]] == [[0, a, c] for a, c in cuts])
    assert S == 3 or np.isin([63, 64, 128, 192, 255, 256], want[4][0]).sum() >= 2


@both
@pytest.mark.parametrize("T,K", [(70, 11), (140, 300)])
def test_ties(T, K, dtype):
    rng = np.random.default_rng(T)
    walk = lambda n, first: tuple(int(v) for v in np.cumsum(np.r_[first, rng.integers(1, 4, n - 1)]) % 4)
    head = walk(42, 0)                                # K = 300: a shared head of 42 labels, itself an alternative, and three tails of 86
    x, tr, graphs = tie_case(T, 1, *([tuple(head + walk(86, head[-1] + 1 + j) for j in range(3)) + (head,)] if K == 300 else []))
    want = _check(torch.from_numpy(x).to(dtype), torch.from_numpy(tr).to(dtype), graphs, None, "ties T=%d" % T)[1]
    assert graphs.Kmax == K and np.isfinite(want[0]).all()


@both
@pytest.mark.parametrize("S", [30, 65])
def test_chains_equal_viterbi_align(S, dtype):
    T, B, N = 70, 4, 7
    tg = torch.from_numpy(np.cumsum(np.random.default_rng(S).integers(1, N, (B, S)), 1) % N)     # neighbouring labels distinct
    tl, il = torch.tensor([S, S - 3, S, S // 2]), torch.tensor([T, 66, S - 1, T])    # utterance 2: shorter than its targets
    x, tr, _ = _case(T, B, N, S, dtype)
    r, want = _check(x, tr, A.TargetGraphs.from_targets(tg, tl, N), il, "chains S=%d" % S)
    scores, pos, labels = A.viterbi_align(x.to(DEV), tg.to(DEV), tr.to(DEV), il.to(DEV), tl.to(DEV))
    assert list(want[0] == NI) == [False, False, True, False] and (want[1][2] == -1).all()
    assert torch.equal(r.scores, scores) and torch.equal(r.nodes, pos) and torch.equal(r.labels, labels)
    assert r.alternatives.tolist() == [0, 0, -1, 0]


@both
def test_alternatives_name_the_spoken_sequence(dtype):
    T, B, N, S = 24, 6, 8, 6
    rng = np.random.default_rng(11)
    steps = rng.integers(1, N, (B, 4, S))
    steps[:, :, 0] = np.arange(4)                                                    # four distinct sequences per utterance
    tg, tl, spoken = np.cumsum(steps, 2) % N, rng.integers(3, S + 1, (B, 4)), rng.integers(0, 4, B)
    x, tr, _ = _case(T, B, N, 12, dtype)
    for b, j in enumerate(spoken):                    # a peak along a random alignment of sequence j
        seg = np.sort(rng.choice(np.arange(1, T), tl[b, j] - 1, replace=False))
        x[torch.arange(T), b, torch.from_numpy(tg[b, j][np.searchsorted(seg, np.arange(T), side="right")])] += 6.0
    graphs = A.TargetGraphs.from_alternatives([[tg[b, j, :tl[b, j]] for j in range(4)] for b in range(B)], N)
    r = _check(x, tr, graphs, None, "alternatives")[0]
    each = torch.stack([A.viterbi_align(x.to(DEV), torch.from_numpy(tg[:, j]).to(DEV), tr.to(DEV), None,
                                        torch.from_numpy(tl[:, j]).to(DEV))[0] for j in range(4)])
    top = each.sort(0, descending=True).values
    assert (top[0] > top[1]).all()                                                   # the best of the four is unique
    assert r.alternatives.tolist() == list(spoken) == each.argmax(0).tolist() and torch.equal(r.scores, top[0])


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
        A.target_graph_viterbi(xs, trd, graphs, ils)      # warm
    torch.cuda.current_stream().wait_stream(s)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        rc = A.target_graph_viterbi(xs, trd, graphs, ils)
    for seed, il in ((3, [8, 5, 2]), (4, [3, 8, 8])):     # fresh emissions and lengths; [.., 2]: too short for its sequence
        x = _case(T, 3, N, seed, torch.float32)[0]
        xs.copy_(x)
        ils.copy_(torch.tensor(il))
        cg.replay()
        torch.cuda.synchronize()
        want = _check(x, trd.cpu(), graphs, torch.tensor(il), "replay", rc)[1]
        eager = m.target_graph_viterbi(xs, graphs, ils)
        assert all(torch.equal(u, v) for u, v in zip(rc, eager)) and (want[0][2] == NI) == (il[2] == 2)
