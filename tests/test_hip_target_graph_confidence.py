"""GPU tests (-m gpu) of the target-graph confidences (csrc/asg_target_graph_conf.hip) against the float64 numpy restatement
(tests/target_graph_conf_ref.py) under the device's own hypothesis; the best path and the normaliser bit for bit against
`target_graph_viterbi` and `target_graph_score`.  Tolerances: tests/test_hip_target_graph.py's for its posteriors (1e-9 in
float64, 1e-4 absolute in float32 for values <= 1), the absolute part times the frames of a window."""
import numpy as np
import pytest
import torch
import torch_asg_amd as A

from target_graph_conf_ref import target_graph_conf_ref
from test_hip_target_graph import DEV, DTYPES, NI, _batch, _case, _mixed, _skips

pytestmark = pytest.mark.gpu
both = pytest.mark.parametrize("dtype", DTYPES)


def _close(got, want, dtype, width, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).max()
    print("%s %s: max error %.3e" % (what, dtype, err))
    if dtype == torch.float64:
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * width), what
    else:
        assert err <= 1e-4 * max(width, np.abs(want).max()), what           # (NaN fails it)


def _check(x, tr, graphs, il, tol, what, got=None):
    """The device call (or `got`) against `target_graph_viterbi`, `target_graph_score` and the restatement -> the result."""
    xd, td, ild = x.to(DEV), tr.to(DEV), None if il is None else il.to(DEV)
    r = got or A.target_graph_confidence(xd, td, graphs, ild, tol)
    v = A.target_graph_viterbi(xd, td, graphs, ild)
    assert all(torch.equal(u, w) if w is not None else u is None for u, w in zip(r[:7], v)), what
    assert torch.equal(r.normalisers, A.target_graph_score(xd, td, graphs, ild)) and r.token_confidences.dtype == x.dtype, what
    Z, conf, post, _ = target_graph_conf_ref(x.double().numpy(), tr.double().numpy(), graphs.graphs,
                                             *(u.cpu().numpy() for u in r[3:6]), None if il is None else il.numpy(), tol)
    gc, gp, dead = r.token_confidences.cpu().numpy(), r.final_posteriors.cpu().numpy(), Z == NI
    assert list(r.normalisers.cpu().numpy() == NI) == list(dead) and not gc[dead].any() and not gp[dead].any(), what
    _close(gc, conf, x.dtype, 2 * tol + 1, what + " confidences")
    _close(gp, post, x.dtype, 1, what + " final posteriors")
    if tol == 0:                                      # a probability, and at least the best path's own
        eps, n = (1e-9 if x.dtype == torch.float64 else 1e-4), r.token_lengths.cpu().numpy()
        low = np.exp((r.scores - r.normalisers).double().cpu().numpy())
        assert all((gc[b, :n[b]] >= low[b] - eps).all() and (gc[b] <= 1 + eps).all() for b in np.flatnonzero(~dead)), what
    return r


@both
@pytest.mark.parametrize("tol", [0, 1])
def test_mixed_batch(tol, dtype):
    graphs, T, N, il = _mixed()
    r = _check(*_case(T, graphs.B, N, 1, dtype)[:2], graphs, il, tol, "mixed")
    assert (r.normalisers == NI).tolist() == [True, False, False, False, False, False, True, True, True, False]
    assert r.alternatives is None and r.alternative_posteriors is None


@both
@pytest.mark.parametrize("K", [64, 65, 256, 257, 1024])
def test_every_workgroup_width(K, dtype):
    graphs = _batch([_skips(K, 12, K), _skips(5, 12, 1)], 12)
    r = _check(*_case(3, 2, 12, K, dtype)[:2], graphs, torch.tensor([3, 2]), 1, "K=%d" % K)
    assert graphs.Kmax == K and torch.isfinite(r.normalisers).all()


@both
@pytest.mark.parametrize("tol", [0, 1, 64])
def test_the_window_at_its_edges_and_the_ring(tol, dtype):
    """Utterance 0: tokens at frames 0, 30 and len-1 = 69; tolerance 64 clips the middle window at both ends.  Utterance 1:
    "a b a" starting at frames 0, 1, 2.  The two a's lie two frames apart, so tolerance 1 has no window with both (the one
    over frames 0 .. 2 is b's): the count above 1 shows at tolerance 64.  Then a chain of 300 nodes that moves at every one of
    300 frames: more tokens than the ring's 256 slots.  (Peaked emissions are normalised again: small scores in float32.)"""
    T, N = 70, 4
    x, tr, _ = _case(T, 2, N, 7, dtype)
    x[:30, 0, 0] += 6; x[30:69, 0, 1] += 6; x[69:, 0, 2] += 6
    x[0, 1, 0] += 4; x[1, 1, 1] += 4; x[2:, 1, 0] += 4
    x = torch.log_softmax(x.double(), -1).to(dtype)
    r = _check(x, tr, A.TargetGraphs.from_alternatives([[[0, 1, 2]], [[0, 1, 0]]], N), None, tol, "tol=%d" % tol)
    assert r.token_frames[:, :3].tolist() == [[0, 30, 69], [0, 1, 2]] and r.token_lengths.tolist() == [3, 3]
    assert (r.token_confidences[1, 0].item() > 1.5) == (tol == 64)
    if tol != 1:
        T, N = 300, 12
        x, tr, _ = _case(T, 1, N, 4, dtype)
        x[torch.arange(T), 0, torch.arange(T) % N] += 6.0
        chain = ([k % N for k in range(T)], [0.0] + [NI] * (T - 1), [0.0] * T, [(k, k + 1, 0.0) for k in range(T - 1)])
        r = _check(torch.log_softmax(x.double(), -1).to(dtype), tr, _batch([chain], N), None, tol, "ring tol=%d" % tol)
        assert r.token_lengths.tolist() == [T]


@both
def test_a_tight_chain_is_certain(dtype):
    T, N = 9, 5
    r = _check(*_case(T, 1, N, 5, dtype)[:2], A.TargetGraphs.from_targets((torch.arange(T) % N)[None], None, N), None, 0, "tight")
    assert torch.equal(r.normalisers, r.scores) and r.alternatives.tolist() == [0]
    _close(r.token_confidences.cpu(), np.ones((1, T)), dtype, 1, "tight confidences")
    _close(r.final_posteriors.cpu(), np.eye(T)[-1:], dtype, 1, "tight final posterior")
    _close(r.alternative_posteriors.cpu(), np.ones((1, 1)), dtype, 1, "tight alternative")


@both
def test_alternative_posteriors_are_the_softmax_of_the_chains(dtype):
    T, B, N, S = 12, 3, 8, 5
    rng = np.random.default_rng(11)
    steps = rng.integers(1, N, (B, 4, S))
    steps[:, :, 0], steps[:, :, 1] = [0, 0, 1, 1], [1, 2, 1, 2]             # two pairs with a shared first label
    tg, tl, w = np.cumsum(steps, 2) % N, rng.integers(2, S + 1, (B, 4)), rng.normal(size=(B, 4))
    seqs = [[list(tg[b, j, :tl[b, j]]) for j in range(4 - (b == 2))] for b in range(B)]     # the last utterance has three
    x, tr, _ = _case(T, B, N, 12, dtype)
    il = torch.tensor([T, 9, T])
    r = _check(x, tr, A.TargetGraphs.from_alternatives(seqs, N, [list(w[b, :len(s)]) for b, s in enumerate(seqs)]), il, 0, "trees")
    each = torch.stack([A.target_graph_score(x.to(DEV), tr.to(DEV), A.TargetGraphs.from_alternatives([s[j:j + 1] for s in seqs], N),
                                             il.to(DEV)) for j in range(4)], 1).double().cpu() + torch.from_numpy(w)
    assert torch.isfinite(each).flatten().tolist() == [True] * 11 + [False] and r.alternative_posteriors[2, 3] == 0
    _close(r.alternative_posteriors.cpu(), torch.softmax(each, 1), dtype, 1, "alternative posteriors")
    _close(r.alternative_posteriors.sum(1).cpu(), np.ones(B), dtype, 1, "their sum")


@both
def test_edge_count_at_the_lds_bound(dtype):
    N, K = 8, 8
    bound = int(A._lib.lib().asg_target_graph_max_edges(int(dtype == torch.float64), K))
    rng = np.random.default_rng(5)
    src = rng.integers(0, K, bound)
    dst = (src + rng.integers(1, K, bound)) % K                              # parallel edges, never a self edge
    ed = [(int(s), int(d), float(w)) for s, d, w in zip(src, dst, rng.normal(size=bound) - 7.0)]
    lab, w = list(range(K)), list(rng.normal(size=K))
    graphs = _batch([(lab, w, w, ed), (lab[:2], w[:2], w[:2], [])], N)
    assert graphs.Emax == bound
    _check(*_case(3, 2, N, 6, dtype)[:2], graphs, None, 0, "at the bound")


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
        A.target_graph_confidence(xs, trd, graphs, ils, 1)    # warm
    torch.cuda.current_stream().wait_stream(s)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        rc = A.target_graph_confidence(xs, trd, graphs, ils, 1)
    for seed, il in ((3, [8, 5, 2]), (4, [3, 8, 8])):     # fresh emissions and lengths; [.., 2]: too short for its sequence
        x = _case(T, 3, N, seed, torch.float32)[0]
        xs.copy_(x)
        ils.copy_(torch.tensor(il))
        cg.replay()
        torch.cuda.synchronize()
        _check(x, trd.cpu(), graphs, torch.tensor(il), 1, "replay", rc)
        plain = A.target_graph_confidence(x.to(DEV), trd.contiguous(), graphs, ils, 1)       # [T,B,N] and row-major
        for eager in (plain, m.target_graph_confidence(xs, graphs, ils, 1), m.target_graph_confidence(xs, graphs, ils, 1)):
            assert all(torch.equal(u, w) for u, w in zip(rc, eager))
        assert (rc.normalisers[2] == NI).item() == (il[2] == 2)
