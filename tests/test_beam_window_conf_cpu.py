"""CPU tests of the lattice-keeping window stream's definition (include/asg_hip.h::asg_beam_conf_window_advance): the restatement
tests/beam_window_conf_ref.py against the growing stream's restatement (tests/beam_stream_conf_ref.py, byte for byte), the one-shot
restatement (tests/beam_conf_ref.py), an enumeration of all label paths, and the regimes by name -- no kernel is launched here."""
import itertools

import numpy as np
import pytest

from beam_conf_ref import beam_conf_ref
from beam_stream_conf_ref import BeamStreamConfRef
from beam_window_conf_ref import BeamWindowConfRef
from beam_window_ref import two_component_emissions, two_components_automaton
from graph_loss_ref import Composed

LW, TS = 0.8, -0.5
INF = np.inf


def _tg():
    from torch_asg_amd import TokenGraph
    return TokenGraph


def _ngram(N, order, seed, holes=False):
    rng = np.random.default_rng(seed)
    lp = np.log(rng.dirichlet(np.ones(N + 1), size=(N + 1,) * (order - 1))) if order > 1 else np.log(rng.dirichlet(np.ones(N + 1)))
    if holes:
        lp[rng.random(size=lp.shape) < 0.2] = -np.inf
    return _tg().from_ngram(lp)


def _case(T, B, N, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(T, B, N))
    x = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(dtype)
    tr = (0.5 * rng.normal(size=(N, N))).astype(dtype)
    il = rng.integers(2, T + 1, size=B)
    il[0] = T
    if B > 1:
        il[1] = 0
    if B > 2:
        il[2] = 1
    return x, tr, il


def _ref(tr, g, B, W, P, K, tol=0, C=None, theta=INF, dtype=np.float64, w=(LW, TS)):
    return BeamWindowConfRef(tr, g.next, g.weight, g.final, g.start, B, W, P, K, theta, *w, dtype, tol, C)


def _feed(ref, x, il, cuts):
    """-> per slot the concatenated (frames, confidences) of all calls."""
    B = x.shape[1]
    tfs, cfs = [[] for _ in range(B)], [[] for _ in range(B)]
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        o = ref.advance(x[t0:t1], np.clip(il - t0, 0, t1 - t0))
        tf, cf, tl = o[5], o[6], o[4]
        assert tf.shape == cf.shape == (B, ref.W + t1 - t0)
        for b in range(B):
            assert (tf[b, tl[b]:] == -1).all() and (cf[b, tl[b]:] == 0).all() and (tf[b, :tl[b]] >= 0).all()
            tfs[b] += tf[b, :tl[b]].tolist()
            cfs[b] += cf[b, :tl[b]].tolist()
    return tfs, cfs


@pytest.mark.parametrize("W,P", [(4, 1), (4, 3), (8, 8), (16, 3)])
@pytest.mark.parametrize("tol", [0, 2])
def test_committed_tokens_carry_the_growing_streams_prefix_values_byte_for_byte(W, P, tol):
    g = _ngram(6, 3, 3, holes=True)
    T, B, K = 30, 4, 3
    x, tr, il = _case(T, B, g.N, 11)
    ref = _ref(tr, g, B, W, P, K, tol, T)
    tfs, cfs = _feed(ref, x, il, [0, T])
    grow = BeamStreamConfRef(tr, g.next, g.weight, g.final, g.start, B, T, K, INF, LW, TS, np.float64)
    at = {}
    for t in range(T):
        grow.advance(x[t:t + 1], np.clip(il - t, 0, 1))
        r = grow.result_confidence(tol, final=False)
        at[t + 1] = (r["token_frames"].copy(), r["token_confidences"].copy(), r["token_lengths"].copy())
    clear = 0
    for b in range(B):
        k = 0
        for p1, b0, k0, k1, status in ref.ends[b]:
            n = k1 - k0
            if not status & 1:                                   # property 3, while bit 0 is clear
                clear += 1
                gf, gc, gl = at[p1]
                assert gl[b] >= k + n and tfs[b][k:k + n] == gf[b, k:k + n].tolist()
                assert np.array(cfs[b][k:k + n]).tobytes() == gc[b, k:k + n].tobytes()
            k += n
        assert k == len(tfs[b])
    assert clear or W == 4 or P == W                             # (a short window, or P = W, forces from its first attempts on)


def test_frames_of_all_calls_and_the_tail_are_the_one_shot_frames():
    g = _ngram(6, 2, 5)
    T, B, W, P, K = 40, 5, 16, 3, 8
    x, tr, il = _case(T, B, g.N, 17)
    one = beam_conf_ref(x, tr, g.next, g.weight, g.final, g.start, il, K, INF, LW, TS, 1)
    ref = _ref(tr, g, B, W, P, K, 1, T)
    tfs, cfs = _feed(ref, x, il, [0, 13, 13, 40])
    tail = ref.result_confidence(final=True)
    clear = 0
    for b in range(B):
        if tail["status"][b] & 1:
            continue
        clear += 1
        n, m = len(tfs[b]), int(tail["token_lengths"][b])
        assert n + m == one["token_lengths"][b]
        assert tfs[b] + tail["token_frames"][b, :m].tolist() == one["token_frames"][b, :n + m].tolist()
        assert tail["token_confidences"][b, :m].tobytes() == one["token_confidences"][b, n:n + m].tobytes()
        assert tail["normalisers"][b] == one["normalisers"][b]
    assert clear >= 3


@pytest.mark.parametrize("seed", [1, 2])
def test_chunk_invariance(seed):
    g = _ngram(6, 3, 3, holes=True)
    T, B, W, P, K, tol = 30, 4, 8, 3, 3, 1
    x, tr, il = _case(T, B, g.N, 11)
    rng = np.random.default_rng(seed)
    rand = np.sort(np.concatenate([[0, T], rng.integers(0, T + 1, size=8)])).tolist()      # (with empty chunks)
    got = [_feed(_ref(tr, g, B, W, P, K, tol, T), x, il, cuts) for cuts in (list(range(T + 1)), [0, T], rand)]
    assert got[0] == got[1] == got[2] and any(len(t) for t in got[0][0])


def test_against_the_enumeration_of_all_label_paths():
    """T = 5, N = 4, a beam that prunes nothing: the lattice is the full composed graph, and the posterior that a token with label
    i starts at frame t is a sum over the 4^5 label paths the automaton accepts."""
    g = _ngram(4, 2, 7)
    T, N, W, P = 5, 4, 4, 1
    x, tr, _ = _case(T, 1, N, 3)
    il = np.array([T])
    nxt, wt = np.asarray(g.next, np.int64), np.asarray(g.weight, np.float64)

    def prefix_events(L):
        """P [L, N] over the label paths of length L, a path ending anywhere with weight 0."""
        Pn, Zs = np.zeros((L, N)), []
        for lab in itertools.product(range(N), repeat=L):
            s, v, ok = g.start, 0.0, True
            for t, i in enumerate(lab):
                v += x[t, 0, i]
                if t == 0 or i != lab[t - 1]:                    # a new token: an arc of the automaton, weighted
                    if nxt[s, i] < 0 or not np.isfinite(wt[s, i]):
                        ok = False
                        break
                    v += LW * wt[s, i] + TS
                    s = nxt[s, i]
                if t > 0:
                    v += tr[i, lab[t - 1]]
            if ok:
                Zs.append((v, lab))
        Z = np.logaddexp.reduce([v for v, _ in Zs])
        for v, lab in Zs:
            for t, i in enumerate(lab):
                if t == 0 or i != lab[t - 1]:
                    Pn[t, i] += np.exp(v - Z)
        return Pn
    ref = _ref(tr, g, 1, W, P, 10 ** 6, 0, T)
    k = 0
    o = ref.advance(x, il)                                       # one call: the log's token indices are the call's columns
    toks = o[2][0, :o[4][0]].tolist()
    for p1, b0, k0, k1, status in ref.ends[0]:
        Pn = prefix_events(p1)
        for j in range(k0, k1):
            assert abs(o[6][0, j] - Pn[o[5][0, j], toks[j]]) < 1e-12, (p1, j)
            k += 1
    assert k == len(toks) > 0


@pytest.mark.parametrize("K", [2, 4])
def test_forced_commits_keep_the_cell_posteriors(K):
    nxt, w, f = two_components_automaton()
    g = _tg()(nxt, w, f, start=0)
    T, B, W, P = 30, 2, 8, 2
    x = two_component_emissions(T, B, g.N, np.float64)
    tr = np.zeros((g.N, g.N))
    il = np.array([T, T - 3])
    ref = _ref(tr, g, B, W, P, K, 1, 11, w=(1.0, -0.5))
    tol, cuts = 1, [0, 5, 6, 17, 28, 30]
    toks, tfs, cfs = [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)]
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        o = ref.advance(x[t0:t1], np.clip(il - t0, 0, t1 - t0))
        for b in range(B):
            n = int(o[4][b])
            toks[b] += o[2][b, :n].tolist()
            tfs[b] += o[5][b, :n].tolist()
            cfs[b] += o[6][b, :n].tolist()
    assert all(v.status == 1 for v in ref.slots)                 # the regime, from the restatement's own status
    assert any(e[4] & 1 for e in ref.ends[0]) and len(tfs[0]) >= 1
    # property 4: a forced token's value is the cell posterior of an INDEPENDENT growing stream that stands at p1, whatever
    # hypothesis committed it (that stream's own tokens are not looked at: only its events P [p1, N])
    grow = BeamStreamConfRef(tr, g.next, g.weight, g.final, g.start, B, T, K, INF, 1.0, -0.5, np.float64)
    events = {}
    for t in range(T):
        grow.advance(x[t:t + 1], np.clip(il - t, 0, 1))
        events[t + 1] = [e.copy() for e in grow.result_confidence(tol, final=False)["events"]]
    checked = 0
    for b in range(B):
        k = 0
        for p1, b0, k0, k1, status in ref.ends[b]:
            Pm = events[p1][b]
            assert Pm.shape[0] == p1
            for j in range(k, k + k1 - k0):
                fr = tfs[b][j]
                assert b0 <= fr < p1
                want = Pm[max(0, fr - tol):min(p1 - 1, fr + tol) + 1, toks[b][j]].sum()
                assert np.float64(cfs[b][j]).tobytes() == np.float64(want).tobytes(), (b, p1, j)
                checked += bool(status & 1)
            k += k1 - k0
    assert checked


def test_bounds():
    g = _ngram(6, 3, 3, holes=True)
    T, B = 30, 4
    x, tr, il = _case(T, B, g.N, 11)
    tfs, cfs = _feed(_ref(tr, g, B, 8, 3, 3, 0, T), x, il, [0, T])
    assert all(c <= 1 + 1e-12 for cs in cfs for c in cs)          # at tol 0 a cell is an event of probability <= 1
    ref = _ref(tr, g, B, 8, 3, 1, 0, T)                          # K = 1: one path, every commit by convergence, every cell sure
    tfs, cfs = _feed(ref, x, il, [0, T])
    assert all(v.status == 0 for v in ref.slots) and sum(len(c) for c in cfs) > 5
    # (1 in exact arithmetic.  The value is exp(d), d the difference of two float64 sums of at most 2 T terms each, no partial sum
    # above |Z| in magnitude, added in different orders: |d| <= 4 T eps |Z|.)
    Z = np.abs(ref.result_confidence(False)["normalisers"][[0, 3]]).max()
    assert all(abs(c - 1.0) <= 4 * T * np.finfo(np.float64).eps * max(1.0, Z) for cs in cfs for c in cs)


def test_an_emptied_beam_gives_zeros_and_never_a_nan():
    g = _ngram(6, 3, 3, holes=True)
    T, B = 30, 2
    x, tr, il = _case(T, B, g.N, 11)
    il[:] = T
    x[20:, 0] = -np.inf
    ref = _ref(tr, g, B, 8, 3, 3, 1, T)
    tfs, cfs = _feed(ref, x, il, [0, 10, 30])
    assert ref.slots[0].aq.size == 0 and ref.slots[0].base > 0 and len(tfs[0]) > 0
    r = ref.result_confidence(False)
    assert r["normalisers"][0] == -np.inf and (r["token_confidences"][0] == 0).all() and (r["token_frames"][0] == -1).all()
    assert not np.isnan(r["token_confidences"]).any() and not np.isnan(np.array(cfs[1])).any()


def test_a_chunk_longer_than_max_chunk_is_refused():
    g = _ngram(4, 2, 7)
    x, tr, il = _case(6, 1, g.N, 3)
    with pytest.raises(AssertionError):
        _ref(tr, g, 1, 4, 1, 2, 0, 5).advance(x, il)


def test_the_python_surface_without_a_device():
    import torch
    import torch_asg_amd as a
    assert a.BeamWindowConfCommit._fields == a.BeamWindowCommit._fields + ("token_frames", "token_confidences")
    assert a.BeamWindowConfidence._fields == ("scores", "path", "tokens", "token_lengths", "states", "token_frames",
                                              "token_confidences", "normalisers", "frames", "committed", "status")
    cs = a.BeamWindowStream._check_shape
    assert cs(None, 2, 8, None) == (8, 2) and cs(None, 2, 8, 3, 1, None) == (8, 3, 1, 8) and cs(None, 2, 8, 3, 0, 5) == (8, 3, 0, 5)
    for bad in ((2, 8, 3, -1, None), (2, 8, 3, 0, 0)):
        with pytest.raises(ValueError):
            cs(None, *bad)
