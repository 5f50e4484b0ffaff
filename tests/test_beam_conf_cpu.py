"""CPU tests that pin the numpy restatement of the token confidences (tests/beam_conf_ref.py) before the GPU tests compare the
kernels with it: every P(i, t) against the enumeration of all label paths, the properties the specification states (K = 1, the
bounds at tolerance 0, the starts at frame 0 summing to one, the starts of a label as a derivative of Z_K, a double start above
1, lengths 1 and 0, a beam that empties), and the C ABI of asg_beam_graph_confidence (symbols, sizes, argument checks) and the
Python surfaces' argument errors -- no kernel is launched here."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch_asg_amd

from beam_conf_ref import beam_conf_ref, start_frames
from beam_loss_cases import _lexicon, _ngram, _random_graph
from beam_loss_ref import beam_loss_ref
from graph_decode_ref import path_score_graph
from graph_loss_ref import Composed, _lse
from test_beam_loss_cpu import _host_view, _path_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
ALL = 10_000
KW = dict(lm_weight=0.8, token_score=0.2)
NAMES = ["asg_beam_graph_confidence_work_bytes", "asg_beam_graph_confidence"]
FIELDS = torch_asg_amd.BeamGraphConfidence._fields      # what the restatement has to return: the public tuple's own fields

# the four automata of tests/beam_loss_cases.py, over N = 4 tokens so that every label path of T = 5 can be enumerated
SMALL = {
    "unigram": lambda: _ngram(4, 1, 1),
    "trigram_holes": lambda: _ngram(4, 3, 3, holes=True),
    "random": lambda: _random_graph(8, 4, 4),
    "lexicon": lambda: _lexicon(4, 12, 5, maxlen=3),
}


def _ref(x, tr, g, il, K, th=INF, tol=0, **kw):
    kw = dict(KW, **kw)
    r = beam_conf_ref(x, tr, g.next, g.weight, g.final, g.start, il, K, th, kw["lm_weight"], kw["token_score"], tol)
    assert all(n in r for n in FIELDS)
    return r


def _emissions(T, B, N, seed, dt=np.float64, scale=1.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.normal(size=(T, B, N))).astype(dt), (0.5 * rng.normal(size=(N, N))).astype(dt)


# ---------------------------------------------------------------------------------------------------------------- enumeration
@pytest.mark.parametrize("name", sorted(SMALL))
def test_every_event_posterior_is_the_sum_over_exactly_the_paths_inside_the_sets(name):
    g = SMALL[name]()
    T, N = 5, 4
    x, tr = _emissions(T, 1, N, 41)
    comp = Composed(g.next, g.weight, g.final, g.start, KW["lm_weight"], KW["token_score"])
    scored = []
    for labels in itertools.product(range(N), repeat=T):                   # all 1024 label paths
        qs = _path_states(labels, g.next, comp.present, g.start, comp)
        if qs is None:
            continue
        s = path_score_graph(x[:, 0], tr, g.next, g.weight, g.final, labels, g.start, KW["lm_weight"], KW["token_score"])[0]
        if s > -np.inf:
            scored.append((s, qs, labels))
    assert len(scored) > 10
    pruned = 0
    for K in (ALL, 1, 2, 3, 8):
        res = {tol: _ref(x, tr, g, None, K, tol=tol) for tol in (0, 1, 5)}
        sets = [set(int(q) for q in u) for u in res[0]["sets"][0]]
        inside = [(s, labels) for s, qs, labels in scored if all(q in sets[t] for t, q in enumerate(qs))]
        assert inside
        pruned += len(inside) < len(scored)
        Z = _lse([s for s, _ in inside])
        assert np.allclose(res[0]["normalisers"][0], Z, rtol=1e-9, atol=1e-9), K
        direct = np.zeros((T, N))
        for s, labels in inside:
            for t in start_frames(labels):
                direct[t, labels[t]] += np.exp(s - Z)
        assert np.allclose(res[0]["events"][0], direct, rtol=1e-9, atol=1e-9), K
        # the hypothesis: the winning path is the best path inside the sets, its frames are the starts of its runs
        best = max(inside, key=lambda it: it[0])[1]
        sk = start_frames(best)
        n = int(res[0]["token_lengths"][0])
        assert n == len(sk) and [best[t] for t in sk] == list(res[0]["tokens"][0, :n])
        for tol in (0, 1, 5):
            r = res[tol]
            assert list(r["token_frames"][0, :n]) == sk
            assert (r["token_frames"][0, n:] == -1).all() and (r["token_confidences"][0, n:] == 0).all()
            for k, s in enumerate(sk):
                want = sum(direct[t, best[s]] for t in range(T) if abs(t - s) <= tol)
                assert abs(r["token_confidences"][0, k] - want) < 1e-9, (K, tol, k)
    assert pruned >= 2                                                     # the narrow beams did cut paths away


# ---------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("name", sorted(SMALL))
def test_a_beam_of_one_is_sure_of_every_token(name):
    g = SMALL[name]()
    x, tr = _emissions(9, 3, 4, 7)
    il = np.array([9, 4, 1])
    r0, r2 = _ref(x, tr, g, il, 1), _ref(x, tr, g, il, 1, tol=2)
    some = 0
    for b in range(3):
        n = int(r0["token_lengths"][b])
        if not np.isfinite(r0["scores"][b]):
            assert n == 0 and r0["normalisers"][b] == -np.inf
            continue
        some += 1
        assert np.allclose(r0["normalisers"][b], r0["scores"][b], rtol=1e-12, atol=1e-12)
        assert np.allclose(r0["token_confidences"][b, :n], 1.0, rtol=1e-12, atol=1e-12)
        tk, s = r2["tokens"][b, :n], r2["token_frames"][b, :n]
        count = [sum(1 for j in range(n) if tk[j] == tk[k] and abs(int(s[j]) - int(s[k])) <= 2) for k in range(n)]
        assert np.allclose(r2["token_confidences"][b, :n], count, rtol=1e-12, atol=1e-12)
    assert some or name == "lexicon"


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_at_tolerance_zero_a_confidence_lies_between_the_paths_share_and_one(dt):
    eps = 1e-5 if dt == np.float32 else 1e-12
    seen = 0
    for name in sorted(SMALL):
        g = SMALL[name]()
        for seed, K, th in itertools.product((1, 2), (1, 2, 4, ALL), (INF, 2.0)):
            x, tr = _emissions(8, 2, 4, 50 + seed, dt)
            r = _ref(x, tr, g, np.array([8, 5]), K, th)
            for b in range(2):
                n = int(r["token_lengths"][b])
                if n == 0:
                    continue
                seen += 1
                share = np.exp(np.float64(r["scores"][b]) - r["normalisers"][b])
                c = r["token_confidences"][b, :n]
                assert (c >= share - eps).all() and (c <= 1 + eps).all() and share <= 1 + eps
    assert seen > 40


def test_the_starts_at_frame_zero_sum_to_one_and_the_starts_of_a_label_are_a_derivative_of_z():
    for name in sorted(SMALL):
        g = SMALL[name]()
        for K in (2, 5, ALL):
            x, tr = _emissions(7, 2, 4, 90)
            il = np.array([7, 4])
            r = _ref(x, tr, g, il, K)
            Z, _, _, _ = beam_loss_ref(x, tr, g.next, g.weight, g.final, g.start, il, K, INF, KW["lm_weight"], KW["token_score"])
            assert np.array_equal(Z, r["normalisers"])
            for b in range(2):
                if not np.isfinite(Z[b]):
                    continue
                P = r["events"][b]
                assert abs(P[0].sum() - 1.0) < 1e-12
                gs = np.zeros(2)
                gs[b] = 1.0
                gtr = beam_loss_ref(x, tr, g.next, g.weight, g.final, g.start, il, K, INF, KW["lm_weight"], KW["token_score"],
                                    grad_scores=gs)[2]
                off = gtr - np.diag(np.diag(gtr))                          # [i][j], j != i: the edges into label i
                assert np.allclose(P[1:].sum(0), off.sum(1), rtol=1e-10, atol=1e-12), (name, K, b)


def double_start_case(dt=np.float64):
    """"a b a" in three frames over a unigram: the window of tolerance 2 around the first a holds the second one."""
    g = _ngram(4, 1, 1)
    x = np.full((3, 1, 4), -6.0)
    x[0, 0, 1] = x[1, 0, 2] = x[2, 0, 1] = 0.0
    return g, x.astype(dt), np.zeros((4, 4), dt)


def test_a_label_started_twice_inside_the_window_counts_twice():
    g, x, tr = double_start_case()
    r0, r2 = _ref(x, tr, g, None, ALL), _ref(x, tr, g, None, ALL, tol=2)
    assert list(r0["tokens"][0, :3]) == [1, 2, 1] and list(r0["token_frames"][0, :3]) == [0, 1, 2]
    assert (r0["token_confidences"][0, :3] <= 1 + 1e-12).all()
    assert r2["token_confidences"][0, 0] > 1.5 and r2["token_confidences"][0, 2] > 1.5
    assert r2["token_confidences"][0, 1] <= 1 + 1e-12                      # b starts once


def test_lengths_one_and_zero_and_a_beam_that_empties():
    g = _ngram(4, 1, 1)
    x, tr = _emissions(6, 3, 4, 5)
    r = _ref(x, tr, g, np.array([1, 0, 6]), 3, tol=1)
    assert r["token_lengths"][0] == 1 and r["token_frames"][0, 0] == 0 and (r["token_frames"][0, 1:] == -1).all()
    P = r["events"][0]
    assert P.shape == (1, 4) and abs(P.sum() - 1) < 1e-12
    assert abs(r["token_confidences"][0, 0] - P[0, r["tokens"][0, 0]]) < 1e-15
    assert r["scores"][1] == -np.inf and r["normalisers"][1] == -np.inf and r["token_lengths"][1] == 0
    assert (r["token_frames"][1] == -1).all() and (r["token_confidences"][1] == 0).all()
    # an automaton that dies after two tokens: the beam is empty from frame 2 on ... unless the path stays
    nxt = np.array([[1, 1], [2, -1], [-1, -1]])
    dead = __import__("torch_asg_amd").TokenGraph(nxt, np.zeros((3, 2)), np.array([-np.inf, -np.inf, -np.inf]))
    x2, tr2 = _emissions(5, 1, 2, 6)
    r = beam_conf_ref(x2, tr2, dead.next, dead.weight, dead.final, dead.start, None, 4, INF)
    assert r["normalisers"][0] == -np.inf and r["scores"][0] == -np.inf and not np.isnan(r["token_confidences"]).any()
    assert (r["token_confidences"] == 0).all() and (r["token_frames"] == -1).all()
    x3 = x2.copy()
    x3[1:, 0, :] = -np.inf                                                 # every candidate of frame 1 is -inf: the beam empties
    ok = __import__("torch_asg_amd").TokenGraph(np.zeros((1, 2), np.int64), np.zeros((1, 2)), np.zeros(1))
    r = beam_conf_ref(x3, tr2, ok.next, ok.weight, ok.final, ok.start, None, 4, INF)
    assert r["sizes"][0][0] > 0 and r["sizes"][0][1] == 0
    assert r["normalisers"][0] == -np.inf and (r["token_confidences"] == 0).all() and (r["token_frames"] == -1).all()


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code) and hasattr(L, n) and n in _lib.SYMBOLS
    assert "#define ASG_HIP_VERSION 230" in src and _lib.ABI_VERSION == 230


def test_work_bytes_are_the_stated_formula_and_targets_change_nothing():
    import torch_asg_amd
    from torch_asg_amd import _lib
    L = _lib.lib()
    al = lambda n: (n + 255) // 256 * 256                                  # noqa: E731
    graph = _ngram(6, 2, 2)
    for dt, e in ((np.float32, 4), (np.float64, 8)):
        Q = graph.compile_host(dt)["Q"]
        for T, B, K, S in ((7, 3, 16, 0), (100, 2, 300, 40), (5, 1, 8, 9)):
            p, gl, keep = _host_view(graph, dt, T, B, S=S)
            M = min(K, Q)
            dec = int(L.asg_beam_decode_graph_work_bytes(ctypes.byref(p), gl.beam, K))
            a = int(L.asg_beam_graph_confidence_work_bytes(ctypes.byref(p), ctypes.byref(gl), K))
            assert a == B * (dec // B + 2 * al(T * 4) + 256 + al(T * M * 4) + al(T * M * e) + al(2 * M * e)) > 0
            p.S = 2 * max(S, 1)                                            # a doubled target length in the problem
            assert a == int(L.asg_beam_graph_confidence_work_bytes(ctypes.byref(p), ctypes.byref(gl), K))
            p.targets = None
            assert a == int(L.asg_beam_graph_confidence_work_bytes(ctypes.byref(p), ctypes.byref(gl), K))
            tail = 2 * al(B * 8) + al(3 * B * T * 8)                       # what the loss keeps behind the utterances
            assert a == int(L.asg_beam_graph_full_work_bytes(ctypes.byref(p), ctypes.byref(gl), K, 1)) - tail + B * al(2 * M * e)
    assert hasattr(torch_asg_amd.TokenGraph, "compile_beam_loss")


def test_abi_argument_checks_without_a_device():
    import torch_asg_amd
    from torch_asg_amd import _lib
    L = _lib.lib()
    graph = _ngram(6, 2, 2)
    outs = ["scores", "path", "tokens", "token_lengths", "states", "token_frames", "token_confidences", "normalisers"]
    for dt in (np.float32, np.float64):
        p, gl, keep = _host_view(graph, dt, 50, 4, S=10)
        wb = lambda K: int(L.asg_beam_graph_confidence_work_bytes(ctypes.byref(p), ctypes.byref(gl), K))      # noqa: E731

        def call(K=8, th=1.0, tol=0, work=256, nbytes=1 << 40, view=gl, **null):
            ptrs = [None if n in null else 256 for n in outs]
            return L.asg_beam_graph_confidence(None, ctypes.byref(p), None if view is None else ctypes.byref(view), K, th, tol, work,
                                               nbytes, *ptrs, 0, None)
        # asg_beam_graph_full_forward's argument checks
        assert wb(8) > 0 and wb(0) == 0
        assert call(K=0) == 1 and call(th=-1.0) == 1 and call(th=float("nan")) == 1 and call(view=None) == 1
        assert call(work=None) == 1
        for n in outs:
            assert call(**{n: None}) == 1, n
        # the tolerance
        assert call(tol=-1) == 1 and call(tol=65) == 2 and call(tol=-1, work=None) == 1 and call(tol=64, nbytes=0) == 3
        # a workspace one byte short, before anything is launched
        assert call(nbytes=wb(8) - 1) == 3 and call(tol=64, nbytes=wb(8) - 1) == 3
        # targets in the problem are not looked at: a target length beyond the loss's limit is no error here
        p.S, p.T = 5000, 5000
        assert L.asg_beam_graph_full_forward(None, ctypes.byref(p), ctypes.byref(gl), 8, 1.0, 256, 1 << 40, 256, 0, None) == 2
        assert call(nbytes=0) == 3
        p.S, p.T = 10, (1 << 20) + 1
        assert call() == 2 and wb(8) == 0
        p.T = 50
        old = gl.start
        gl.start = graph.S
        assert call() == 1 and wb(8) == 0
        gl.start = old
    big = torch_asg_amd.TokenGraph(np.zeros((1, 1025), np.int64), np.zeros((1, 1025)), np.zeros(1))
    p2, gl2, keep2 = _host_view(big, np.float32, 5, 1)
    assert L.asg_beam_graph_confidence(None, ctypes.byref(p2), ctypes.byref(gl2), 8, 1.0, 0, 256, 1 << 40, *([256] * 8), 0,
                                       None) == 2                          # N > 1024


# ---------------------------------------------------------------------------------------------------------------- Python
def test_python_surfaces_refuse_bad_arguments_before_any_launch():
    import torch_asg_amd as A
    from torch_asg_amd.asg import native
    g = _ngram(5, 2, 2)
    x, tr = torch.zeros(4, 2, 5), torch.zeros(5, 5)
    crit = A.ASGLoss(5)
    surfaces = (lambda *a, **k: A.beam_decode_graph_confidence(x, tr, *a, **k),
                lambda graph, **k: native().beam_decode_graph_confidence(x, tr, graph, None, k.pop("beam_size", 8), **k),
                lambda *a, **k: crit.beam_decode_graph_confidence(x, *a, **k))
    for f in surfaces:
        with pytest.raises(TypeError, match="TokenGraph"):
            f(None)
        with pytest.raises(RuntimeError, match="tokens"):
            f(_ngram(4, 1, 1))
        with pytest.raises(RuntimeError, match="ROCm device"):             # the arguments are checked before the device
            f(g, frame_tolerance=1)
    with pytest.raises(ValueError, match="beam_size"):
        A.beam_decode_graph_confidence(x, tr, g, beam_size=0)
    with pytest.raises(ValueError, match="beam_threshold"):
        crit.beam_decode_graph_confidence(x, g, beam_threshold=-1.0)
    for name in ("BeamGraphConfidence", "beam_decode_graph_confidence"):
        assert name in A.__all__ and hasattr(A, name)
    assert A.BeamGraphConfidence._fields == ("scores", "path", "tokens", "token_lengths", "states", "token_frames",
                                             "token_confidences", "normalisers")
