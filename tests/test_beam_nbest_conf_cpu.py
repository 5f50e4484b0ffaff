"""CPU tests that pin the numpy restatement of the token confidences of every row of the token-graph n-best list
(tests/beam_nbest_conf_ref.py) before the GPU tests compare the kernels with it: every row against the enumeration of all label
paths, row 0 against tests/beam_conf_ref.py, the bounds at tolerance 0, cells shared by rows, the degenerate utterances, and the
C ABI of asg_beam_graph_nbest_confidence (symbols, sizes, every argument error in its order, the LDS limit on both sides) and
the Python surfaces' argument errors -- no kernel is launched here."""
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
from beam_nbest_conf_ref import NAMES as EIGHT, beam_nbest_conf_ref, window_confidences
from graph_decode_ref import path_score_graph
from graph_loss_ref import Composed, _lse
from test_beam_loss_cpu import _host_view, _path_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
ALL = 10_000
KW = dict(lm_weight=0.8, token_score=0.2)
CALLS = ("asg_beam_graph_nbest_confidence_work_bytes", "asg_beam_graph_nbest_confidence")
FIELDS = ("scores", "emission_scores", "graph_scores", "tokens", "token_lengths", "num_hyps", "path", "states", "token_frames",
          "token_confidences", "normalisers")

# the four automata of tests/beam_loss_cases.py, over N = 4 tokens so that every label path of T = 5 can be enumerated
SMALL = {
    "unigram": lambda: _ngram(4, 1, 1),
    "trigram_holes": lambda: _ngram(4, 3, 3, holes=True),
    "random": lambda: _random_graph(8, 4, 4),
    "lexicon": lambda: _lexicon(4, 12, 5, maxlen=3),
}


def _ref(x, tr, g, il, K, nbest, th=INF, tol=0, **kw):
    kw = dict(KW, **kw)
    r = beam_nbest_conf_ref(x, tr, g.next, g.weight, g.final, g.start, il, K, nbest, th, kw["lm_weight"], kw["token_score"], tol)
    assert all(n in r for n in FIELDS)
    return r


def _one(x, tr, g, il, K, th=INF, tol=0):
    return beam_conf_ref(x, tr, g.next, g.weight, g.final, g.start, il, K, th, KW["lm_weight"], KW["token_score"], tol)


def _emissions(T, B, N, seed, dt=np.float64, scale=1.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.normal(size=(T, B, N))).astype(dt), (0.5 * rng.normal(size=(N, N))).astype(dt)


# ---------------------------------------------------------------------------------------------------------------- enumeration
@pytest.mark.parametrize("name", sorted(SMALL))
def test_every_row_reads_the_sum_over_exactly_the_paths_inside_the_sets(name):
    g = SMALL[name]()
    T, N, nbest = 5, 4, 6
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
    pruned = rows_seen = 0
    for K in (ALL, 1, 2, 3, 8):
        res = {tol: _ref(x, tr, g, None, K, nbest, tol=tol) for tol in (0, 1, 5)}
        sets = [set(int(q) for q in u) for u in res[0]["sets"][0]]
        inside = {labels: s for s, qs, labels in scored if all(q in sets[t] for t, q in enumerate(qs))}
        assert inside
        pruned += len(inside) < len(scored)
        Z = _lse(list(inside.values()))
        assert np.allclose(res[0]["normalisers"][0], Z, rtol=1e-9, atol=1e-9), K
        direct = np.zeros((T, N))
        for labels, s in inside.items():
            for t in start_frames(labels):
                direct[t, labels[t]] += np.exp(s - Z)
        nh = int(res[0]["num_hyps"][0])
        assert 1 <= nh <= min(nbest, len(sets[T - 1]))
        assert (np.diff(res[0]["scores"][0, :nh]) <= 0).all()
        for r in range(nh):
            rows_seen += 1
            labels = tuple(int(v) for v in res[0]["path"][0, r])
            assert labels in inside and abs(inside[labels] - res[0]["scores"][0, r]) < 1e-9  # a row is a lattice path
            sk = start_frames(labels)
            n = int(res[0]["token_lengths"][0, r])
            assert n == len(sk) and [labels[t] for t in sk] == list(res[0]["tokens"][0, r, :n])
            for tol in (0, 1, 5):
                rr = res[tol]
                assert list(rr["token_frames"][0, r, :n]) == sk
                assert (rr["token_frames"][0, r, n:] == -1).all() and (rr["token_confidences"][0, r, n:] == 0).all()
                for k, s in enumerate(sk):
                    want = sum(direct[t, labels[s]] for t in range(T) if abs(t - s) <= tol)
                    assert abs(rr["token_confidences"][0, r, k] - want) < 1e-9, (K, tol, r, k)
        for tol in (0, 1, 5):                                              # the padding rows
            assert (res[tol]["token_frames"][0, nh:] == -1).all() and (res[tol]["token_confidences"][0, nh:] == 0).all()
    assert pruned >= 2 and rows_seen >= 8                                  # the narrow beams did cut paths away


# ---------------------------------------------------------------------------------------------------------------- row 0
@pytest.mark.parametrize("name", sorted(SMALL))
def test_row_zero_and_a_list_of_one_are_the_one_best_confidences(name):
    g = SMALL[name]()
    x, tr = _emissions(9, 3, 4, 7)
    il = np.array([9, 4, 1])
    for K, th, tol in ((1, INF, 0), (3, INF, 1), (ALL, 2.0, 2), (ALL, INF, 5)):
        one = _one(x, tr, g, il, K, th, tol)
        for nbest in (1, 5):
            r = _ref(x, tr, g, il, K, nbest, th, tol)
            assert np.array_equal(r["normalisers"], one["normalisers"])
            assert np.array_equal(r["token_frames"][:, 0], one["token_frames"])
            assert np.array_equal(r["token_confidences"][:, 0], one["token_confidences"])
            for n in ("scores", "tokens", "token_lengths", "path", "states"):
                assert np.array_equal(r[n][:, 0], one[n]), n
            assert np.array_equal(window_confidences(r, il, tol), r["token_confidences"])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_at_tolerance_zero_every_token_of_every_row_lies_between_the_rows_share_and_one(dt):
    eps = 1e-5 if dt == np.float32 else 1e-12
    seen = lower = 0
    for name in sorted(SMALL):
        g = SMALL[name]()
        for seed, K, th in itertools.product((1, 2), (1, 2, 4, ALL), (INF, 2.0)):
            x, tr = _emissions(8, 2, 4, 50 + seed, dt)
            r = _ref(x, tr, g, np.array([8, 5]), K, 4, th)
            for b in range(2):
                for row in range(int(r["num_hyps"][b])):
                    n = int(r["token_lengths"][b, row])
                    assert n >= 1
                    seen += 1
                    lower += row > 0
                    share = np.exp(np.float64(r["scores"][b, row]) - r["normalisers"][b])
                    c = r["token_confidences"][b, row, :n]
                    assert (c >= share - eps).all() and (c <= 1 + eps).all() and share <= 1 + eps
    assert seen > 80 and lower > 30


# ---------------------------------------------------------------------------------------------------------------- cells
def cells_case(dt=np.float64):
    """A bigram over 5 tokens at T = 6 with the whole beam: among the rows, a cell read by two rows, a label that two rows start
    one frame apart, and a frame at which the rows start different labels (asserted by the test below)."""
    x, tr = _emissions(6, 1, 5, 0, dt)
    return _ngram(5, 2, 2), x, tr


def test_rows_share_cells_shift_windows_and_differ_within_a_frame():
    g, x, tr = cells_case()
    r0, r1 = _ref(x, tr, g, None, ALL, 8), _ref(x, tr, g, None, ALL, 8, tol=1)
    nh = int(r0["num_hyps"][0])
    assert nh >= 4
    P = r0["events"][0]
    toks = {}                                                              # (frame, label) -> [(row, k)]
    for r in range(nh):
        for k in range(int(r0["token_lengths"][0, r])):
            toks.setdefault((int(r0["token_frames"][0, r, k]), int(r0["tokens"][0, r, k])), []).append((r, k))
    assert sorted(toks) == r0["cells"][0] and r0["queries"][0] == sum(len(v) for v in toks.values()) > len(toks)
    shared = [v for v in toks.values() if len(set(r for r, _ in v)) >= 2]
    assert shared                                                          # two rows read one cell ...
    for res in (r0, r1):
        for v in shared:
            assert len(set(res["token_confidences"][0, r, k] for r, k in v)) == 1                  # ... and get one value
    shifted = [(t, c) for (t, c) in toks if (t + 1, c) in toks and t >= 1 and t + 2 <= 5
               and set(r for r, _ in toks[(t, c)]) != set(r for r, _ in toks[(t + 1, c)])]
    assert shifted                                                         # the same label one frame apart in two rows
    for t, c in shifted:
        (ra, ka), (rb, kb) = toks[(t, c)][0], toks[(t + 1, c)][0]
        a, b = r1["token_confidences"][0, ra, ka], r1["token_confidences"][0, rb, kb]
        assert abs(a - P[t - 1:t + 2, c].sum()) < 1e-15 and abs(b - P[t:t + 3, c].sum()) < 1e-15
        assert abs((b - a) - (P[t + 2, c] - P[t - 1, c])) < 1e-12          # the same window sum, moved by one frame
    frames = {}
    for t, c in toks:
        frames.setdefault(t, set()).add(c)
    assert any(len(v) >= 2 for v in frames.values())                       # the rows of one frame hold different labels


# ---------------------------------------------------------------------------------------------------------------- edges
def test_lengths_one_and_zero_an_empty_beam_no_final_weight_and_fewer_candidates_than_nbest():
    g = _ngram(4, 1, 1)
    x, tr = _emissions(6, 3, 4, 5)
    r = _ref(x, tr, g, np.array([1, 0, 6]), 3, 5, tol=1)
    assert r["num_hyps"][0] == 3 and (r["token_lengths"][0, :3] == 1).all() and (r["token_frames"][0, :3, 0] == 0).all()
    P = r["events"][0]
    assert P.shape == (1, 4) and abs(P.sum() - 1) < 1e-12
    for row in range(3):
        assert abs(r["token_confidences"][0, row, 0] - P[0, r["tokens"][0, row, 0]]) < 1e-15
    assert abs(r["token_confidences"][0, :3, 0].sum() - 1) < 1e-12         # the three kept states are the whole lattice
    assert (r["token_frames"][0, :, 1:] == -1).all() and (r["token_frames"][0, 3:] == -1).all()
    assert (r["token_confidences"][0, 3:] == 0).all()                      # fewer candidates than nbest: padding rows
    assert r["num_hyps"][1] == 0 and r["normalisers"][1] == -np.inf and (r["scores"][1] == -np.inf).all()
    assert (r["token_frames"][1] == -1).all() and (r["token_confidences"][1] == 0).all()
    assert r["num_hyps"][2] == 3
    # an end without a final weight
    nxt = np.array([[1, 1], [2, -1], [-1, -1]])
    dead = torch_asg_amd.TokenGraph(nxt, np.zeros((3, 2)), np.array([-np.inf, -np.inf, -np.inf]))
    x2, tr2 = _emissions(5, 1, 2, 6)
    r = beam_nbest_conf_ref(x2, tr2, dead.next, dead.weight, dead.final, dead.start, None, 4, 3, INF)
    assert r["num_hyps"][0] == 0 and r["normalisers"][0] == -np.inf and (r["scores"] == -np.inf).all()
    assert not np.isnan(r["token_confidences"]).any() and (r["token_confidences"] == 0).all() and (r["token_frames"] == -1).all()
    # a beam that empties
    x3 = x2.copy()
    x3[1:, 0, :] = -np.inf
    ok = torch_asg_amd.TokenGraph(np.zeros((1, 2), np.int64), np.zeros((1, 2)), np.zeros(1))
    r = beam_nbest_conf_ref(x3, tr2, ok.next, ok.weight, ok.final, ok.start, None, 4, 3, INF)
    assert r["sizes"][0][0] > 0 and r["sizes"][0][1] == 0 and r["num_hyps"][0] == 0
    assert r["normalisers"][0] == -np.inf and (r["token_confidences"] == 0).all() and (r["token_frames"] == -1).all()


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for n in CALLS:
        assert re.search(r"\b%s\s*\(" % n, code) and hasattr(L, n) and n in _lib.SYMBOLS
    assert "#define ASG_HIP_VERSION 230" in src and _lib.ABI_VERSION == 230


def _p2(n):
    r = 2
    while r < n:
        r *= 2
    return r


def test_work_bytes_are_the_stated_formula_and_targets_change_nothing():
    from torch_asg_amd import _lib
    L = _lib.lib()
    al = lambda n: (n + 255) // 256 * 256                                  # noqa: E731
    graph = _ngram(6, 2, 2)
    for dt, e in ((np.float32, 4), (np.float64, 8)):
        Q = graph.compile_host(dt)["Q"]
        for T, B, K, S, nbest in ((7, 3, 16, 0, 1), (100, 2, 300, 40, 10), (5, 1, 8, 9, 100), (130, 2, 30, 0, 20)):
            p, gl, keep = _host_view(graph, dt, T, B, S=S)
            M = min(K, Q)
            nb = min(nbest, M)
            conf = int(L.asg_beam_graph_confidence_work_bytes(ctypes.byref(p), ctypes.byref(gl), K))
            a = int(L.asg_beam_graph_nbest_confidence_work_bytes(ctypes.byref(p), ctypes.byref(gl), K, nbest))
            assert conf % B == 0
            per = (conf // B + al(8 + M * e) + al(T * nb * 4) + 256 + al((T + 2) * 4) + al(_p2(nb * T) * 8) + 2 * al(nb * T * 8))
            assert a == B * per + 2 * al(B * 8) + al(3 * B * T * 8) > 0
            p.S = 2 * max(S, 1)                                            # a doubled target length in the problem
            assert a == int(L.asg_beam_graph_nbest_confidence_work_bytes(ctypes.byref(p), ctypes.byref(gl), K, nbest))
            p.targets = None
            assert a == int(L.asg_beam_graph_nbest_confidence_work_bytes(ctypes.byref(p), ctypes.byref(gl), K, nbest))


def _lds(M, e, rows, tol):
    """The left side of the limit stated in include/asg_hip.h."""
    return 16 * ((M * (e + 4) + 15) // 16) + 1024 + 12 * _p2(rows * (2 * tol + 2))


def test_abi_argument_checks_without_a_device():
    from torch_asg_amd import _lib
    L = _lib.lib()
    graph = _ngram(6, 2, 2)
    outs = ["scores", "emission_scores", "graph_scores", "path", "tokens", "token_lengths", "states", "num_hyps", "token_frames",
            "token_confidences", "normalisers"]
    optional = ("path", "states")
    for dt in (np.float32, np.float64):
        p, gl, keep = _host_view(graph, dt, 50, 4, S=10)
        wb = lambda K, n=4: int(L.asg_beam_graph_nbest_confidence_work_bytes(ctypes.byref(p), ctypes.byref(gl), K, n))    # noqa: E731

        def call(K=8, th=1.0, nbest=4, tol=0, work=256, nbytes=1 << 40, view=gl, **null):
            ptrs = [None if n in null else 256 for n in outs]
            return L.asg_beam_graph_nbest_confidence(None, ctypes.byref(p), None if view is None else ctypes.byref(view), K, th, nbest,
                                                     tol, work, nbytes, *ptrs, 0, None)
        # asg_beam_graph_confidence's checks of p, gl and beam_size come first
        assert wb(8) > 0 and wb(0) == 0 and wb(8, 0) == 0 and wb(8, 8193) == 0
        assert call(K=0) == 1 and call(view=None) == 1 and call(K=0, nbest=8193) == 1 and call(view=None, tol=65) == 1
        # nbest, before the tolerance
        assert call(nbest=0) == 1 and call(nbest=8193) == 2 and call(nbest=0, tol=65) == 1 and call(nbest=8193, tol=-1) == 2
        # the tolerance, before the threshold, the buffers and the workspace
        assert call(tol=-1) == 1 and call(tol=65) == 2 and call(tol=65, th=-1.0) == 2 and call(tol=-1, work=None) == 1
        assert call(tol=65, nbytes=0) == 2
        # the threshold, before the buffers
        assert call(th=-1.0) == 1 and call(th=float("nan")) == 1 and call(th=-1.0, nbytes=0) == 1
        # a NULL buffer, before the workspace; path and states may be NULL
        assert call(work=None) == 1 and call(work=None, nbytes=0) == 1
        for n in outs:
            assert call(nbytes=0, **{n: None}) == (3 if n in optional else 1), n
        # a workspace one byte short, before anything is launched
        assert call(nbytes=wb(8) - 1) == 3 and call(tol=64, nbytes=wb(8) - 1) == 3 and call(nbest=100, nbytes=wb(8, 100) - 1) == 3
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
    assert L.asg_beam_graph_nbest_confidence(None, ctypes.byref(p2), ctypes.byref(gl2), 8, 1.0, 4, 0, 256, 1 << 40, *([256] * 11), 0,
                                             None) == 2                    # N > 1024


def test_the_lds_limit_on_both_sides_at_two_beams():
    """16 * ceil(M (e + 4) / 16) + 1024 + 12 * P2(min(nbest, K) * (2 tol + 2)) <= 163840, and min(nbest, K) * T <= 2^30: the
    expression of the header, evaluated here, decides which side a combination is on."""
    from torch_asg_amd import _lib
    L = _lib.lib()
    graph = _ngram(40, 3, 13)
    for dt, e in ((np.float32, 4), (np.float64, 8)):
        assert graph.compile_host(dt)["Q"] == 1640
        p, gl, keep = _host_view(graph, dt, 50, 2)

        def call(K, nbest, tol):
            return L.asg_beam_graph_nbest_confidence(None, ctypes.byref(p), ctypes.byref(gl), K, 1.0, nbest, tol, 256, 0,
                                                     *([256] * 11), 0, None)
        for K, inside, beyond in ((64, (63, 64), (64, 64)), (64, (64, 63), (100, 64)),
                                  (1024, (1024, 3), (1024, 4)), (1024, (63, 64), (64, 64))):
            rows = lambda n: min(n, K)                                     # noqa: E731
            assert _lds(K, e, rows(inside[0]), inside[1]) <= 163840 < _lds(K, e, rows(beyond[0]), beyond[1])
            assert call(K, *inside) == 3                                   # accepted up to the (empty) workspace
            assert call(K, *beyond) == 2
            assert L.asg_beam_graph_nbest_confidence_work_bytes(ctypes.byref(p), ctypes.byref(gl), K, beyond[0]) > 0   # (no tol in the size)
        p.T = 1 << 20
        assert min(8192, 1640) * p.T > 1 << 30 >= 1024 * p.T
        assert call(8192, 8192, 0) == 2 and call(8192, 1024, 0) == 3
        p.T = 50


# ---------------------------------------------------------------------------------------------------------------- Python
def test_python_surfaces_refuse_bad_arguments_before_any_launch():
    import torch_asg_amd as A
    from torch_asg_amd.asg import native
    g = _ngram(5, 2, 2)
    x, tr = torch.zeros(4, 2, 5), torch.zeros(5, 5)
    crit = A.ASGLoss(5)
    surfaces = (lambda *a, **k: A.beam_decode_graph_nbest_confidence(x, tr, *a, **k),
                lambda graph, **k: native().beam_decode_graph_nbest_confidence(x, tr, graph, None, k.pop("beam_size", 8),
                                                                               k.pop("nbest", 3), **k),
                lambda *a, **k: crit.beam_decode_graph_nbest_confidence(x, *a, **k))
    for f in surfaces:
        with pytest.raises(TypeError, match="TokenGraph"):
            f(None)
        with pytest.raises(RuntimeError, match="tokens"):
            f(_ngram(4, 1, 1))
        with pytest.raises(RuntimeError, match="ROCm device"):             # the arguments are checked before the device
            f(g, frame_tolerance=1, return_alignments=True)
    with pytest.raises(ValueError, match="beam_size"):
        A.beam_decode_graph_nbest_confidence(x, tr, g, beam_size=0)
    with pytest.raises(ValueError, match="beam_threshold"):
        crit.beam_decode_graph_nbest_confidence(x, g, beam_threshold=-1.0)
    with pytest.raises(ValueError, match="nbest"):
        A.beam_decode_graph_nbest_confidence(x, tr, g, nbest=0)
    with pytest.raises(ValueError, match="nbest"):
        crit.beam_decode_graph_nbest_confidence(x, g, nbest=0)
    for name in ("BeamNbestConfidence", "beam_decode_graph_nbest_confidence"):
        assert name in A.__all__ and hasattr(A, name)
    assert A.BeamNbestConfidence._fields == A.BeamNbest._fields + ("token_frames", "token_confidences", "normalisers") == FIELDS
    assert tuple(EIGHT) == A.BeamNbest._fields
