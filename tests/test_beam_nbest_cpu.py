"""CPU tests that pin the test-side reference of the n-best beam decoder (tests/beam_nbest_ref.py): its hypotheses against
exhaustive path enumeration, its first row against tests/beam_decode_ref.py, the bound between the score and the sum of its
two parts, and the C ABI of asg_beam_decode_graph_nbest (symbols, sizes, argument checks) -- no kernel is launched here."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from beam_decode_ref import beam_decode_ref
from beam_nbest_ref import beam_nbest_ref
from graph_decode_ref import fold, product

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("asg_beam_decode_graph_nbest_work_bytes", "asg_beam_decode_graph_nbest")


def _random_automaton(rng, S, N):
    nxt = rng.integers(0, S, size=(S, N))
    nxt[rng.random(size=(S, N)) < 0.2] = -1
    w = rng.normal(size=(S, N))
    f = rng.normal(size=S)
    f[rng.random(size=S) < 0.3] = -np.inf
    return nxt, w, f


def _ngram(rng, N, order, holes=False):
    import torch_asg_amd
    lp = np.log(rng.dirichlet(np.ones(N + 1), size=(N + 1,) * (order - 1))) if order > 1 else np.log(rng.dirichlet(np.ones(N + 1)))
    if holes:
        lp[rng.random(size=lp.shape) < 0.2] = -np.inf
    g = torch_asg_amd.TokenGraph.from_ngram(lp)
    return g.next, g.weight, g.final


def _enumerate(xb, tr, nxt, w, f, start, lw, ts):
    """Every label path of one utterance through the composed lattice -> {(label, state) at the last frame: the best
    (end, labels, states, emission part, graph part)}.  A path's sums are formed in the order the specification gives."""
    T, N = xb.shape
    dt = xb.dtype.type
    present, arcw, finw = fold(nxt, w, f, dt, lw, ts)
    best = {}
    for labels in itertools.product(range(N), repeat=T):
        i = labels[0]
        if not present[start, i]:
            continue
        s = int(nxt[start, i])
        v = arcw[start, i] + xb[0, i]
        a, g = xb[0, i], arcw[start, i]
        sts, ok = [s], True
        for t in range(1, T):
            i, j = labels[t], labels[t - 1]
            a = (a + tr[i, j]) + xb[t, i]
            if i == j:
                v = (v + tr[i, i]) + xb[t, i]
            else:
                if not present[s, i]:
                    ok = False
                    break
                v = ((v + tr[i, j]) + arcw[s, i]) + xb[t, i]
                g = g + arcw[s, i]
                s = int(nxt[s, i])
            sts.append(s)
        if not ok:
            continue
        end = v + finw[s]
        g = g + finw[s]
        if not end > -np.inf:
            continue
        key = (labels[-1], s)
        if key not in best or end > best[key][0]:
            best[key] = (end, labels, sts, a, g)
    return best


@pytest.mark.parametrize("kind", ["bigram", "random"])
@pytest.mark.parametrize("seed", range(3))
def test_hypotheses_equal_exhaustive_enumeration(seed, kind):
    rng = np.random.default_rng(300 + seed)
    N, T, B = 3, 4, 3
    nxt, w, f = _ngram(rng, N, 2) if kind == "bigram" else _random_automaton(rng, 5, N)
    nxt = np.asarray(nxt, np.int64)
    x = rng.normal(size=(T, B, N))
    tr = rng.normal(size=(N, N))
    lw, ts = 0.8, -0.3
    present, _, _ = fold(nxt, w, f, np.float64, lw, ts)
    label, state, _, _, Q = product(nxt, present)
    number = {(int(i), int(s)): q for q, (i, s) in enumerate(zip(label, state))}
    nbest = Q + 3
    sc, em, gr, tok, tl, nh, path, st = beam_nbest_ref(x, tr, nxt, w, f, 0, None, Q + 1, nbest, np.inf, lw, ts)
    seen = 0
    for b in range(B):
        best = _enumerate(x[:, b], tr, nxt, w, f, 0, lw, ts)
        ranked = sorted(best.items(), key=lambda kv: (-kv[1][0], number[kv[0]]))
        assert nh[b] == len(ranked) <= Q
        seen += len(ranked)
        for r, (_, (end, labels, sts, a, g)) in enumerate(ranked):
            assert sc[b, r] == end and em[b, r] == a and gr[b, r] == g          # the same additions in the same order
            assert path[b, r].tolist() == list(labels) and st[b, r].tolist() == sts
            toks = [k for k, _ in itertools.groupby(labels)]
            assert tl[b, r] == len(toks) and tok[b, r, :len(toks)].tolist() == toks and (tok[b, r, len(toks):] == -1).all()
        pad = slice(int(nh[b]), nbest)
        assert (sc[b, pad] == -np.inf).all() and (em[b, pad] == -np.inf).all() and (gr[b, pad] == -np.inf).all()
        assert (tok[b, pad] == -1).all() and (path[b, pad] == -1).all() and (st[b, pad] == -1).all() and (tl[b, pad] == 0).all()
    assert seen > B                                                             # more than one hypothesis somewhere


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("seed", range(4))
def test_row_0_equals_beam_decode_ref(seed, dt):
    rng = np.random.default_rng(400 + seed)
    N = int(rng.integers(3, 8))
    nxt, w, f = _ngram(rng, N, 2 + seed % 2, holes=bool(seed & 1)) if seed < 2 else _random_automaton(rng, 6, N)
    T, B = 9, 4
    x = rng.normal(size=(T, B, N)).astype(dt)
    tr = rng.normal(size=(N, N)).astype(dt)
    il = np.array([T, 0, 1, 6])
    for K, th in ((1, np.inf), (3, np.inf), (5, 1.5), (1000, np.inf), (4, 0.0), (6, 3.0)):
        s1, s2 = [], []
        want = beam_decode_ref(x, tr, nxt, w, f, 0, il, K, th, 0.8, 0.1, sizes=s1)
        for nbest in (1, 4):
            sc, em, gr, tok, tl, nh, path, st = beam_nbest_ref(x, tr, nxt, w, f, 0, il, K, nbest, th, 0.8, 0.1, sizes=s2)
            for name, got, ref in zip(("scores", "path", "tokens", "token_lengths", "states"),
                                      (sc[:, 0], path[:, 0], tok[:, 0], tl[:, 0], st[:, 0]), want):
                assert got.dtype == ref.dtype and np.array_equal(got, ref), (name, K, th, nbest)
            assert np.array_equal(nh > 0, want[0] > -np.inf)
        assert [s for s in s2 if s][:len(s1)] == s1                       # the same active sets, frame by frame


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_score_is_the_sum_of_its_parts_to_rounding(dt):
    """scores adds the path's terms in the search's order, emission_scores and graph_scores add the same n <= 3*len terms in
    another.  A sequential sum of n terms lies within (n - 1) * u * sum|terms| of the exact sum to first order, u = eps / 2
    (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), so the two differ by at most (n - 1) * eps * sum|terms|;
    the (3*len + 2) of the specification leaves room for the addition that joins the parts and for the second-order terms."""
    rng = np.random.default_rng(500)
    eps = np.finfo(dt).eps
    checked = 0
    for nxt, w, f, N in [(*_ngram(rng, 6, 3, holes=True), 6), (*_random_automaton(rng, 8, 5), 5)]:
        T, B = 40, 4
        x = (3.0 * rng.normal(size=(T, B, N))).astype(dt)
        tr = rng.normal(size=(N, N)).astype(dt)
        il = np.array([T, 1, 17, 0])
        terms = {}
        sc, em, gr, _, _, nh, _, _ = beam_nbest_ref(x, tr, nxt, w, f, 0, il, 12, 12, np.inf, 1.3, 0.25, terms=terms)
        for b in range(B):
            for r in range(int(nh[b])):
                mag = float(np.sum(np.abs(np.asarray(terms[(b, r)], np.float64))))
                assert len(terms[(b, r)]) <= 3 * il[b]
                assert abs(float(sc[b, r]) - (float(em[b, r]) + float(gr[b, r]))) <= (3 * il[b] + 2) * eps * mag
                checked += 1
    assert checked > 20


def test_abi_declares_and_exports_the_nbest_entry_points():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    import torch_asg_amd
    assert hasattr(torch_asg_amd, "beam_decode_graph_nbest") and hasattr(torch_asg_amd.ASGLoss, "beam_decode_graph_nbest")
    assert torch_asg_amd.BeamNbest._fields == ("scores", "emission_scores", "graph_scores", "tokens", "token_lengths", "num_hyps",
                                               "path", "states")
    assert L.asg_hip_version() == 230


def _host_view(graph, dt, T, B):
    """An asg_token_graph_beam over HOST arrays (sizes and validation read no array) and a problem."""
    from torch_asg_amd import _lib
    h = graph.compile_host(dt)
    hb = graph.compile_beam_host(dt)
    keep = [h, hb]
    g = _lib.AsgTokenGraph()
    g.Q, g.E, g.N = h["Q"], h["E"], graph.N
    g.dtype = _lib.ASG_DTYPE_F32 if dt == np.float32 else _lib.ASG_DTYPE_F64
    for n in ("label", "state", "row", "src", "src_label", "start_w", "final_w", "edge_w"):
        setattr(g, n, h[n].ctypes.data)
    gb = _lib.AsgTokenGraphBeam()
    gb.graph = ctypes.pointer(g)
    gb.num_start, gb.max_out = hb["num_start"], hb["max_out"]
    for n in ("orow", "oarc", "ow", "start_q"):
        setattr(gb, n, hb[n].ctypes.data)
    p = _lib.AsgProblem()
    dummy = np.zeros(8, dt)
    keep += [dummy, g]
    p.inputs, p.transition = dummy.ctypes.data, dummy.ctypes.data
    p.T, p.B, p.N, p.S, p.dtype = T, B, graph.N, 1, g.dtype
    return p, gb, keep


def _a256(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_sizes_and_argument_validation_without_gpu(dt):
    import torch_asg_amd
    from torch_asg_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(0)
    graph = torch_asg_amd.TokenGraph(*_ngram(rng, 6, 3))
    T, B, e = 50, 4, np.dtype(dt).itemsize
    p, gb, keep = _host_view(graph, dt, T, B)
    Q = graph.compile_host(dt)["Q"]
    wb, search = L.asg_beam_decode_graph_nbest_work_bytes, L.asg_beam_decode_graph_work_bytes
    P, G = ctypes.byref(p), ctypes.byref(gb)
    # the formula of include/asg_hip.h
    for beam, nbest in ((8, 1), (8, 5), (8, 8), (8, 100), (1000, 7), (1000, 8192), (1, 3)):
        K = min(beam, Q)
        nb = min(nbest, K)
        p.B = 1
        per = search(P, G, beam)
        p.B = B
        assert search(P, G, beam) == B * per
        want = B * (per + _a256(8 + K * e) + _a256(T * nb * 4)) + 2 * _a256(B * 8) + _a256(3 * B * T * 8)
        assert wb(P, G, beam, nbest) == want, (beam, nbest)
    assert wb(P, G, 8, 0) == 0 and wb(P, G, 8, -3) == 0 and wb(P, G, 8, 8193) == 0 and wb(P, G, 0, 4) == 0
    assert wb(P, G, 8192, 8192) > 0                                     # nbest = 8192 is accepted
    f = L.asg_beam_decode_graph_nbest
    one = ctypes.c_void_p(1)
    big = 1 << 40

    def call(beam=8, theta=1.0, nbest=4, gbp=G, work=one, nbytes=big, sc=one, em=one, gr=one, path=one, tok=one, tl=one,
             st=one, nh=one):
        return f(None, P, gbp, beam, theta, nbest, work, nbytes, sc, em, gr, path, tok, tl, st, nh, 0, None)
    assert call(nbest=0) == 1 and call(nbest=-1) == 1                   # ASG_ERR_INVALID
    assert call(nbest=8193) == 2                                        # ASG_ERR_UNSUPPORTED
    assert call(beam=0) == 1 and call(theta=-1.0) == 1 and call(theta=float("nan")) == 1 and call(gbp=None) == 1
    for missing in ("work", "sc", "em", "gr", "tok", "tl", "nh"):
        assert call(**{missing: None}) == 1
    a = wb(P, G, 8, 4)
    assert call(nbytes=a - 1) == 3                                      # ASG_ERR_WORKSPACE
    assert call(nbytes=a - 1, path=None, st=None) == 3                  # path and states may be NULL: past the argument checks
    assert call(nbest=8192, nbytes=0) == 3                              # nbest = 8192 passes validation
    g4 = torch_asg_amd.TokenGraph(*_ngram(rng, 21, 4))                  # Q > 8192: beam_size above the limit
    p2, gb2, keep2 = _host_view(g4, dt, 5, 1)
    assert g4.compile_host(dt)["Q"] > 8192
    assert f(None, ctypes.byref(p2), ctypes.byref(gb2), 10000, 1.0, 4, one, big, one, one, one, one, one, one, one, one, 0,
             None) == 2
    assert wb(ctypes.byref(p2), ctypes.byref(gb2), 8192, 8192) > 0
