"""CPU tests of Viterbi decoding with a token automaton: the test-side reference (tests/graph_decode_ref.py) against exhaustive
path enumeration and against the plain decoder, n-gram automata, the compiled product graph, and the C ABI of
asg_viterbi_decode_graph (sizes, argument checks) -- no kernel is launched here."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from decode_ref import decode_ref
from graph_decode_ref import decode_graph_ref, path_score_graph, product, fold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_automaton(rng, S, N):
    nxt = rng.integers(0, S, size=(S, N))
    nxt[rng.random(size=(S, N)) < 0.25] = -1                      # missing arcs
    w = rng.normal(size=(S, N))
    w[rng.random(size=(S, N)) < 0.1] = -np.inf                    # arcs that are there but weigh -inf: absent too
    f = rng.normal(size=S)
    f[rng.random(size=S) < 0.3] = -np.inf                         # non-accepting states
    return nxt, w, f


FOLDS = [(1.0, 0.0), (0.5, -0.3), (2.0, 1.25)]


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_against_exhaustive_enumeration(seed, dtype):
    rng = np.random.default_rng(700 + seed)
    for _ in range(12):
        T, B, N, S = int(rng.integers(1, 7)), int(rng.integers(1, 4)), int(rng.integers(2, 5)), int(rng.integers(1, 5))
        nxt, w, f = _random_automaton(rng, S, N)
        lw, ts = FOLDS[int(rng.integers(len(FOLDS)))]
        x = rng.normal(size=(T, B, N)).astype(dtype)
        tr = rng.normal(size=(N, N)).astype(dtype)
        il = rng.integers(0, T + 1, size=B)
        il[0] = T
        sc, path, tok, tl, st = decode_graph_ref(x, tr, nxt, w, f, 0, il, lw, ts)
        for b in range(B):
            L = int(il[b])
            assert (path[b, L:] == -1).all() and (st[b, L:] == -1).all()
            if L == 0:
                assert sc[b] == -np.inf and (path[b] == -1).all() and tl[b] == 0
                continue
            best, arg = -np.inf, []
            for p in itertools.product(range(N), repeat=L):
                s, _ = path_score_graph(x[:, b], tr, nxt, w, f, p, 0, lw, ts)
                if s > best:
                    best, arg = s, [p]
                elif s == best and s > -np.inf:
                    arg.append(p)
            if best == -np.inf:
                assert sc[b] == -np.inf and (path[b] == -1).all() and (tok[b] == -1).all() and tl[b] == 0
                assert (st[b] == -1).all()
                continue
            assert sc[b] == best
            p = tuple(int(v) for v in path[b, :L])
            assert p in arg
            s, sts = path_score_graph(x[:, b], tr, nxt, w, f, p, 0, lw, ts)
            assert s == sc[b] and list(st[b, :L]) == sts
            c = [v for i, v in enumerate(p) if i == 0 or p[i - 1] != v]
            assert tl[b] == len(c) and list(tok[b, :len(c)]) == c and (tok[b, len(c):] == -1).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("N", [1, 2, 5, 40])
def test_one_state_reference_equals_the_plain_decoder(N, dtype):
    rng = np.random.default_rng(N)
    T, B = 30, 4
    x = rng.normal(size=(T, B, N)).astype(dtype)
    tr = rng.normal(size=(N, N)).astype(dtype)
    il = np.array([T, 0, 1, 17])
    got = decode_graph_ref(x, tr, np.zeros((1, N), np.int64), np.zeros((1, N)), np.zeros(1), 0, il)
    want = decode_ref(x, tr, il)
    for g, r in zip(got[:4], want):
        assert np.array_equal(g, r)
    assert (got[4][il[:, None] > np.arange(T)[None, :]] == 0).all()


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_from_ngram_walks_reproduce_the_table(order):
    from torch_asg_amd import TokenGraph
    rng = np.random.default_rng(order)
    N = 3
    lp = rng.normal(size=(N + 1,) * order)
    g = TokenGraph.from_ngram(lp)
    assert g.S == sum(N ** k for k in range(order)) and g.N == N and g.start == 0
    for _ in range(20):
        seq = rng.integers(0, N, size=int(rng.integers(0, 8)))
        s, total = g.start, 0.0
        ctx, want = (N,) * (order - 1), 0.0
        for tk in seq:
            assert g.next[s, tk] >= 0
            total += g.weight[s, tk]
            s = g.next[s, tk]
            want += lp[ctx + (tk,)]
            ctx = (ctx + (int(tk),))[1:]
        total += g.final[s]
        want += lp[ctx + (N,)]
        assert total == want


def test_from_ngram_rejects_bad_tables():
    from torch_asg_amd import TokenGraph
    with pytest.raises(ValueError):
        TokenGraph.from_ngram(np.zeros((4, 4, 4, 4, 4)))
    with pytest.raises(ValueError):
        TokenGraph.from_ngram(np.zeros((4, 3)))
    with pytest.raises(ValueError):
        TokenGraph.from_ngram(np.full((3, 3), np.nan))


def test_token_graph_validation():
    from torch_asg_amd import TokenGraph
    nxt, w, f = np.zeros((2, 3), np.int64), np.zeros((2, 3)), np.zeros(2)
    TokenGraph(nxt, w, f, start=1)
    TokenGraph(torch.from_numpy(nxt), torch.from_numpy(w), torch.from_numpy(f))
    bad = [(nxt[:, :2], w, f, 0), (nxt, w[:1], f, 0), (nxt, w, f[:1], 0), (nxt + 2, w, f, 0), (nxt - 2, w, f, 0),
           (nxt, np.where(nxt == 0, np.nan, 0.0), f, 0), (nxt, w, np.array([0.0, np.nan]), 0), (nxt, w + np.inf, f, 0),
           (nxt, w, f, 2), (nxt, w, f, -1), (np.zeros(3, np.int64), w, f, 0)]
    for args in bad:
        with pytest.raises(ValueError):
            TokenGraph(*args[:3], start=args[3])


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_compiled_graph_invariants(seed, dt):
    from torch_asg_amd import TokenGraph
    rng = np.random.default_rng(40 + seed)
    S, N = int(rng.integers(1, 12)), int(rng.integers(1, 9))
    nxt, w, f = _random_automaton(rng, S, N)
    g = TokenGraph(nxt, w, f, start=int(rng.integers(S)))
    lw, ts = FOLDS[seed % len(FOLDS)]
    c = g.compile_host(dt, lw, ts)
    Q, E = c["Q"], c["E"]
    label, state, row, src = c["label"], c["state"], c["row"], c["src"]
    assert all(a.dtype == np.int32 for a in (label, state, row, src, c["src_label"]))
    assert all(c[k].dtype == dt for k in ("start_w", "final_w", "edge_w"))
    key = state.astype(np.int64) * N + label
    assert (np.diff(key) > 0).all()                                     # Q sorted by (s', i), no duplicates
    assert row[0] == 0 and row[-1] == E and (np.diff(row) >= 0).all()
    for q in range(Q):
        r = src[row[q]:row[q + 1]]
        assert (np.diff(r) > 0).all()                                   # each CSR row strictly ascending
        assert (label[r] != label[q]).all()                             # no j == i edge
    assert (c["src_label"] == label[src]).all()
    # the same product graph as the reference enumerates from the sources, and the same folded weights
    present, arcw, finw = fold(nxt, w, f, dt, lw, ts)
    rl, rs, rsrc, rtgt, rQ = product(nxt, present)
    tgt = np.repeat(np.arange(Q), np.diff(row))
    assert rQ == Q and (rl == label).all() and (rs == state).all() and (rsrc == src).all() and (rtgt == tgt).all()
    assert np.array_equal(c["edge_w"], arcw[state[src], label[tgt]])
    assert np.array_equal(c["final_w"], finw[state])
    s0 = g.start
    want = np.where(present[s0, label] & (nxt[s0, label] == state), arcw[s0, label], -np.inf).astype(dt)
    assert np.array_equal(c["start_w"], want)


def test_compile_is_cached_per_device_dtype_and_weights():
    from torch_asg_amd import TokenGraph
    g = TokenGraph.from_ngram(np.zeros((4, 4)))
    a = g.compile("cpu", torch.float32, 1.0, 0.0)
    assert g.compile("cpu", torch.float32, 1.0, 0.0) is a
    assert g.compile("cpu", torch.float64, 1.0, 0.0) is not a
    assert g.compile("cpu", torch.float32, 0.5, 0.0) is not a
    assert g.compile("cpu", torch.float32, 1.0, 0.5) is not a
    assert a["Q"] == 3 and a["E"] == 6 and a["label"].dtype == torch.int32
    with pytest.raises(ValueError):
        g.compile("cpu", torch.float32, float("nan"), 0.0)


# ---- the C ABI: no kernel is launched -------------------------------------------------------------------------------------
def test_header_and_library_declare_and_export_the_graph_decoder():
    from torch_asg_amd import _lib
    names = {"asg_viterbi_decode_graph", "asg_viterbi_decode_graph_work_bytes"}
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(L, n) for n in names) and names <= set(_lib.SYMBOLS)
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    assert "#define ASG_FLAG_DECODE_GRAPH_STREAMING 16" in src and _lib.FLAG_DECODE_GRAPH_STREAMING == 16


def _problem(T, B, N, dtype):
    from torch_asg_amd import _lib
    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.S = T, B, N, 0
    p.dtype = dtype
    p.inputs, p.transition = 16, 16          # never dereferenced: only sizes / checks
    return p


def _graph(Q, E, N, dtype):
    from torch_asg_amd import _lib
    g = _lib.AsgTokenGraph()
    g.Q, g.E, g.N, g.dtype = Q, E, N, dtype
    for name in ("label", "state", "row", "src", "src_label", "start_w", "final_w", "edge_w"):
        setattr(g, name, 16)
    return g


@pytest.mark.parametrize("T,B,Q", [(400, 64, 40), (7, 3, 1), (400, 64, 1641), (400, 64, 65641), (5, 1, 0)])
def test_graph_work_bytes_follow_the_documented_formula(T, B, Q):
    from torch_asg_amd import _lib
    L = _lib.lib()
    for dt, e in ((_lib.ASG_DTYPE_F32, 4), (_lib.ASG_DTYPE_F64, 8)):
        p, g = _problem(T, B, 40, dt), _graph(Q, 40 * Q, 40, dt)
        want = (T * B * Q * 4 + 255) // 256 * 256 + 2 * Q * B * e
        assert L.asg_viterbi_decode_graph_work_bytes(ctypes.byref(p), ctypes.byref(g)) == want


def test_graph_decode_argument_validation():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32, F64 = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64
    p, g = _problem(10, 2, 40, F32), _graph(40, 1560, 40, F32)
    wb = L.asg_viterbi_decode_graph_work_bytes
    dec = L.asg_viterbi_decode_graph
    assert wb(None, None) == 0 and wb(ctypes.byref(p), None) == 0
    assert dec(None, None, None, None, 0, None, None, None, None, None, 0, None) == 1
    need = wb(ctypes.byref(p), ctypes.byref(g))
    assert need == (10 * 2 * 40 * 4 + 255) // 256 * 256 + 2 * 40 * 2 * 4
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.addressof(buf)
    pp, gp = ctypes.byref(p), ctypes.byref(g)
    assert dec(None, pp, None, None, 1 << 12, a, a, a, a, a, 0, None) == 1            # null graph
    # null work / outputs
    for k in range(6):
        args = [a] * 6
        args[k] = None
        assert dec(None, pp, gp, args[0], 1 << 12, *args[1:], 0, None) == 1
    assert dec(None, pp, gp, a, need - 1, a, a, a, a, a, 0, None) == 3                 # a workspace one byte short
    # null graph arrays
    for name in ("label", "state", "row", "src", "src_label", "start_w", "final_w", "edge_w"):
        h = _graph(40, 1560, 40, F32)
        setattr(h, name, None)
        assert wb(pp, ctypes.byref(h)) == 0
        assert dec(None, pp, ctypes.byref(h), a, 1 << 12, a, a, a, a, a, 0, None) == 1
    # dtype: bad, or not the problem's; N not the problem's; negative sizes
    for Q, E, N, dt in ((40, 1560, 40, 7), (40, 1560, 40, F64), (40, 1560, 39, F32), (-1, 0, 40, F32), (40, -1, 40, F32)):
        h = _graph(Q, E, N, dt)
        assert wb(pp, ctypes.byref(h)) == 0
        assert dec(None, pp, ctypes.byref(h), a, 1 << 12, a, a, a, a, a, 0, None) == 1
    q = _problem(10, 2, 40, 7)
    assert dec(None, ctypes.byref(q), gp, a, 1 << 12, a, a, a, a, a, 0, None) == 1
    q = _problem(0, 2, 40, F32)
    assert dec(None, ctypes.byref(q), gp, a, 1 << 12, a, a, a, a, a, 0, None) == 1
    # limits: Q, E < 2^31, N <= 2^16, B <= 2^22
    for Q, E in (((1 << 31), 0), (40, (1 << 31))):
        h = _graph(Q, E, 40, F32)
        assert wb(pp, ctypes.byref(h)) == 0
        assert dec(None, pp, ctypes.byref(h), a, 1 << 12, a, a, a, a, a, 0, None) == 2
    q, h = _problem(10, 2, (1 << 16) + 1, F32), _graph(40, 1560, (1 << 16) + 1, F32)
    assert dec(None, ctypes.byref(q), ctypes.byref(h), a, 1 << 12, a, a, a, a, a, 0, None) == 2
    q = _problem(10, (1 << 22) + 1, 40, F32)
    assert dec(None, ctypes.byref(q), gp, a, 1 << 12, a, a, a, a, a, 0, None) == 2
