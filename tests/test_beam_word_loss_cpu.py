"""CPU tests that pin the numpy restatement of the beam-pruned loss over pairs (tests/beam_word_loss_ref.py) before the GPU
tests compare the kernels with it: Z_K against the enumeration of every label path, its gradients against central differences
with the sets frozen, the whole beam against tests/beam_loss_ref.py and tests/graph_loss_ref.py on the static composition, the
inequalities of the specification, the forced-pair walk against an independent scorer, and the C ABI of asg_beam_words_full_* and
asg_words_target_scores (symbols, sizes, argument checks) -- no kernel is launched here."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from beam_loss_ref import beam_loss_ref
from beam_word_cases import arpa_lm, compose_static, eighths, path_score_words, small_lexicon, without_unigrams
from beam_word_loss_ref import beam_word_loss_ref, forced_sets, lattice_sets, word_model, words_target_scores_ref
from graph_loss_ref import full_graph_ref

INF = float("inf")
KW = dict(lm_weight=0.7, word_score=-0.4, token_score=0.3)
TARGET = [0, 1, 4, 2, 4]                                  # words 1 ("0 1") and 3 ("2") of small_lexicon, each closed


def _emissions(T, B, N, seed, dt=np.float64, grid=None):
    rng = np.random.default_rng(seed)
    if grid:
        return (rng.integers(-4 * grid, 4 * grid, (T, B, N)) / grid).astype(dt), (rng.integers(-2 * grid, 2 * grid, (N, N)) / grid).astype(dt)
    return rng.normal(size=(T, B, N)).astype(dt), rng.normal(size=(N, N)).astype(dt)


def _lse(v):
    v = np.asarray([a for a in v if a > -np.inf], np.float64)
    if v.size == 0:
        return -np.inf
    return v.max() + np.log(np.exp(v - v.max()).sum())


def _pair_seq(m, labels):
    """The pair of every frame of a label path, None if the lexicon or the LM rejects it on the way."""
    l0 = int(labels[0])
    start = [q for q in range(m.Q) if m.start_w[q] > -np.inf and m.label[q] == l0]
    if not start:
        return None
    p = (int(m.lm.start), start[0])
    seq = [p]
    for t in range(1, len(labels)):
        i = int(labels[t])
        if i != int(labels[t - 1]):
            nxt = [p2 for p2, _, lab in m.edges(p)[1:] if lab == i]
            if not nxt:
                return None
            p = nxt[0]
        seq.append(p)
    return seq


@pytest.mark.parametrize("order", [2, 3])
def test_z_is_lse_over_exactly_the_paths_inside_the_sets(order):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = without_unigrams(arpa_lm(5, order, 3 + order), {2})
    T = 5
    x, tr = _emissions(T, 1, 5, 31 + order)
    m = word_model(lex, lm, np.float64, **KW)
    scored = []
    for labels in itertools.product(range(5), repeat=T):
        s = path_score_words(x[:, 0], tr, lex, lm, labels, **KW)
        if s > -np.inf:
            scored.append((s, _pair_seq(m, labels)))
    assert len(scored) > 20 and all(seq is not None for _, seq in scored)
    whole = _lse([s for s, _ in scored])
    Z, _, _, U = beam_word_loss_ref(x, tr, lex, lm, None, 10_000, INF, **KW)
    assert np.allclose(Z[0], whole, rtol=1e-9, atol=1e-9)
    tg = np.array([TARGET])
    pruned = 0
    for K in (1, 2, 3, 8):
        for targets in (None, tg):
            Z, _, _, U = beam_word_loss_ref(x, tr, lex, lm, None, K, INF, targets=targets, **KW)
            sets = [set(u) for u in U[0]]
            inside = [s for s, seq in scored if all(p in sets[t] for t, p in enumerate(seq))]
            pruned += len(inside) < len(scored)
            assert np.allclose(Z[0], _lse(inside), rtol=1e-9, atol=1e-9), (K, targets is not None)
    assert pruned >= 6


def test_gradients_match_central_differences_with_the_sets_frozen():
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 2, 9)
    T, B, N = 6, 2, 5
    x, tr = _emissions(T, B, N, 41)
    il = np.array([6, 4])
    tg = np.array([TARGET, [2, 4, 2, 4, 0]])
    tl = np.array([5, 3])
    gs = np.array([0.7, -1.3])
    sets = lattice_sets(x, tr, lex, lm, il, 3, INF, targets=tg, target_lengths=tl, **KW)
    Z, gx, gtr, _ = beam_word_loss_ref(x, tr, lex, lm, il, 3, INF, targets=tg, target_lengths=tl, grad_scores=gs, sets=sets, **KW)
    assert np.isfinite(Z).all()
    f = lambda x_, tr_: float((gs * beam_word_loss_ref(x_, tr_, lex, lm, il, 3, INF, sets=sets, **KW)[0]).sum())    # noqa: E731
    eps = 1e-6
    rng = np.random.default_rng(0)
    for _ in range(25):
        t, b, i = rng.integers(T), rng.integers(B), rng.integers(N)
        d = np.zeros_like(x)
        d[t, b, i] = eps
        assert abs((f(x + d, tr) - f(x - d, tr)) / (2 * eps) - gx[t, b, i]) < 1e-7
    for i in range(N):
        for j in range(N):
            d = np.zeros_like(tr)
            d[i, j] = eps
            assert abs((f(x, tr + d) - f(x, tr - d)) / (2 * eps) - gtr[i, j]) < 1e-7
    assert (gx[4:, 1] == 0).all() and np.allclose(gx[:4, 1].sum(axis=1), gs[1]) and np.allclose(gx[:, 0].sum(axis=1), gs[0])


@pytest.mark.parametrize("order", [2, 3])
def test_whole_beam_in_eighths_equals_the_static_composition(order):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = without_unigrams(eighths(arpa_lm(5, order, 40 + order)), {3})
    nxt, wt, fin, start = compose_static(lex, lm)
    x, tr = _emissions(7, 4, 5, 23, grid=8)
    il = np.array([7, 4, 1, 0])
    gs = np.array([1.0, -0.5, 2.0, 3.0])
    Z, gx, gtr, _ = beam_word_loss_ref(x, tr, lex, lm, il, 10_000, INF, token_score=0.125, grad_scores=gs)
    Zf, gxf, gtrf = full_graph_ref(x, tr, nxt, wt, fin, start, il, 1.0, 0.125, grad_scores=gs)
    assert np.isfinite(Z[:3]).all() and Z[3] == -np.inf
    assert np.allclose(Z[:3], Zf[:3], rtol=1e-9, atol=1e-9) and Zf[3] == -np.inf
    assert np.allclose(gx, gxf, rtol=1e-9, atol=1e-9) and np.allclose(gtr, gtrf, rtol=1e-9, atol=1e-9)
    # a pruned beam: the same sets on both sides (tests/test_beam_word_cpu.py pins that), so the same Z_K
    for K, th in ((2, INF), (8, 2.0)):
        Z, gx, gtr, _ = beam_word_loss_ref(x, tr, lex, lm, il, K, th, token_score=0.125, grad_scores=gs)
        Zs, gxs, gtrs, _ = beam_loss_ref(x, tr, nxt, wt, fin, start, il, K, th, 1.0, 0.125, grad_scores=gs)
        ok = np.isfinite(Zs)
        assert np.array_equal(ok, np.isfinite(Z)) and np.allclose(Z[ok], Zs[ok], rtol=1e-9, atol=1e-9)
        assert np.allclose(gx, gxs, rtol=1e-9, atol=1e-9) and np.allclose(gtr, gtrs, rtol=1e-9, atol=1e-9)


def _aligned(x, tr, y):
    """lse over every alignment of the merged target y (ASG force-aligned score), float64."""
    T, n = x.shape[0], len(y)
    a = np.full(n, -np.inf)
    a[0] = x[0, y[0]]
    for t in range(1, T):
        b = np.full(n, -np.inf)
        for k in range(n):
            c = [a[k] + tr[y[k], y[k]]] + ([a[k - 1] + tr[y[k], y[k - 1]]] if k else [])
            b[k] = _lse(c) + x[t, y[k]]
        a = b
    return a[n - 1]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_inequalities_of_the_specification(dt):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 3, 7)
    T, B = 7, 3
    x, tr = _emissions(T, B, 5, 51, dt)
    il = np.array([7, 6, 5])
    tg = np.array([TARGET, [2, 4, 1, 0, 4], [0, 4, 0, 0, 0]])
    tl = np.array([5, 5, 2])
    walk = words_target_scores_ref(lex, lm, tg, tl, dt, **KW)
    assert np.isfinite(walk).all()
    for K in (1, 2, 3, 8, 10_000):
        for th in (INF, 2.0, 0.0):
            info = {}
            Z, _, _, _ = beam_word_loss_ref(x, tr, lex, lm, il, K, th, info=info, **KW)
            assert (Z >= info["decode"]["scores"].astype(np.float64) - 1e-5).all()
            Zt, _, _, _ = beam_word_loss_ref(x, tr, lex, lm, il, K, th, targets=tg, target_lengths=tl, **KW)
            for b in range(B):
                y = [int(v) for k, v in enumerate(tg[b, :tl[b]]) if k == 0 or v != tg[b, k - 1]]
                loss = Zt[b] - (_aligned(x[:il[b], b].astype(np.float64), tr.astype(np.float64), y) + walk[b])
                assert loss >= -1e-9 and Zt[b] >= Z[b] - 1e-12, (K, th, b)


def test_the_forced_walk_against_the_path_scorer():
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = without_unigrams(arpa_lm(5, 2, 5), {4})
    zero_x, zero_tr = np.zeros((8, 5)), np.zeros((5, 5))
    cases = [TARGET, [0, 1, 2], [1, 0, 4, 0, 4, 0, 1], [2, 4, 2, 4], [0, 1, 2, 4], [0, 0, 1, 1, 4], [1, 4], [0, 1], [3, 4], [4],
             [0, 1, 2, 4, 4]]
    S = max(len(c) for c in cases)
    tg = np.zeros((len(cases), S), np.int64)
    for b, c in enumerate(cases):
        tg[b, :len(c)] = c
    tl = np.array([len(c) for c in cases])
    got = words_target_scores_ref(lex, lm, tg, tl, np.float64, **KW)
    m = word_model(lex, lm, np.float64, **KW)
    seen = set()
    for b, c in enumerate(cases):
        y = [v for k, v in enumerate(c) if k == 0 or v != c[k - 1]]
        want = path_score_words(zero_x[:len(y)], zero_tr, lex, lm, y, **KW)
        assert (got[b] == -np.inf) == (want == -np.inf) and (want == -np.inf or abs(got[b] - want) < 1e-12), c
        seen.add(bool(want > -np.inf))
        F = forced_sets(m, c, 8)
        if want == -np.inf:
            assert all(f == [] for f in F)
        else:
            pairs = _pair_seq(m, y)
            n = len(y)
            assert F[0] == [pairs[0]] and F[7] == [pairs[-1]]
            assert [sorted({pairs[k - 1] for k in range(1, n + 1) if k - 1 <= t and n - k <= 7 - t}) for t in range(8)] == F
    assert seen == {True, False}
    # outside labels and targets that cannot be aligned
    assert all(f == [] for f in forced_sets(m, [0, 5], 8)) and all(f == [] for f in forced_sets(m, [-1], 8))
    assert all(f == [] for f in forced_sets(m, TARGET, 4)) and all(f == [] for f in forced_sets(m, [], 4))
    bad = words_target_scores_ref(lex, lm, np.array([[0, 5], [-1, 4]]), None, np.float64)
    assert (bad == -np.inf).all()


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _abi(lex, lm, T, B, dtype=torch.float32, S=0):
    from torch_asg_amd import _lib, graph, wordlm
    c = lex.compile_words("cpu", dtype, 0.0)
    gb = graph.abi_graph_beam(c)
    w = wordlm.abi_word_lm(lm.compile("cpu", dtype, 1.0, 0.0), c)
    w.separator = lex.separator
    p = _lib.AsgProblem()
    N = lex.graph.N
    x, tr = torch.zeros(T, B, N, dtype=dtype), torch.zeros(N, N, dtype=dtype)
    tg = torch.zeros(B, max(S, 1), dtype=torch.int64)
    p.inputs, p.transition = x.data_ptr(), tr.data_ptr()
    p.T, p.B, p.N, p.S = T, B, N, max(S, 1)
    if S:
        p.targets = tg.data_ptr()
        p.targets_strides[0], p.targets_strides[1] = S, 1
    p.dtype = _lib.ASG_DTYPE_F32 if dtype == torch.float32 else _lib.ASG_DTYPE_F64
    return _lib.lib(), p, gb, w, (c, x, tr, tg)


def _refs(p, gb, w):
    return ctypes.byref(p), ctypes.byref(gb), ctypes.byref(w)


def test_byte_formulas_and_no_term_in_the_lm():
    lex = small_lexicon()
    small, big = arpa_lm(5, 2, 1), arpa_lm(5, 3, 1, keep=(1.0, 1.0, 1.0))
    assert big.H > 2 * small.H and big.A > 2 * small.A
    al = lambda n: (n + 255) // 256 * 256                                                       # noqa: E731
    for dtype, e in ((torch.float32, 4), (torch.float64, 8)):
        for T, B, K, S in ((7, 3, 16, 0), (100, 2, 300, 40), (5, 1, 8, 9)):
            L, p, gb, w, keep = _abi(lex, small, T, B, dtype, S)
            L2, p2, gb2, w2, keep2 = _abi(lex, big, T, B, dtype, S)
            dec = int(L.asg_beam_decode_words_work_bytes(*_refs(p, gb, w), K))
            nf = min(S, T)
            M = K + nf
            for store in (0, 1):
                a = int(L.asg_beam_words_full_work_bytes(*_refs(p, gb, w), K, store))
                assert a == int(L2.asg_beam_words_full_work_bytes(*_refs(p2, gb2, w2), K, store)) > 0
                assert a == B * (dec // B + 2 * al(T * 4) + 256 + al(nf * 8) + al(T * M * 8) + al((T if store else 2) * M * e))
            s = int(L.asg_beam_words_full_scratch_bytes(*_refs(p, gb, w), K))
            assert s == int(L2.asg_beam_words_full_scratch_bytes(*_refs(p2, gb2, w2), K)) == B * (al(2 * M * e) + al(25 * 8))


def test_abi_argument_checks_without_a_device():
    lex, lm = small_lexicon(), arpa_lm(5, 2, 1)
    for dtype, e in ((torch.float32, 4), (torch.float64, 8)):
        L, p, gb, w, keep = _abi(lex, lm, 7, 3, dtype, 4)
        wb = lambda K, store=1: int(L.asg_beam_words_full_work_bytes(*_refs(p, gb, w), K, store))    # noqa: E731
        sb = lambda K: int(L.asg_beam_words_full_scratch_bytes(*_refs(p, gb, w), K))                  # noqa: E731
        mmax = (160 * 1024 - 256) // (16 + e)              # the header's bound on M = K + nf, nf = 4 here
        assert mmax == (8179 if e == 4 else 6816)
        assert wb(mmax - 4) > 0 and sb(mmax - 4) > 0 and wb(mmax - 3) == 0 and sb(mmax - 3) == 0 and wb(0) == 0 and sb(0) == 0

        def fwd(K, th, work=256, nbytes=1 << 40, scores=256, flags=64):
            return L.asg_beam_words_full_forward(None, *_refs(p, gb, w), K, th, work, nbytes, scores, flags, None)

        def bwd(K, work=256, nbytes=1 << 40, sc=256, gs=256, gin=256, gtr=256, scratch=256, sbytes=1 << 40):
            return L.asg_beam_words_full_backward(None, *_refs(p, gb, w), K, work, nbytes, sc, gs, gin, gtr, scratch, sbytes, 0, None)
        assert fwd(mmax - 3, 1.0) == 2 and bwd(mmax - 3) == 2 and fwd(8193, 1.0) == 2
        assert fwd(0, 1.0) == 1 and fwd(8, -1.0) == 1 and fwd(8, float("nan")) == 1 and bwd(0) == 1
        assert fwd(8, 1.0, work=None) == 1 and fwd(8, 1.0, scores=None) == 1
        assert fwd(8, 1.0, nbytes=wb(8) - 1) == 3 and fwd(8, 1.0, nbytes=wb(8, 0) - 1, flags=0) == 3
        for name in ("work", "sc", "gs", "gin", "gtr", "scratch"):
            assert bwd(8, **{name: None}) == 1, name
        assert bwd(8, nbytes=wb(8) - 1) == 3 and bwd(8, sbytes=sb(8) - 1) == 3
        tsc = lambda out=256: L.asg_words_target_scores(None, *_refs(p, gb, w), out, None)            # noqa: E731
        assert tsc(None) == 1
        w.dtype = 1 - w.dtype
        assert fwd(8, 1.0) == 1 and bwd(8) == 1 and tsc() == 1 and wb(8) == 0
        w.dtype = 1 - w.dtype
        for field, bad in (("start", lm.H), ("separator", 5), ("H", 0), ("row", None), ("word_of_state", None)):
            old = getattr(w, field)
            setattr(w, field, bad)
            assert fwd(8, 1.0) == 1 and bwd(8) == 1 and tsc() == 1, field
            setattr(w, field, old)
        w.H = (1 << 25) + 1
        assert fwd(8, 1.0) == 2 and bwd(8) == 2 and tsc() == 2
        w.H = lm.H
        old = (p.targets, p.S)
        p.S = 0
        assert fwd(8, 1.0) == 1 and tsc() == 1              # targets with S < 1
        p.targets, p.S = None, 1
        assert tsc() == 1 and wb(8) > 0                    # the walk needs targets, the normaliser does not
        p.targets, p.S = old
        p.N = 1025
        assert fwd(8, 1.0) in (1, 2)                       # (the graph is over 5 tokens: refused either way)
        p.N = 5
        p.T = (1 << 20) + 1
        assert fwd(8, 1.0) == 2 and wb(8) == 0
        p.T = 7
    # min(S, T) with targets above 2048
    L, p, gb, w, keep = _abi(lex, lm, 2049, 1, torch.float32, 2049)
    assert int(L.asg_beam_words_full_work_bytes(*_refs(p, gb, w), 8, 1)) == 0
    assert L.asg_beam_words_full_forward(None, *_refs(p, gb, w), 8, 1.0, 256, 1 << 40, 256, 64, None) == 2
    L, p, gb, w, keep = _abi(lex, lm, 2048, 1, torch.float32, 2049)
    assert int(L.asg_beam_words_full_work_bytes(*_refs(p, gb, w), 8, 1)) > 0


def test_python_surface_refuses_bad_arguments_before_any_launch():
    import torch_asg_amd as A
    lex, lm = small_lexicon(), arpa_lm(5, 2, 1)
    x, tr = torch.zeros(4, 2, 5), torch.zeros(5, 5)
    tg = torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="beam_size"):
        A.beam_words_full_score(x, tr, lex, lm, beam_size=0)
    with pytest.raises(ValueError, match="beam_threshold"):
        A.beam_words_asg_loss(x, tg, tr, lex, lm, beam_threshold=-1.0)
    with pytest.raises(TypeError, match="Lexicon"):
        A.beam_words_full_score(x, tr, lex.graph, lm)
    with pytest.raises(TypeError, match="WordLM"):
        A.beam_words_asg_loss(x, tg, tr, lex, None)
    with pytest.raises(RuntimeError, match="knows"):
        A.beam_words_full_score(x, tr, lex, A.WordLM.null(3))
    assert hasattr(A.ASGLoss, "beam_word_loss")
    for name in ("BeamWordsFullScore", "beam_words_full_score", "beam_words_asg_loss"):
        assert name in A.__all__ and hasattr(A, name)
