"""CPU tests of the beam-pruned loss over the pairs a LOOK-AHEAD search keeps (`beam_words_full_score(..., lookahead=)`,
`beam_words_asg_loss(..., lookahead=)`, `ASGLoss.beam_word_loss(..., lookahead=)`,
include/asg_hip.h::asg_beam_words_full_forward_la).  They pin the numpy restatement (tests/beam_word_la_loss_ref.py) before the
GPU tests compare the kernels with it: the inequalities of the specification on the grid of the plain loss, the whole beam
against the plain restatement bit for bit, that every pruned setting of the grid separates the two losses, the gradients against
central differences with the sets frozen, the case the look-ahead is for, what dead-end nodes change (nothing but the sets), and
the C entry point's and the Python surface's argument checks -- no kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, eighths, small_lexicon
from beam_word_la_loss_ref import beam_word_la_loss_ref, la_lattice_sets
from beam_word_loss_ref import beam_word_loss_ref, lattice_sets, words_target_scores_ref
from beam_word_ref import beam_word_ref
from test_beam_word_la_cpu import hand_case, rescue_case
from test_beam_word_loss_cpu import _abi, _aligned, _refs
from test_hip_beam_word_loss import W, grid_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
ALL = 1024                                                 # more than every pair of the small cases
PRUNED = [(K, th) for K in (1, 2, 3, 8) for th in (INF, 2.0)] + [(ALL, 2.0)]
GS = np.array([1.0, -0.5, 2.0, 3.0])


def _grid(lm_order):
    lex, lm, x, tr, il, tg, tl = grid_case(lm_order, torch.float64)
    return lex, lm, x.numpy(), tr.numpy(), il.numpy(), tg.numpy(), tl.numpy()


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("lm_order", [2, 3], ids=["bigram", "trigram"])
def test_grid_losses_are_nonnegative_whole_beam_is_the_plain_loss_and_pruned_settings_separate(lm_order, order):
    lex, lm, x, tr, il, tg, tl = _grid(lm_order)
    walk = words_target_scores_ref(lex, lm, tg, tl, np.float64, *W)
    merged = [[int(v) for k, v in enumerate(tg[b, :tl[b]]) if k == 0 or v != tg[b, k - 1]] for b in range(4)]
    aligned = np.array([_aligned(x[:il[b], b], tr, merged[b]) if 0 < len(merged[b]) <= il[b] else -np.inf for b in range(4)])
    assert np.isfinite(walk[:3]).all() and np.isfinite(aligned[:3]).all()
    gaps = []
    for targets, lengths in ((None, None), (tg, tl)):
        for K, th in PRUNED + [(ALL, INF)]:
            Z, gx, gtr, U = beam_word_la_loss_ref(x, tr, lex, lm, order, il, K, th, *W, targets, lengths, GS)
            Zp, gxp, gtrp, Up = beam_word_loss_ref(x, tr, lex, lm, il, K, th, *W, targets, lengths, GS)
            assert Z[3] == -np.inf and not np.isnan(Z).any()
            if targets is not None:
                loss = Z[:3] - (aligned[:3] + walk[:3])
                assert np.isfinite(loss).all() and (loss >= -1e-9).all(), (K, th)
            if (K, th) == (ALL, INF):                      # nothing pruned, no dead end: the plain loss, bit for bit
                assert U == Up and _same(Z, Zp) and _same(gx, gxp) and _same(gtr, gtrp)
            else:                                          # the grid separates the two losses in every pruned setting
                differ = sum(u != up for Ub, Upb in zip(U, Up) for u, up in zip(Ub, Upb))
                assert differ >= 1, (K, th, targets is not None)
                gaps.append(np.abs(Z[:3] - Zp[:3]).max())
    assert max(gaps) > 0.04


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("lm_order", [2, 3], ids=["bigram", "trigram"])
def test_in_eighths_z_is_at_least_the_look_ahead_decoders_score(lm_order, order, dt):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = eighths(arpa_lm(5, lm_order, 60 + lm_order, keep=(1.0, 0.5, 0.5)))
    rng = np.random.default_rng(35)
    x, tr = (rng.integers(-32, 32, (7, 4, 5)) / 8.0).astype(dt), (rng.integers(-16, 16, (5, 5)) / 8.0).astype(dt)
    il = np.array([7, 4, 1, 0])
    w = (1.0, 0.25, 0.125)
    finite = 0
    for K, th in PRUNED + [(ALL, INF)]:
        info = {}
        Z, _, _, _ = beam_word_la_loss_ref(x, tr, lex, lm, order, il, K, th, *w, info=info)
        dec = info["decode"]["scores"].astype(np.float64)
        assert dec[3] == -np.inf and Z[3] == -np.inf
        assert (Z[:3] >= dec[:3]).all(), (K, th)            # no sum of the search rounds: no tolerance
        assert np.array_equal(np.isfinite(Z), np.isfinite(dec))                # (a narrow beam may end mid-word: both -inf)
        finite += int(np.isfinite(dec).sum())
    assert finite >= 2 * len(PRUNED) and np.isfinite(dec[:3]).all()            # the whole beam, the last setting, ends everywhere


def test_gradients_match_central_differences_with_the_sets_frozen():
    lex, lm, x, tr, il, tg, tl = _grid(2)
    gs = GS
    sets = la_lattice_sets(x, tr, lex, lm, 2, il, 3, INF, *W, tg, tl)
    plain = lattice_sets(x, tr, lex, lm, il, 3, INF, *W, tg, tl)
    assert sets[4] != plain[4]                             # a pruned setting: not the plain loss's lattice
    Z, gx, gtr, _ = beam_word_la_loss_ref(x, tr, lex, lm, 2, il, 3, INF, *W, tg, tl, gs, sets=sets)
    assert np.isfinite(Z[:3]).all()
    f = lambda x_, tr_: float((gs[:3] * beam_word_la_loss_ref(x_, tr_, lex, lm, 2, il, 3, INF, *W, sets=sets)[0][:3]).sum())   # noqa: E731
    eps = 1e-6
    rng = np.random.default_rng(0)
    for _ in range(25):
        t, b, i = rng.integers(7), rng.integers(4), rng.integers(5)
        d = np.zeros_like(x)
        d[t, b, i] = eps
        assert abs((f(x + d, tr) - f(x - d, tr)) / (2 * eps) - gx[t, b, i]) < 1e-7
    for i in range(5):
        for j in range(5):
            d = np.zeros_like(tr)
            d[i, j] = eps
            assert abs((f(x, tr + d) - f(x, tr - d)) / (2 * eps) - gtr[i, j]) < 1e-7
    assert (gx[4:, 1] == 0).all() and (gx[:, 3] == 0).all() and np.allclose(gx[:, 0].sum(axis=1), gs[0])


@pytest.mark.parametrize("order", [1, 2])
def test_a_beam_of_one_normalises_over_the_rescued_word(order):
    lex, lm, x, tr = rescue_case(np.float64)
    best = beam_word_ref(x, tr, lex, lm, None, ALL)
    Z, _, _, U = beam_word_la_loss_ref(x, tr, lex, lm, order, None, 1)
    Zp, _, _, Up = beam_word_loss_ref(x, tr, lex, lm, None, 1)
    assert all(len(u) == 1 for u in U[0])                  # one pair per frame: one label path, the rescued one
    assert abs(Z[0] - float(best["scores"][0])) < 1e-12    # its PLAIN score: the look-ahead terms are not in the lattice
    assert U[0] != Up[0] and abs(Z[0] - Zp[0]) > 1.0       # the plain loss at K = 1 normalises over the word the LM dislikes


@pytest.mark.parametrize("order", [1, 2, 3])
def test_dead_end_nodes_leave_the_sets_and_change_no_bit_of_the_whole_beam_loss(order):
    """Word d = [3, 0] of the hand-built case has no arc in the LM: the nodes [3] and [3, 0] are dead ends.  The look-ahead
    search never enters them, the plain search keeps them; no complete path runs through them, so alpha of every other pair,
    the ends, Z and -- beta of a dead-end pair being -inf -- both gradients are those of the plain whole-beam loss, bit for bit
    in this restatement (an absent member and a -inf member add the same nothing to a sum)."""
    from beam_word_la_ref import words_below
    lex, lm = hand_case()
    dead_nodes = {n for n in range(lex.graph.S) if not (words_below(lex)[n] - {4})}
    assert len(dead_nodes) == 2
    rng = np.random.default_rng(77)
    x, tr = rng.normal(size=(6, 3, 5)), rng.normal(size=(5, 5))
    il = np.array([6, 4, 1])
    gs = np.array([1.0, -0.5, 2.0])
    m, _, A, _, U = la_lattice_sets(x, tr, lex, lm, order, il, ALL, INF, *W)
    Z, gx, gtr, _ = beam_word_la_loss_ref(x, tr, lex, lm, order, il, ALL, INF, *W, grad_scores=gs)
    Zp, gxp, gtrp, Up = beam_word_loss_ref(x, tr, lex, lm, il, ALL, INF, *W, grad_scores=gs)
    dead = lambda u: {p for p in u if int(m.state[p[1]]) in dead_nodes}                  # noqa: E731
    assert not any(dead(a) for Ab in A for a in Ab)
    assert sum(len(dead(u)) for Ub in Up for u in Ub) > 5
    for Ub, Upb in zip(U, Up):
        for u, up in zip(Ub, Upb):
            assert set(u) == set(up) - dead(up)            # the look-ahead sets are the plain ones without the dead-end pairs
    assert np.isfinite(Z).all() and _same(Z, Zp) and _same(gx, gxp) and _same(gtr, gtrp)
    # a target through the dead end is rejected by the walk, as without look-ahead: nothing is forced, the normaliser stays
    tg = np.array([[3, 0, 4, 0, 4]] * 3)
    Zt, _, _, Ut = beam_word_la_loss_ref(x, tr, lex, lm, order, il, 2, INF, *W, tg, np.array([5, 3, 1]))
    Zn, _, _, Un = beam_word_la_loss_ref(x, tr, lex, lm, order, il, 2, INF, *W)
    assert Ut == Un and _same(Zt, Zn) and (words_target_scores_ref(lex, lm, tg, None, np.float64, *W) == -np.inf).all()


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_point_is_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    n = "asg_beam_words_full_forward_la"
    assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    assert int(L.asg_hip_version()) == 230 and "#define ASG_HIP_VERSION 230" in src       # an addition
    for twin in ("asg_beam_words_full_backward_la", "asg_beam_words_full_work_bytes_la", "asg_beam_words_full_scratch_bytes_la"):
        assert not hasattr(L, twin)                        # the backward and the sizes serve both forms


def _look(lex, lm, dtype, order=2):
    from torch_asg_amd import WordLookahead, wordlm
    dev = WordLookahead(lex, lm, order).compile("cpu", dtype, 1.0, 0.0)
    return wordlm.abi_lookahead(dev), dev


def test_abi_argument_checks_without_a_device():
    from torch_asg_amd import _lib
    lex = small_lexicon()
    lm, big = arpa_lm(5, 2, 1), arpa_lm(5, 3, 1, keep=(1.0, 1.0, 1.0))
    assert big.H > 2 * lm.H and big.A > 2 * lm.A
    for dtype, e in ((torch.float32, 4), (torch.float64, 8)):
        L, p, gb, w, keep = _abi(lex, lm, 7, 3, dtype, 4)
        la, keep_la = _look(lex, lm, dtype)
        wb = lambda K, store=1: int(L.asg_beam_words_full_work_bytes(*_refs(p, gb, w), K, store))    # noqa: E731
        mmax = (160 * 1024 - 256) // (16 + e)

        def fwd(K=8, th=1.0, work=256, nbytes=1 << 40, scores=256, flags=64, look=la):
            return L.asg_beam_words_full_forward_la(None, *_refs(p, gb, w), None if look is None else ctypes.byref(look), K, th,
                                                    work, nbytes, scores, flags, None)
        # the plain call's errors
        assert fwd(mmax - 3) == 2 and fwd(8193) == 2 and fwd(0) == 1 and fwd(th=-1.0) == 1 and fwd(th=float("nan")) == 1
        assert fwd(work=None) == 1 and fwd(scores=None) == 1
        assert fwd(nbytes=wb(8) - 1) == 3 and fwd(nbytes=wb(8, 0) - 1, flags=0) == 3            # the plain call's size, to the byte
        w.dtype = 1 - w.dtype
        assert fwd() == 1
        w.dtype = 1 - w.dtype
        for field, bad in (("start", lm.H), ("separator", 5), ("H", 0), ("row", None), ("word_of_state", None)):
            old = getattr(w, field)
            setattr(w, field, bad)
            assert fwd() == 1, field
            setattr(w, field, old)
        p.T = (1 << 20) + 1
        assert fwd() == 2
        p.T = 7
        # the look-ahead's own: NULL, another dtype, a NULL array, mis-sized
        assert fwd(look=None) == 1
        la.dtype = 1 - la.dtype
        assert fwd() == 1
        la.dtype = 1 - la.dtype
        for name in ("rlo", "rhi", "la_state", "krow", "krank", "tab", "dense0"):
            old = getattr(la, name)
            setattr(la, name, None)
            assert fwd() == 1, name
            setattr(la, name, old)
        for field, bad in (("S", la.S + 1), ("H", la.H + 1), ("A", -1), ("A", w.A + 1), ("levels", 0), ("levels", 32),
                           ("levels", la.levels + 8)):
            old = getattr(la, field)
            setattr(la, field, bad)
            assert fwd() == 1, (field, bad)
            setattr(la, field, old)
        assert fwd(nbytes=wb(8) - 1) == 3                  # (everything is back in place: only the size is wrong)
        # the LM doubled: the same bytes, and the look-ahead sizes nothing
        L2, p2, gb2, w2, keep2 = _abi(lex, big, 7, 3, dtype, 4)
        la2, keep_la2 = _look(lex, big, dtype, 3)
        assert la2.A > la.A
        for store in (0, 1):
            assert int(L2.asg_beam_words_full_work_bytes(*_refs(p2, gb2, w2), 8, store)) == wb(8, store) > 0
        assert L2.asg_beam_words_full_forward_la(None, *_refs(p2, gb2, w2), ctypes.byref(la2), 8, 1.0, 256, wb(8) - 1, 256, 64,
                                                 None) == 3
        assert L2.asg_beam_words_full_forward_la(None, *_refs(p2, gb2, w2), ctypes.byref(la), 8, 1.0, 256, 1 << 40, 256, 64,
                                                 None) == 1             # built for the other LM's shape
    assert _lib.ASG_DTYPE_F32 + _lib.ASG_DTYPE_F64 == 1    # (what "1 - dtype" above relies on)


def test_python_surface_checks_the_look_ahead_before_any_device_work():
    import torch_asg_amd as A
    lex, lm = small_lexicon(), arpa_lm(5, 2, 1)
    other = A.WordLookahead(small_lexicon(), lm, 2)        # an equal lexicon, but not this one
    good = A.WordLookahead(lex, lm, 2)
    x, tr = torch.zeros(4, 2, 5), torch.zeros(5, 5)        # CPU tensors: a device check would refuse them
    tg = torch.zeros(2, 2, dtype=torch.int64)
    crit = A.ASGLoss(5)
    calls = (lambda la: A.beam_words_full_score(x, tr, lex, lm, beam_size=4, lookahead=la),
             lambda la: A.beam_words_asg_loss(x, tg, tr, lex, lm, beam_size=4, lookahead=la),
             lambda la: crit.beam_word_loss(x, tg, lex, lm, beam_size=4, lookahead=la))
    for call in calls:
        with pytest.raises(TypeError, match="WordLookahead"):
            call("order 2")
        with pytest.raises(RuntimeError, match="another lexicon or word LM"):
            call(other)
        with pytest.raises(RuntimeError) as err:           # a good look-ahead gets as far as the device check
            call(good)
        assert "another lexicon" not in str(err.value)
    with pytest.raises(TypeError, match="Lexicon"):        # the pair's own checks still come first
        A.beam_words_full_score(x, tr, lex.graph, lm, lookahead=good)
    with pytest.raises(ValueError, match="beam_size"):
        A.beam_words_full_score(x, tr, lex, lm, beam_size=0, lookahead=good)
