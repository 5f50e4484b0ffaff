"""GPU tests (-m gpu) of the beam-pruned loss over the pairs a LOOK-AHEAD search keeps (`beam_words_full_score(..., lookahead=)`,
`beam_words_asg_loss(..., lookahead=)`, csrc/asg_beam_word_loss.hip with the search's look-ahead flag on): score and both
gradients against the test-side numpy restatement (tests/beam_word_la_loss_ref.py, pinned on the CPU by
tests/test_beam_word_la_loss_cpu.py) with the comparison and the tolerances of tests/test_hip_beam_word_loss.py -- float64:
np.allclose(rtol=1e-9, atol=1e-9); float32: tests/util.py::assert_close; the inf pattern exact.  The lattice kernels are that
file's; what is new is the search that feeds them.  Every case first asserts, from the restatement's own sets, that its input is
in the regime it names."""
import numpy as np
import pytest
import torch

from beam_word_la_loss_ref import beam_word_la_loss_ref, la_lattice_sets
from beam_word_loss_ref import lattice_sets, words_target_scores_ref
from test_beam_word_la_cpu import hand_case, rescue_case
from test_hip_beam_word import ties_case
from test_hip_beam_word_loss import ALL, DEV, DTYPES, INF, W, _close, _gpu, _normal, grid_case, wide_lexicon_and_lm

pytestmark = pytest.mark.gpu
WW = (0.5, -0.2, 0.1)                                      # the weights of the wide cases


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _n(t):
    return None if t is None else t.numpy()


def _ref(x, tr, lex, lm, la, il, K, theta=INF, w=W, tg=None, tl=None, gs=None, info=None):
    return beam_word_la_loss_ref(x.numpy(), tr.numpy(), lex, lm, la.order, _n(il), K, theta, *w, _n(tg), _n(tl), _n(gs), info=info)


def _check(x, tr, lex, lm, la, il, K, theta=INF, w=W, tg=None, tl=None, gs=None, info=None, what="", **kw):
    got = _gpu(x, tr, lex, lm, il, K, theta, w, tg, tl, gs, lookahead=la, **kw)
    want = _ref(x, tr, lex, lm, la, il, K, theta, w, tg, tl, gs, info)
    for name, g_, w_ in zip(("Z", "grad_inputs", "grad_transition"), got, want):
        _close(g_, w_, x.dtype, "%s %s K=%d theta=%s order=%d targets=%s" % (name, what, K, theta, la.order, tg is not None))
    return got, want


def _plain_sets(x, tr, lex, lm, il, K, theta, w=W, tg=None, tl=None):
    return lattice_sets(x.numpy(), tr.numpy(), lex, lm, _n(il), K, theta, *w, _n(tg), _n(tl))[4]


# ---------------------------------------------------------------------------------------------------------------- grid
@DTYPES
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("lm_order", [2, 3], ids=["bigram", "trigram"])
def test_grid_of_beams_thresholds_and_orders(lm_order, order, dtype):
    lex, lm, x, tr, il, tg, tl = grid_case(lm_order, dtype)
    la = _asg().WordLookahead(lex, lm, order)
    gs = torch.tensor([1.0, -0.5, 2.0, 3.0])
    forced_outside = 0
    for K in (1, 2, 3, 8, ALL):
        for theta in (INF, 2.0):
            for t_, l_ in ((None, None), (tg, tl)):
                (Z, gx, _), (_, _, _, U) = _check(x, tr, lex, lm, la, il, K, theta, tg=t_, tl=l_, gs=gs, what="grid")
                assert Z[3] == -np.inf and (gx[:, 3] == 0).all() and (gx[1:, 2] == 0).all()        # lengths 0 and 1
                if (K, theta) != (ALL, INF):               # the regime: not the plain loss's lattice
                    assert U != _plain_sets(x, tr, lex, lm, il, K, theta, W, t_, l_), (K, theta)
            _, _, A_, F_, _ = la_lattice_sets(x.numpy(), tr.numpy(), lex, lm, order, il.numpy(), K, theta, *W, tg.numpy(), tl.numpy())
            forced_outside += sum(len(set(f) - set(a)) for Ab, Fb in zip(A_, F_) for a, f in zip(Ab, Fb))
    assert forced_outside > 0                              # some forced pair was not in the beam: leaving F out cannot pass


# ---------------------------------------------------------------------------------------------------------------- ties
@DTYPES
def test_integer_ties_at_the_last_rank_and_between_sources(dtype):
    lex, lm, x, tr, il = ties_case(dtype)
    cuts = srcs = 0
    for order in (1, 2):
        la = _asg().WordLookahead(lex, lm, order)
        for K in (1, 2, 3, 5, 8):
            for theta in (INF, 1.0):
                info = {}
                _check(x, tr, lex, lm, la, il, K, theta, (1.0, 1.0, 0.0), info=info, what="ties")
                cuts += info["tie_cuts"]
                srcs += info["src_ties"]
    assert cuts > 0 and srcs > 0


# ---------------------------------------------------------------------------------------------------------------- rescue
@DTYPES
def test_a_beam_of_one_normalises_over_the_rescued_word(dtype):
    A = _asg()
    lex, lm, x, tr = rescue_case(np.float32 if dtype == torch.float32 else np.float64)
    x, tr = torch.from_numpy(x), torch.from_numpy(tr)
    w = (1.0, 0.0, 0.0)
    best = A.beam_decode_words(x.to(DEV), tr.to(DEV), lex, lm, None, ALL).scores.cpu().numpy()
    plain = _gpu(x, tr, lex, lm, None, 1, INF, w)[0]
    for order in (1, 2):
        (Z, _, _), (_, _, _, U) = _check(x, tr, lex, lm, A.WordLookahead(lex, lm, order), None, 1, INF, w, what="rescue")
        assert all(len(u) == 1 for u in U[0]) and U[0] != _plain_sets(x, tr, lex, lm, None, 1, INF, w)[0]
        assert abs(Z[0] - best[0]) < 1e-5 and abs(Z[0] - plain[0]) > 1.0       # the rescued path's plain score, not the poor word's


# ---------------------------------------------------------------------------------------------------------------- dead ends
@DTYPES
def test_dead_ends_pruned_on_entry_and_a_target_forced_through_dropped_pairs(dtype):
    from beam_word_la_ref import words_below
    A = _asg()
    lex, lm = hand_case()                                  # the nodes [3] and [3, 0] have no word below them that the LM knows
    dead_nodes = {n for n in range(lex.graph.S) if not (words_below(lex)[n] - {4})}
    x, tr = _normal(7, 4, 5, 37, dtype)
    x[:, :, 3] += 2.0                                      # acoustics like the dead branch
    il = torch.tensor([7, 4, 1, 0])
    tg = torch.tensor([[0, 1, 4, 1, 4], [2, 4, 0, 4, 0], [0, 4, 0, 0, 0], [2, 4, 0, 0, 0]])      # "ab" "b" / "c" "a" / "a"
    tl = torch.tensor([5, 4, 1, 2])
    assert np.isfinite(words_target_scores_ref(lex, lm, tg.numpy(), tl.numpy(), np.float64, *W)[:3]).all()
    gs = torch.tensor([1.0, -0.5, 2.0, 3.0])
    for order in (1, 2, 3):
        la = A.WordLookahead(lex, lm, order)
        for K in (2, 8, ALL):
            info = {}
            _check(x, tr, lex, lm, la, il, K, INF, gs=gs, info=info, what="dead")
            m, _, A_, F_, _ = la_lattice_sets(x.numpy(), tr.numpy(), lex, lm, order, il.numpy(), K, INF, *W, tg.numpy(), tl.numpy())
            assert info["dead"] > 0 and not any(int(m.state[q]) in dead_nodes for Ab in A_ for a in Ab for _, q in a)
            if K == 2:                                     # some frame's forced pairs are not among the kept ones
                assert any(f and not (set(f) <= set(a)) for Ab, Fb in zip(A_, F_) for a, f in zip(Ab, Fb))
            _check(x, tr, lex, lm, la, il, K, INF, tg=tg, tl=tl, gs=gs, what="dead, forced")
        plain = _plain_sets(x, tr, lex, lm, il, ALL, INF)  # the plain whole beam holds the dead-end pairs, and Z is the same
        assert any(int(m.state[q]) in dead_nodes for Ub in plain for u in Ub for _, q in u)
        a = _gpu(x, tr, lex, lm, il, ALL, INF, gs=gs, lookahead=la)
        b = _gpu(x, tr, lex, lm, il, ALL, INF, gs=gs)
        for name, u, v in zip(("Z", "grad_inputs", "grad_transition"), a, b):
            _close(u, v, dtype, "dead ends, whole beam against the plain loss: " + name)


@DTYPES
def test_a_target_the_lm_rejects_gives_inf_and_the_normalisers_posterior(dtype):
    A = _asg()
    lex, lm = hand_case()
    la = A.WordLookahead(lex, lm, 2)
    x, tr = _normal(7, 3, 5, 39, dtype)
    tg = torch.tensor([[3, 0, 4, 0, 4],                   # word d = [3, 0]: the LM has no arc for it
                       [0, 1, 4, 1, 4],                   # accepted
                       [0, 3, 4, 0, 0]])                  # no word "0 3": the lexicon rejects
    tl = torch.tensor([5, 5, 3])
    walk = words_target_scores_ref(lex, lm, tg.numpy(), tl.numpy(), np.float64, *W)
    assert np.array_equal(np.isfinite(walk), [False, True, False])
    xd, trd = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
    loss = A.beam_words_asg_loss(xd, tg.to(DEV), trd, lex, lm, None, tl.to(DEV), 3, INF, *W, lookahead=la)
    got = loss.detach().cpu().numpy()
    assert np.array_equal(got == np.inf, ~np.isfinite(walk)) and np.isfinite(got[1]) and got[1] >= -1e-4
    gs = torch.tensor([1.0, 0.0, 1.0])
    Z = A.beam_words_full_score(xd, trd, lex, lm, None, 3, INF, *W, tg.to(DEV), tl.to(DEV), lookahead=la)
    Z.backward(gs.to(DEV).to(Z.dtype))
    _, gx, gtr, _ = _ref(x, tr, lex, lm, la, None, 3, INF, gs=gs)                         # the normaliser WITHOUT targets
    _close(xd.grad.cpu().numpy(), gx, dtype, "posterior grad_inputs")
    _close(trd.grad.cpu().numpy(), gtr, dtype, "posterior grad_transition")


# ---------------------------------------------------------------------------------------------------------------- histories
@DTYPES
@pytest.mark.parametrize("order", [2, 3])
def test_a_separator_edge_whose_history_reads_another_row_than_the_empty_historys(order, dtype):
    lex, lm, x, tr, il, _, _ = grid_case(3, dtype)
    la = _asg().WordLookahead(lex, lm, order)
    _, (_, _, _, U) = _check(x, tr, lex, lm, la, il, 4, INF, what="history")
    m = la_lattice_sets(x.numpy(), tr.numpy(), lex, lm, order, il.numpy(), 4, INF, *W)[0]
    carried = 0
    for Ub in U:
        for t in range(1, len(Ub)):
            here = set(Ub[t])
            for p in Ub[t - 1]:                            # a separator edge inside the lattice out of a pair whose look-ahead
                if int(la.la_state[p[0]]) != 0:            # row is not state 0's
                    carried += sum(1 for p2, _, i in m.edges(p)[1:] if i == m.sep and p2 in here)
    assert carried > 0


# ---------------------------------------------------------------------------------------------------------------- set sizes
@DTYPES
@pytest.mark.parametrize("K", [32, 33, 63, 64, 65])
def test_set_sizes_around_a_lane_group_boundary_and_the_wavefront(K, dtype):
    """|U_{t-1}| = K exactly in a frame that has a successor, the sets taken under look-ahead: 32 / 33 is where the lanes per
    source pair of the forward and the backward halve, 63 / 64 / 65 lie around a wavefront."""
    lex, lm = wide_lexicon_and_lm()
    la = _asg().WordLookahead(lex, lm, 2)
    x, tr = _normal(5, 2, 40, 33, dtype)
    info = {}
    _, (_, _, _, U) = _check(x * 0.25, tr * 0.25, lex, lm, la, torch.tensor([5, 4]), K, INF, WW, info=info, what="sizes")
    assert max(max(s) for s in info["sizes"]) == K
    assert any(len(u) == K for Ub in U for u in Ub[:-1])
    assert U != _plain_sets(x * 0.25, tr * 0.25, lex, lm, torch.tensor([5, 4]), K, INF, WW)


def test_wide_beam_more_than_1024_candidates_and_kept_pairs_in_a_frame():
    """N = 40, 300 words, T = 12, K = 1200, float32: the search strips the workgroup over its candidates and its select over
    more than 1024 of them, with the ranges of a 300-word row over the upper levels of the look-ahead's table."""
    lex, lm = wide_lexicon_and_lm()
    la = _asg().WordLookahead(lex, lm, 2)
    assert la.levels >= 8                                  # state 0's row holds all 300 words
    x, tr = _normal(12, 2, 40, 33, torch.float32)
    info = {}
    _, (Z, _, _, U) = _check(x * 0.25, tr * 0.25, lex, lm, la, torch.tensor([12, 4]), 1200, INF, WW, info=info, what="wide")
    assert max(max(c) for c in info["cands"]) > 1024 and max(max(s) for s in info["sizes"]) > 1024
    assert max(len(u) for Ub in U for u in Ub[:-1]) > 1024 and np.isfinite(Z).all()


@pytest.mark.parametrize("N", [141, 142], ids=["transitions-in-lds", "transitions-in-global-memory"])
def test_both_transition_layouts_of_the_search(N):
    """float64, K = 8: 4096 + 8 * 16 + N * N * 8 bytes is within the 160 KiB of LDS for N = 141 and beyond them for N = 142."""
    from beam_word_cases import arpa_lm
    A = _asg()
    K = 8
    assert (4096 + K * 16 + N * N * 8 <= 160 * 1024) == (N == 141)
    lex = A.Lexicon([[3, 7], [3, 100, 5], [N - 2]], N, N - 1)
    lm = arpa_lm(3, 2, 73)
    x, tr = _normal(4, 2, N, 37, torch.float64)
    for t, lab in enumerate([3, 7, N - 1, N - 2]):
        x[t, 0, lab] += 6.0
    tg = torch.tensor([[3, 7, N - 1, N - 2], [N - 2, N - 1, 0, 0]])
    tl = torch.tensor([4, 2])
    info = {}
    (Z, _, _), _ = _check(x, tr, lex, lm, A.WordLookahead(lex, lm, 2), torch.tensor([4, 3]), K, INF, tg=tg, tl=tl,
                          gs=torch.tensor([1.0, -2.0]), info=info, what="N=%d" % N)
    assert np.isfinite(Z).all() and max(max(z) for z in info["sizes"]) > 1


# ---------------------------------------------------------------------------------------------------------------- equivalences
@DTYPES
@pytest.mark.parametrize("order", [1, 2, 3])
def test_the_whole_beam_is_the_devices_plain_loss_and_none_is_the_call_as_it_was(order, dtype):
    A = _asg()
    lex, lm, x, tr, il, tg, tl = grid_case(3, dtype)
    la = A.WordLookahead(lex, lm, order)
    gs = torch.tensor([1.0, -0.5, 2.0, 3.0])
    for t_, l_ in ((None, None), (tg, tl)):
        a = _gpu(x, tr, lex, lm, il, ALL, INF, W, t_, l_, gs, lookahead=la)
        b = _gpu(x, tr, lex, lm, il, ALL, INF, W, t_, l_, gs)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))           # nothing pruned, no dead end: bit for bit
        assert np.isfinite(a[0][:3]).all()
    for K, theta in ((2, INF), (16, 3.0)):
        a = _gpu(x, tr, lex, lm, il, K, theta, W, tg, tl, gs)
        b = _gpu(x, tr, lex, lm, il, K, theta, W, tg, tl, gs, lookahead=None)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


@DTYPES
@pytest.mark.parametrize("order", [1, 2, 3])
def test_in_eighths_z_is_at_least_the_devices_look_ahead_decode(order, dtype):
    from beam_word_cases import arpa_lm, eighths, small_lexicon
    A = _asg()
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = eighths(arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5)))
    la = A.WordLookahead(lex, lm, order)
    g = torch.Generator().manual_seed(35)
    x = (torch.randint(-32, 32, (7, 4, 5), generator=g) / 8.0).to(dtype)
    tr = (torch.randint(-16, 16, (5, 5), generator=g) / 8.0).to(dtype)
    il = torch.tensor([7, 4, 1, 0])
    w = (1.0, 0.25, 0.125)
    finite = 0
    for K in (1, 2, 3, 8, ALL):
        for theta in (INF, 2.0):
            Z = _gpu(x, tr, lex, lm, il, K, theta, w, lookahead=la)[0]
            dec = A.beam_decode_words(x.to(DEV), tr.to(DEV), lex, lm, il.to(DEV), K, theta, *w, lookahead=la).scores.cpu().numpy()
            assert (Z >= dec).all() and np.array_equal(np.isfinite(Z), np.isfinite(dec)), (K, theta)     # no sum rounds
            finite += int(np.isfinite(dec).sum())
    assert finite >= 20


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_two_runs_give_identical_bits_and_groups_equal_one_call():
    A = _asg()
    lex, lm = wide_lexicon_and_lm()
    la = A.WordLookahead(lex, lm, 2)
    x, tr = _normal(12, 6, 40, 36, torch.float32)
    il = torch.tensor([12, 3, 0, 1, 11, 7])
    tg = torch.tensor([[3, 7, 39, 11, 2, 39]] * 6)
    tl = torch.tensor([6, 3, 3, 1, 6, 0])
    gs = torch.tensor([1.0, 2.0, 3.0, -1.0, 0.5, 1.5])
    a = _gpu(x * 0.25, tr, lex, lm, il, 100, 6.0, WW, tg, tl, gs, lookahead=la)
    assert np.isfinite(a[0][[0, 1, 3, 4, 5]]).all()
    plain = _gpu(x * 0.25, tr, lex, lm, il, 100, 6.0, WW, tg, tl, gs)
    assert a[0].tobytes() != plain[0].tobytes()            # it is another lattice
    for _ in range(2):
        b = _gpu(x * 0.25, tr, lex, lm, il, 100, 6.0, WW, tg, tl, gs, lookahead=la)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    from torch_asg_amd.asg import native
    be = native()
    seen = []
    buf = be._buf
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    try:
        _gpu(x * 0.25, tr, lex, lm, il, 100, 6.0, WW, tg, tl, gs)
        plain_bytes = max(seen)
        seen.clear()
        _gpu(x * 0.25, tr, lex, lm, il, 100, 6.0, WW, tg, tl, gs, lookahead=la)
        assert max(seen) == plain_bytes                    # no workspace of its own
        per = plain_bytes // 6
        seen.clear()
        small = _gpu(x * 0.25, tr, lex, lm, il, 100, 6.0, WW, tg, tl, gs, lookahead=la, max_work_bytes=2 * per + per // 2)
        assert seen.count(2 * per) == 3                    # three groups of two utterances, each keeps its alpha
    finally:
        del be._buf
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, small))
    assert la.compile(DEV, torch.float32, 0.5, -0.2) is la.compile(DEV, torch.float32, 0.5, -0.2)      # a warm call copies nothing


def test_capture_of_forward_and_backward_with_three_replays_on_new_emissions():
    A = _asg()
    lex, lm, x0, tr, _, tg, tl = grid_case(3, torch.float32)
    la = A.WordLookahead(lex, lm, 2)
    T, B, N = 7, 4, 5
    x = torch.zeros(T, B, N, device=DEV, requires_grad=True)
    trd = tr.to(DEV).requires_grad_(True)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)
    tgd, tld = tg.to(DEV), tl.to(DEV)
    gs = torch.tensor([1.0, -0.5, 2.0, 3.0], device=DEV)

    def step():
        Z = A.beam_words_full_score(x, trd, lex, lm, il, 4, 3.0, *W, tgd, tld, lookahead=la)
        gx, gtr = torch.autograd.grad(Z, (x, trd), gs)
        return Z.detach(), gx, gtr
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                             # warm-up: compiles and caches lexicon, LM and look-ahead
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = step()
    for seed in (1, 2, 3):
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            x.copy_(torch.randn(T, B, N, generator=gen))
        il.copy_(torch.tensor([T, 4 + seed % 2, 1, T - seed]))
        tld.copy_(torch.tensor([5, 4, 1, min(2, T - seed)]))
        gr.replay()
        torch.cuda.synchronize()
        eager = step()
        for u, v in zip(out, eager):
            assert torch.equal(u, v)
        want = beam_word_la_loss_ref(x.detach().cpu().numpy(), tr.numpy(), lex, lm, 2, il.cpu().numpy(), 4, 3.0, *W, tg.numpy(),
                                     tld.cpu().numpy(), gs.cpu().numpy())
        for n, u, w_ in zip(("Z", "gx", "gtr"), out, want):
            _close(u.cpu().numpy(), w_, torch.float32, "replay %d %s" % (seed, n))


def test_the_neighbours_are_unchanged_right_after_a_look_ahead_loss_call():
    A = _asg()
    lex, lm, x, tr, il, tg, tl = grid_case(3, torch.float32)
    la = A.WordLookahead(lex, lm, 2)
    xd, trd, ild, tgd, tld = x.to(DEV), tr.to(DEV), il.to(DEV), tg.to(DEV), tl.to(DEV)

    def others():
        out = list(A.beam_decode_words(xd, trd, lex, lm, ild, 6, 4.0, *W))
        out += list(A.beam_decode_words(xd, trd, lex, lm, ild, 6, 4.0, *W, lookahead=la))
        xg, tg_ = xd.clone().requires_grad_(True), trd.clone().requires_grad_(True)
        loss = A.beam_words_asg_loss(xg, tgd, tg_, lex, lm, ild, tld, 6, 4.0, *W)
        loss[:2].sum().backward()
        out += [loss.detach(), xg.grad, tg_.grad]
        return [o.cpu() for o in out]
    before = others()
    xg = xd.clone().requires_grad_(True)
    A.beam_words_asg_loss(xg, tgd, trd, lex, lm, ild, tld, 64, 4.0, *W, lookahead=la)[:2].sum().backward()
    after = others()
    for u, v in zip(before, after):
        assert torch.equal(u, v)


def test_the_module_method_reductions_and_an_upstream_parameter():
    A = _asg()
    lex, lm, x, tr, il, tg, tl = grid_case(2, torch.float32)
    la = A.WordLookahead(lex, lm, 2)
    il, tl = torch.tensor([7, 5, 6, 7]), torch.tensor([5, 4, 1, 2])
    crit = {r: A.ASGLoss(5, reduction=r).to(DEV) for r in ("none", "sum", "mean")}
    for c in crit.values():
        with torch.no_grad():
            c.transition.copy_(tr.to(DEV))
    lin = torch.nn.Linear(5, 5).to(DEV)
    args = (tg.to(DEV), lex, lm, il.to(DEV), tl.to(DEV), *W)
    per = crit["none"].beam_word_loss(lin(x.to(DEV)), *args, beam_size=2, beam_threshold=5.0, lookahead=la)
    fn = A.beam_words_asg_loss(lin(x.to(DEV)), tg.to(DEV), crit["none"].transition, lex, lm, il.to(DEV), tl.to(DEV), 2, 5.0, *W,
                               lookahead=la)
    plain = crit["none"].beam_word_loss(lin(x.to(DEV)), *args, beam_size=2, beam_threshold=5.0)
    assert per.shape == (4,) and torch.isfinite(per).all() and (per >= -1e-4).all() and torch.equal(per, fn)
    assert not torch.equal(per, plain)                     # the keyword reached the search
    tot = crit["sum"].beam_word_loss(lin(x.to(DEV)), *args, beam_size=2, beam_threshold=5.0, lookahead=la)
    mean = crit["mean"].beam_word_loss(lin(x.to(DEV)), *args, beam_size=2, beam_threshold=5.0, lookahead=la)
    assert torch.allclose(tot, per.sum(), rtol=1e-5) and torch.allclose(mean, per.mean(), rtol=1e-5)
    mean.backward()
    assert lin.weight.grad is not None and torch.isfinite(lin.weight.grad).all() and lin.weight.grad.abs().sum() > 0
    assert crit["mean"].transition.grad is not None and crit["mean"].transition.grad.abs().sum() > 0
