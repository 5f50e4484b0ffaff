"""GPU tests (-m gpu) of the beam-pruned loss over the pairs of the word decoder (`torch_asg_amd.beam_words_full_score`,
`beam_words_asg_loss`, csrc/asg_beam_word_loss.hip): score and both gradients against the test-side numpy restatement
(tests/beam_word_loss_ref.py, pinned on the CPU by tests/test_beam_word_loss_cpu.py).  float64: np.allclose(rtol=1e-9,
atol=1e-9); float32: tests/util.py::assert_close; the inf pattern exact.  Every case first asserts, from the restatement's own
sets, that its input is in the regime it names."""
import functools

import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, compose_static, eighths, small_lexicon, without_unigrams
from beam_word_loss_ref import beam_word_loss_ref, lattice_sets, word_model, words_target_scores_ref
from util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
ALL = 1024                                                 # more than every pair of the small cases
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
W = (0.7, -0.4, 0.3)                                       # lm_weight, word_score, token_score
TARGET = [0, 1, 4, 2, 4]


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _normal(T, B, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, B, N, generator=g, dtype=torch.float64).to(dtype), torch.randn(N, N, generator=g, dtype=torch.float64).to(dtype)


def _close(got, want, dtype, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any(), what
    if dtype == torch.float64:
        assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got[np.isinf(got)], want[np.isinf(want)]), what
        fin = np.isfinite(want)
        assert np.allclose(got[fin], want[fin], rtol=1e-9, atol=1e-9), "%s: %.3e" % (what, np.abs(got[fin] - want[fin]).max())
    else:
        assert_close(got, want, what=what)


def _gpu(x, tr, lex, lm, il, K, theta=INF, w=W, tg=None, tl=None, gs=None, **kw):
    """-> (Z, grad_inputs, grad_transition) of sum_b gs[b] * Z[b] on the device, as numpy."""
    A = _asg()
    xd, trd = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
    Z = A.beam_words_full_score(xd, trd, lex, lm, None if il is None else il.to(DEV), K, theta, *w,
                                None if tg is None else tg.to(DEV), None if tl is None else tl.to(DEV), **kw)
    assert Z.dtype == x.dtype and Z.shape == (x.shape[1],)
    g = torch.ones_like(Z) if gs is None else gs.to(DEV).to(Z.dtype)
    Z.backward(g)
    torch.cuda.synchronize()
    return Z.detach().cpu().numpy(), xd.grad.cpu().numpy(), trd.grad.cpu().numpy()


def _ref(x, tr, lex, lm, il, K, theta=INF, w=W, tg=None, tl=None, gs=None, info=None):
    n = lambda t: None if t is None else t.numpy()          # noqa: E731
    return beam_word_loss_ref(x.numpy(), tr.numpy(), lex, lm, n(il), K, theta, *w, n(tg), n(tl), n(gs), info=info)


def _check(x, tr, lex, lm, il, K, theta=INF, w=W, tg=None, tl=None, gs=None, info=None, what="", **kw):
    got = _gpu(x, tr, lex, lm, il, K, theta, w, tg, tl, gs, **kw)
    want = _ref(x, tr, lex, lm, il, K, theta, w, tg, tl, gs, info)
    for name, g_, w_ in zip(("Z", "grad_inputs", "grad_transition"), got, want):
        _close(g_, w_, x.dtype, "%s %s K=%d theta=%s targets=%s" % (name, what, K, theta, tg is not None))
    return got, want


# ---------------------------------------------------------------------------------------------------------------- grid
def grid_case(order, dtype):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, order, 60 + order, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(7, 4, 5, 31, dtype)
    tg = torch.tensor([TARGET, [2, 4, 1, 0, 0], [0, 4, 0, 0, 0], [2, 4, 0, 0, 0]])
    return lex, lm, x, tr, torch.tensor([7, 4, 1, 0]), tg, torch.tensor([5, 4, 1, 2])


@DTYPES
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_grid_of_beams_and_thresholds(order, dtype):
    A = _asg()
    lex, lm, x, tr, il, tg, tl = grid_case(order, dtype)
    if order == 2:                                         # the bigram has missing pairs: some step backs off
        assert lm.A < lm.H * 5
    gs = torch.tensor([1.0, -0.5, 2.0, 3.0])
    forced_outside = 0
    for K in (1, 2, 3, 8, ALL):
        for theta in (INF, 2.0, 0.0):
            (Z, _, _), _ = _check(x, tr, lex, lm, il, K, theta, gs=gs, what="grid")
            dec = A.beam_decode_words(x.to(DEV), tr.to(DEV), lex, lm, il.to(DEV), K, theta, *W).scores.cpu().numpy()
            assert (Z >= dec - 1e-5 * np.maximum(1.0, np.abs(dec))).all() and Z[3] == -np.inf
            _, _, A_, F_, _ = lattice_sets(x.numpy(), tr.numpy(), lex, lm, il.numpy(), K, theta, *W, tg.numpy(), tl.numpy())
            forced_outside += sum(len(set(f) - set(a)) for Ab, Fb in zip(A_, F_) for a, f in zip(Ab, Fb))
            (Zt, _, _), _ = _check(x, tr, lex, lm, il, K, theta, tg=tg, tl=tl, gs=gs, what="grid")
            assert (Zt >= Z - 1e-5 * np.maximum(1.0, np.abs(Z)))[:3].all()
    assert forced_outside > 0                              # some forced pair was not in the beam: leaving F out cannot pass


# ---------------------------------------------------------------------------------------------------------------- regimes
def test_fan_in_through_the_lm():
    """Two kept pairs with different histories and one word-end node push into ONE (h', separator) pair."""
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 2, 62, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(7, 2, 5, 37, torch.float64)
    (_, _, _), (_, _, _, U) = _check(x * 0.5, tr * 0.5, lex, lm, None, ALL, INF, what="fan-in")
    m = word_model(lex, lm, np.float64, *W)
    merges = 0
    for Ub in U:
        for t in range(1, len(Ub)):
            into, here = {}, set(Ub[t])
            for p in Ub[t - 1]:
                for p2, _, i in m.edges(p)[1:]:
                    if i == m.sep and p2 in here:
                        into.setdefault(p2, set()).add(p)
            merges += sum(1 for srcs in into.values() if len({h for h, _ in srcs}) > 1 and len({q for _, q in srcs}) < len(srcs))
    assert merges > 0


@DTYPES
def test_every_kind_of_end(dtype):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 2, 63)
    x, tr = _normal(5, 3, 5, 38, dtype)
    (_, _, _), (_, _, _, U) = _check(x, tr, lex, lm, None, ALL, INF, what="ends")
    m = word_model(lex, lm, np.float64, *W)
    last = U[0][-1]
    kinds = {("root" if m.state[q] == 0 else "word" if m.wos[m.state[q]] >= 0 else "mid") for _, q in last}
    assert kinds == {"root", "word", "mid"}
    assert any(m.endw(p) == -np.inf for p in last) and any(m.endw(p) > -np.inf for p in last)


@DTYPES
def test_loss_with_a_beam_of_one_that_never_keeps_the_target(dtype):
    A = _asg()
    lex, lm, x, tr, il, tg, tl = grid_case(2, dtype)
    x = x.clone()
    x[0, 0, 1] += 8.0                                      # the beam of one enters "1 0" and stays on its last token;
    x[1:, 0, 0] += 8.0                                     # the target begins with "0 1"
    il = torch.tensor([7, 4, 1, 0])
    _, _, A_, F_, _ = lattice_sets(x.numpy(), tr.numpy(), lex, lm, il.numpy(), 1, INF, *W, tg.numpy(), tl.numpy())
    assert all(len(f) > 0 and not (set(f) & set(a)) for a, f in zip(A_[0], F_[0]))
    xd, trd = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
    loss = A.beam_words_asg_loss(xd, tg.to(DEV), trd, lex, lm, il.to(DEV), tl.to(DEV), 1, INF, *W)
    got = loss.detach().cpu().numpy()
    assert np.isfinite(got[0]) and got[0] >= -1e-4 and got[3] == np.inf and not np.isnan(got).any()
    Zt = _ref(x, tr, lex, lm, il, 1, INF, tg=tg, tl=tl)[0]
    fac = A.FAC.apply(trd, xd, tg.to(DEV), il.to(DEV), tl.to(DEV)).detach().cpu().numpy().astype(np.float64)
    walk = words_target_scores_ref(lex, lm, tg.numpy(), tl.numpy(), x.numpy().dtype.type, *W)
    fin = np.isfinite(got)
    _close(got[fin], Zt[fin] - (fac[fin] + walk[fin]), dtype, "loss K=1")
    loss[torch.tensor(fin, device=DEV)].sum().backward()
    assert torch.isfinite(xd.grad).all() and torch.isfinite(trd.grad).all()


@DTYPES
def test_rejected_targets_give_inf_and_the_normalisers_posterior(dtype):
    A = _asg()
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = without_unigrams(arpa_lm(5, 2, 64, keep=(1.0, 0.0, 0.0)), {3})     # unigrams only: word 3 ("2") is rejected everywhere
    x, tr = _normal(7, 6, 5, 39, dtype)
    tg = torch.tensor([[0, 3, 4, 0, 0],                   # no word "0 3": the lexicon rejects
                       [2, 4, 0, 4, 0],                   # the LM rejects word 3
                       [0, 1, 2, 0, 0],                   # accepted: ends in a word-end node
                       [1, 0, 4, 1, 0],                   # ends mid-word ("1" of "1 0")
                       [0, -1, 4, 0, 0],                  # outside labels
                       [0, 5, 4, 0, 0]])
    tl = torch.tensor([3, 4, 3, 4, 3, 3])
    walk = words_target_scores_ref(lex, lm, tg.numpy(), tl.numpy(), np.float64, *W)
    assert np.array_equal(np.isfinite(walk), [False, False, True, False, False, False])
    xd, trd = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
    loss = A.beam_words_asg_loss(xd, tg.to(DEV), trd, lex, lm, None, tl.to(DEV), 3, INF, *W)
    got = loss.detach().cpu().numpy()
    assert np.array_equal(got == np.inf, ~np.isfinite(walk)) and np.isfinite(got[2]) and got[2] >= -1e-4
    dev_walk = A.asg.native().words_target_scores(xd.detach(), trd.detach(), lex, lm, tg.to(DEV), tl.to(DEV), *W).cpu().numpy()
    _close(dev_walk, walk, dtype, "target scores")
    gs = torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0, 1.0])
    Z = A.beam_words_full_score(xd, trd, lex, lm, None, 3, INF, *W, tg.to(DEV), tl.to(DEV))
    Z.backward(gs.to(DEV).to(Z.dtype))
    _, gx, gtr, _ = _ref(x, tr, lex, lm, None, 3, INF, gs=gs)                              # the normaliser WITHOUT targets
    _close(xd.grad.cpu().numpy(), gx, dtype, "posterior grad_inputs")
    _close(trd.grad.cpu().numpy(), gtr, dtype, "posterior grad_transition")


@DTYPES
def test_a_repeat_in_the_target(dtype):
    lex, lm, x, tr, il, _, _ = grid_case(3, dtype)
    tg = torch.tensor([[0, 0, 1, 1, 4, 2, 2], [2, 2, 4, 4, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0]])
    tl = torch.tensor([7, 4, 1, 0])
    for K in (1, 4):
        _check(x, tr, lex, lm, il, K, INF, tg=tg, tl=tl, what="repeat")
    # seven raw labels, four merged: the windows of F_t are those of the merged target
    a = _ref(x, tr, lex, lm, il, 1, INF, tg=tg, tl=tl)[3]
    b = _ref(x, tr, lex, lm, il, 1, INF, tg=torch.tensor([[0, 1, 4, 2, 0, 0, 0]] * 4), tl=torch.tensor([4, 0, 0, 0]))[3]
    assert a[0] == b[0] and sum(len(u) for u in a[0]) > 7


@functools.lru_cache(maxsize=None)
def wide_lexicon_and_lm():
    from torch_asg_amd import Lexicon
    rng = np.random.default_rng(5)
    words, seen = [], set()
    while len(words) < 300:
        n = int(rng.integers(1, 4))
        w = tuple(int(t) for t in rng.integers(0, 39, n))
        if w in seen or any(a == b for a, b in zip(w, w[1:])):
            continue
        seen.add(w)
        words.append(list(w))
    return Lexicon(words, 40, 39), arpa_lm(300, 2, 72, keep=(1.0, 0.03))


@DTYPES
@pytest.mark.parametrize("K", [16, 17, 32, 33, 63, 64, 65, 128, 129, 256, 257, 512, 513])
def test_set_sizes_around_the_wavefront_and_the_lanes_per_pair(K, dtype):
    """|U_{t-1}| = K exactly in a frame that has a successor: 63 / 64 / 65 around a wavefront; 16 / 17, 32 / 33, 64 / 65, 128 / 129,
    256 / 257 and 512 / 513 are where the lanes per source pair of the forward and the backward halve (64 -> 32 -> ... -> 1)."""
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(5, 2, 40, 33, dtype)
    info = {}
    _, (_, _, _, U) = _check(x * 0.25, tr * 0.25, lex, lm, torch.tensor([5, 4]), K, INF, (0.5, -0.2, 0.1), info=info, what="sizes")
    assert max(max(s) for s in info["sizes"]) == K
    assert any(len(u) == K for Ub in U for u in Ub[:-1])   # a source set of exactly K pairs: G = lanes(K) in both directions


@DTYPES
def test_more_than_1024_pairs_in_a_frame(dtype):
    """The k0 loops of the forward and the backward take a second pass over the source pairs."""
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(5, 2, 40, 33, dtype)
    _, (Z, _, _, U) = _check(x * 0.25, tr * 0.25, lex, lm, torch.tensor([5, 4]), 1200, INF, (0.5, -0.2, 0.1), what="wide")
    assert max(len(u) for Ub in U for u in Ub[:-1]) > 1024 and np.isfinite(Z).all()


@pytest.mark.parametrize("N", [89, 90, 142, 143])
@DTYPES
def test_count_tile_in_lds_and_in_scratch(N, dtype):
    """[N][N] u64 beside a small lattice: from N = 90 on the backward asks for more than 64 KiB of LDS; it fits 160 KiB up to
    N = 142; from 143 on the tile lives in the utterance's scratch."""
    A = _asg()
    words = [[i, (i * 7 + 3) % (N - 1)] for i in range(0, N - 1, 5) if i != (i * 7 + 3) % (N - 1)] + [[1], [2, 1]]
    lex = A.Lexicon(words, N, N - 1)
    lm = arpa_lm(len(words), 2, 73, keep=(1.0, 0.1))
    x, tr = _normal(6, 2, N, 40, dtype)
    tg = torch.tensor([words[0] + [N - 1] + words[-1], [2, 1, N - 1, 1, 0]])
    tl = torch.tensor([5, 4])
    M = 8 + 5
    e = 4 if dtype == torch.float32 else 8
    lds = 256 + ((M * (8 + e) + 15) // 16 * 16) + N * 8 + N * N * 8
    assert (lds <= 160 * 1024) == (N <= 142) and (lds > 64 * 1024) == (N >= 90)
    _check(x, tr, lex, lm, torch.tensor([6, 5]), 8, INF, tg=tg, tl=tl, gs=torch.tensor([1.0, -2.0]), what="tile N=%d" % N)


@DTYPES
def test_both_sides_of_the_bound_on_the_lattice_set(dtype):
    A = _asg()
    lex, lm, x, tr, il, tg, tl = grid_case(2, dtype)
    e = 4 if dtype == torch.float32 else 8
    mmax = (160 * 1024 - 256) // (16 + e)
    nf = 5                                                 # min(S, T)
    _check(x, tr, lex, lm, il, mmax - nf, INF, tg=tg, tl=tl, what="M = bound")
    with pytest.raises(RuntimeError, match="unsupported|limit|support"):
        A.beam_words_full_score(x.to(DEV), tr.to(DEV), lex, lm, il.to(DEV), mmax - nf + 1, INF, *W, tg.to(DEV), tl.to(DEV))
    _check(x[:, :2], tr, lex, lm, il[:2], min(mmax, 8192), INF, what="M = bound, no targets")


def test_lengths_1_2_3_64_65_in_one_batch():
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 2, 65)
    x, tr = _normal(65, 5, 5, 41, torch.float64)
    il = torch.tensor([1, 2, 3, 64, 65])
    tg = torch.tensor([[2, 0, 0, 0, 0], [2, 4, 0, 0, 0], [0, 1, 4, 0, 0], TARGET, TARGET])
    tl = torch.tensor([1, 2, 3, 5, 5])
    (Z, _, _), _ = _check(x * 0.5, tr * 0.5, lex, lm, il, 6, INF, tg=tg, tl=tl, gs=torch.tensor([1.0, 2.0, -1.0, 0.5, 1.5]), what="lengths")
    assert np.isfinite(Z).all()


def test_more_frames_than_one_grid_axis_holds():
    """The sets kernel strides 65535 workgroups over the frames of an utterance: 65540 frames take a second round.  Z_K alone is
    compared: over this many frames the float64 restatement's own rounding of alpha and beta (about T * 2^-53 * max|alpha|
    = 2e-7 in the exponent of every posterior) is above the 1e-9 of the gradient comparison; a set missed or misplaced beyond
    frame 65534 changes Z_K by far more than its tolerance."""
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 2, 65)
    x, tr = _normal(65540, 1, 5, 43, torch.float64)
    Z, gx, gtr = _gpu(x * 0.5, tr * 0.5, lex, lm, None, 2, INF)
    info = {}
    want = _ref(x * 0.5, tr * 0.5, lex, lm, None, 2, INF, info=info)
    assert min(info["sizes"][0]) == 2 and np.isfinite(want[0]).all()
    _close(Z, want[0], torch.float64, "Z over 65540 frames")
    assert np.isfinite(gx).all() and np.isfinite(gtr).all() and (gx[-1].sum() > 0.5)


@DTYPES
def test_a_beam_that_empties(dtype):
    lex, lm, x, tr, il, tg, tl = grid_case(2, dtype)
    x = x.clone()
    x[3, 0, :] = -INF                                      # no candidate survives frame 3 of utterance 0
    info = {}
    (Z, gx, gtr), _ = _check(x, tr, lex, lm, il, 4, INF, tg=tg, tl=tl, info=info, what="empties")
    assert info["sizes"][0][3] == 0 and Z[0] == -np.inf and (gx[:, 0] == 0).all() and np.isfinite(Z[1])


# ---------------------------------------------------------------------------------------------------------------- equivalences
@DTYPES
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_the_whole_beam_in_eighths_equals_the_static_composition_on_the_device(order, dtype):
    A = _asg()
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = without_unigrams(eighths(arpa_lm(5, order, 40 + order)), {3})
    static = A.TokenGraph(*compose_static(lex, lm))
    g = torch.Generator().manual_seed(35)
    x = (torch.randint(-32, 32, (8, 4, 5), generator=g) / 8.0).to(dtype)
    tr = (torch.randint(-16, 16, (5, 5), generator=g) / 8.0).to(dtype)
    il = torch.tensor([8, 5, 1, 0])
    gs = torch.tensor([1.0, -0.5, 2.0, 3.0])
    Z, gx, gtr = _gpu(x, tr, lex, lm, il, ALL, INF, (1.0, 0.0, 0.125), gs=gs)
    xd, trd = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
    Zf = A.graph_full_score(xd, trd, static, il.to(DEV), 1.0, 0.125)
    Zf.backward(gs.to(DEV).to(Zf.dtype))
    _close(Z, Zf.detach().cpu().numpy(), dtype, "Z")
    _close(gx, xd.grad.cpu().numpy(), dtype, "grad_inputs")
    _close(gtr, trd.grad.cpu().numpy(), dtype, "grad_transition")
    assert np.isfinite(Z[:3]).all()


@DTYPES
def test_the_null_lm_equals_the_token_automaton_loss(dtype):
    A = _asg()
    lex, _, x, tr, il, tg, tl = grid_case(2, dtype)
    null = A.WordLM.null(5)
    for K, theta in ((1, INF), (3, INF), (7, 1.5), (ALL, INF)):
        for t_, l_ in ((None, None), (tg, tl)):
            Z, gx, gtr = _gpu(x, tr, lex, null, il, K, theta, (1.0, 0.0, -0.3), t_, l_)
            xd, trd = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
            Zg = A.beam_graph_full_score(xd, trd, lex.graph, il.to(DEV), K, theta, 1.0, -0.3, None if t_ is None else t_.to(DEV),
                                         None if l_ is None else l_.to(DEV))
            Zg.backward(torch.ones_like(Zg))
            _close(Z, Zg.detach().cpu().numpy(), dtype, "Z K=%d" % K)
            _close(gx, xd.grad.cpu().numpy(), dtype, "grad_inputs K=%d" % K)
            _close(gtr, trd.grad.cpu().numpy(), dtype, "grad_transition K=%d" % K)


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _bits(ts):
    return [t.detach().cpu().numpy().tobytes() for t in ts]


def test_two_runs_give_identical_bits_and_groups_equal_one_call():
    A = _asg()
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(12, 6, 40, 36, torch.float32)
    il = torch.tensor([12, 3, 0, 1, 11, 7])
    tg = torch.tensor([[3, 7, 39, 11, 2, 39]] * 6)
    tl = torch.tensor([6, 3, 3, 1, 6, 0])
    gs = torch.tensor([1.0, 2.0, 3.0, -1.0, 0.5, 1.5])
    w = (0.5, -0.2, 0.1)
    a = _gpu(x * 0.25, tr, lex, lm, il, 300, 6.0, w, tg, tl, gs)
    assert np.isfinite(a[0][[0, 1, 3, 4, 5]]).all()
    for _ in range(2):
        b = _gpu(x * 0.25, tr, lex, lm, il, 300, 6.0, w, tg, tl, gs)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    from torch_asg_amd.asg import native
    be = native()
    seen = []
    buf = be._buf
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    try:
        _gpu(x * 0.25, tr, lex, lm, il, 300, 6.0, w, tg, tl, gs)
        per = max(seen) // 6
        seen.clear()
        small = _gpu(x * 0.25, tr, lex, lm, il, 300, 6.0, w, tg, tl, gs, max_work_bytes=2 * per + per // 2)
        assert seen.count(2 * per) == 3                    # three groups of two utterances, each keeps its alpha
    finally:
        del be._buf
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, small))
    # half precision widens as the other losses do; a warm call compiles nothing
    xh = (x * 0.25).to(torch.bfloat16)
    u = A.beam_words_full_score(xh.to(DEV), tr.to(DEV), lex, lm, il.to(DEV), 50, INF, *w)
    v = A.beam_words_full_score(xh.float().to(DEV), tr.to(DEV), lex, lm, il.to(DEV), 50, INF, *w)
    assert torch.equal(u, v)
    assert lm.compile(DEV, torch.float32, 0.5, -0.2) is lm.compile(DEV, torch.float32, 0.5, -0.2)
    assert lex.compile_words(DEV, torch.float32, 0.1) is lex.compile_words(DEV, torch.float32, 0.1)


def test_capture_and_replay_with_new_emissions_and_lengths():
    A = _asg()
    lex, lm, x0, tr, _, tg, tl = grid_case(3, torch.float32)
    T, B, N = 7, 4, 5
    x = torch.zeros(T, B, N, device=DEV, requires_grad=True)
    trd = tr.to(DEV).requires_grad_(True)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)
    tgd, tld = tg.to(DEV), tl.to(DEV)
    gs = torch.tensor([1.0, -0.5, 2.0, 3.0], device=DEV)

    def step():
        Z = A.beam_words_full_score(x, trd, lex, lm, il, 6, 3.0, *W, tgd, tld)
        gx, gtr = torch.autograd.grad(Z, (x, trd), gs)
        return Z.detach(), gx, gtr
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                             # warm-up: compiles and caches lexicon and LM
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
        want = beam_word_loss_ref(x.detach().cpu().numpy(), tr.numpy(), lex, lm, il.cpu().numpy(), 6, 3.0, *W, tg.numpy(),
                                  tld.cpu().numpy(), gs.cpu().numpy())
        for n, u, w_ in zip(("Z", "gx", "gtr"), out, want):
            _close(u.cpu().numpy(), w_, torch.float32, "replay %d %s" % (seed, n))


def test_the_other_entry_points_are_undisturbed_by_a_loss_call():
    A = _asg()
    lex, lm, x, tr, il, tg, tl = grid_case(3, torch.float32)
    xd, trd, ild, tgd, tld = x.to(DEV), tr.to(DEV), il.to(DEV), tg.to(DEV), tl.to(DEV)

    def others():
        out = list(A.beam_decode_words(xd, trd, lex, lm, ild, 6, 4.0, *W))
        out += [o for o in A.beam_decode_words_nbest(xd, trd, lex, lm, ild, 6, 3, 4.0, *W) if o is not None]
        out.append(A.beam_graph_asg_loss(xd, tgd, trd, lex.graph, ild, tld, 6, 4.0, 0.8, -0.5))
        return [o.cpu() for o in out]
    before = others()
    xg = xd.clone().requires_grad_(True)
    A.beam_words_asg_loss(xg, tgd, trd, lex, lm, ild, tld, 64, 4.0, *W)[:2].sum().backward()
    after = others()
    for u, v in zip(before, after):
        assert torch.equal(u, v)


def test_the_module_method_reductions_and_an_upstream_parameter():
    A = _asg()
    lex, lm, x, tr, il, tg, tl = grid_case(2, torch.float32)
    il, tl = torch.tensor([7, 5, 6, 7]), torch.tensor([5, 4, 1, 2])
    crit = {r: A.ASGLoss(5, reduction=r).to(DEV) for r in ("none", "sum", "mean")}
    for c in crit.values():
        with torch.no_grad():
            c.transition.copy_(tr.to(DEV))
    lin = torch.nn.Linear(5, 5).to(DEV)
    args = (tg.to(DEV), lex, lm, il.to(DEV), tl.to(DEV), *W)
    per = crit["none"].beam_word_loss(lin(x.to(DEV)), *args, beam_size=4, beam_threshold=5.0)
    fn = A.beam_words_asg_loss(lin(x.to(DEV)), tg.to(DEV), crit["none"].transition, lex, lm, il.to(DEV), tl.to(DEV), 4, 5.0, *W)
    assert per.shape == (4,) and torch.isfinite(per).all() and (per >= -1e-4).all() and torch.equal(per, fn)
    tot = crit["sum"].beam_word_loss(lin(x.to(DEV)), *args, beam_size=4, beam_threshold=5.0)
    mean = crit["mean"].beam_word_loss(lin(x.to(DEV)), *args, beam_size=4, beam_threshold=5.0)
    assert torch.allclose(tot, per.sum(), rtol=1e-5) and torch.allclose(mean, per.mean(), rtol=1e-5)
    mean.backward()
    assert lin.weight.grad is not None and torch.isfinite(lin.weight.grad).all() and lin.weight.grad.abs().sum() > 0
    assert crit["mean"].transition.grad is not None and crit["mean"].transition.grad.abs().sum() > 0
