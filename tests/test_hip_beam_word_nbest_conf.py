"""GPU tests (-m gpu) of the word confidences and end frames of every row of the word-LM beam decoder's n-best list
(`torch_asg_amd.beam_decode_words_nbest_confidence`, csrc/asg_beam_word_nbest_conf.hip).  In every case

  the twelve n-best fields are compared byte for byte with the device's own `beam_decode_words_nbest`,
  the normalisers bit for bit with the device's `beam_words_full_score` without targets,
  row 0's frames and confidences bit for bit with the device's `beam_decode_words_confidence`,
  word_frames exactly and word_confidences within tests/test_hip_beam_word_loss.py's rule (float64 rtol = atol = 1e-9, float32
  tests/util.py::assert_close, the padding exact) with the numpy restatement (tests/beam_word_nbest_conf_ref.py, pinned on the
  CPU by tests/test_beam_word_nbest_conf_cpu.py),

and rows that read one cell carry one value.  Every case first asserts, from the restatement, that its input is in the regime
it names.  The sizes named here are DESIGN.md 5y's: the prep kernel sorts up to 2048 queries in LDS and more in the workspace;
the ring has P2(min(nbest, K) * (2 tol + 2)) slots; the word filter has 256 bits over word mod 256."""
import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, small_lexicon
from beam_word_nbest_conf_ref import beam_word_nbest_conf_ref
from beam_word_nbest_ref import NAMES
from test_beam_word_conf_cpu import double_completion_case
from test_beam_word_la_cpu import rescue_case
from test_hip_beam_word_loss import ALL, DEV, DTYPES, INF, W, _close, _normal, grid_case, wide_lexicon_and_lm

pytestmark = pytest.mark.gpu
WW = (0.5, -0.2, 0.1)                                      # the weights of the wide cases
SORT_LDS = 2048                                            # kBeamWordNbestConfSortLds
FILTER_BITS = 256


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _d(t):
    return None if t is None else t.to(DEV)


def _p2(n):
    r = 2
    while r < n:
        r *= 2
    return r


def fits(elem, K, nbest, tol):
    """The one new limit, as include/asg_hip.h states it (M = K)."""
    return 16 * ((K * (elem + 8) + 15) // 16) + 1024 + 12 * _p2(min(nbest, K) * (2 * tol + 2)) <= 163840


def _run(x, tr, lex, lm, il, K, nbest, theta=INF, w=W, tol=0, la=None, **kw):
    kw.setdefault("return_alignments", True)
    r = _asg().beam_decode_words_nbest_confidence(_d(x), _d(tr), lex, lm, _d(il), K, nbest, theta, *w, tol, lookahead=la, **kw)
    torch.cuda.synchronize()
    return r


def _bits(ts):
    return [None if t is None else t.detach().cpu().numpy().tobytes() for t in ts]


def _check(x, tr, lex, lm, il, K, nbest, theta=INF, w=W, tol=0, la=None, info=None, what="", identities=True, want=None, **kw):
    """One call against the device's own n-best list, normaliser and one-best confidences (bits) and against the restatement
    (values) -> (got, want).  `want`: a restatement of the same arguments with at least `nbest` rows (its first rows are used)."""
    A = _asg()
    T, B, _ = x.shape
    got = _run(x, tr, lex, lm, il, K, nbest, theta, w, tol, la, **kw)
    what = "%s K=%d nbest=%d theta=%s tol=%d order=%s" % (what, K, nbest, theta, tol, la and la.order)
    assert got.word_frames.shape == (B, nbest, T) and got.word_frames.dtype == torch.int64
    assert got.word_confidences.shape == (B, nbest, T) and got.word_confidences.dtype == x.dtype
    assert got.normalisers.shape == (B,) and got.normalisers.dtype == x.dtype
    one = A.beam_decode_words_confidence(_d(x), _d(tr), lex, lm, _d(il), K, theta, *w, tol, lookahead=la)
    assert torch.equal(got.word_frames[:, 0], one.word_frames), what
    assert _bits([got.word_confidences[:, 0].contiguous()]) == _bits([one.word_confidences]), what
    assert _bits([got.normalisers]) == _bits([one.normalisers]), what
    if identities:
        nb = A.beam_decode_words_nbest(_d(x), _d(tr), lex, lm, _d(il), K, nbest, theta, *w, return_alignments=True, lookahead=la)
        for n in NAMES:
            assert getattr(got, n).dtype == getattr(nb, n).dtype and _bits([getattr(got, n)]) == _bits([getattr(nb, n)]), (n, what)
        Z = A.beam_words_full_score(_d(x), _d(tr), lex, lm, _d(il), K, theta, *w, lookahead=la)
        assert _bits([got.normalisers]) == _bits([Z]), what
    if want is None:
        want = beam_word_nbest_conf_ref(x.numpy(), tr.numpy(), lex, lm, None if il is None else il.numpy(), K, nbest, theta, *w, tol,
                                        None if la is None else la.order, info)
    wl, ww = want["word_lengths"][:, :nbest], want["words"][:, :nbest]
    wwf, wcf = want["word_frames"][:, :nbest], want["word_confidences"][:, :nbest]
    wf, cf = got.word_frames.cpu().numpy(), got.word_confidences.cpu().numpy()
    assert np.array_equal(got.num_hyps.cpu().numpy(), np.minimum(want["num_hyps"], nbest)), what
    assert np.array_equal(got.word_lengths.cpu().numpy(), wl) and np.array_equal(got.words.cpu().numpy(), ww), what
    assert np.array_equal(wf, wwf), what
    pad = np.arange(T)[None, None, :] >= wl[:, :, None]
    assert (cf[pad] == 0).all() and (wf[pad] == -1).all() and not np.isnan(cf).any(), what
    _close(cf, wcf, x.dtype, "word_confidences " + what)
    _close(got.normalisers.cpu().numpy(), want["normalisers"], x.dtype, "normalisers " + what)
    words = got.words.cpu().numpy()
    for b in range(B):                                     # rows that hold the same word ending at the same frame: the same bits
        seen = {}
        for r, k in zip(*np.nonzero(wf[b] >= 0)):
            assert seen.setdefault((int(wf[b, r, k]), int(words[b, r, k])), cf[b, r, k].tobytes()) == cf[b, r, k].tobytes(), what
    if tol == 0:                                           # a row's path is a lattice path that has the event
        eps = 1e-3 if x.dtype == torch.float32 else 1e-9   # the rounding of two sums of up to 2 T terms of size <= ~100
        sc, Z = got.scores.cpu().numpy().astype(np.float64), got.normalisers.cpu().numpy().astype(np.float64)
        for b, r, k in zip(*np.nonzero(wf >= 0)):
            assert np.exp(sc[b, r] - Z[b]) * (1 - eps) <= cf[b, r, k] <= 1 + eps, (what, b, r, k)
    return got, want


# ---------------------------------------------------------------------------------------------------------------- grid
@DTYPES
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_grid_of_beams_thresholds_rows_and_tolerances(order, dtype):
    lex, lm, x, tr, il, _, _ = grid_case(order, dtype)
    elem = 4 if dtype == torch.float32 else 8
    shared = below = refused = padded = 0
    for K in (1, 3, 8, ALL):
        for theta in (INF, 2.0):
            for tol in (0, 1, 3, 64):
                want = beam_word_nbest_conf_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), K, 64, theta, *W, tol)
                assert want["normalisers"][3] == -np.inf and want["num_hyps"][3] == 0 and want["num_hyps"][2] >= 1
                for nbest in (1, 2, 8, 64):
                    if not fits(elem, K, nbest, tol):
                        with pytest.raises(RuntimeError, match="asg_beam_words_nbest_confidence"):
                            _run(x, tr, lex, lm, il, K, nbest, theta, W, tol)
                        refused += 1
                        continue
                    got, _ = _check(x, tr, lex, lm, il, K, nbest, theta, tol=tol, what="grid", identities=tol == 0, want=want)
                    assert got.normalisers[3].item() == -INF and got.num_hyps[3].item() == 0
                    assert (got.word_frames[3] == -1).all() and (got.word_confidences[3] == 0).all()
                    padded += int((want["num_hyps"] < nbest).any())
                if tol == 0:
                    shared += sum(q - len(c) for q, c in zip(want["queries"], want["cells"]))
                    c = want["word_confidences"]
                    below += int(((c > 0) & (c < 0.999)).sum())
    # the regime: cells shared between rows, confidences below 1, padding rows, and the limit refused where it is passed
    assert shared > 20 and below > 20 and padded > 20 and refused == 2


# ---------------------------------------------------------------------------------------------------------------- the ring
def _long_case(dtype=torch.float64, order=3):
    """T = 130, lengths 63 / 64 / 65 / 129; "0 1", separator, "2", separator, ...: two words every five frames."""
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, order, 65)
    x, tr = _normal(130, 4, 5, 41, dtype)
    x = x * 0.5
    for t in range(130):
        x[t, :, [0, 1, 4, 2, 4][t % 5]] += 2.0
    return lex, lm, x, tr * 0.5, torch.tensor([63, 64, 65, 129])


_LONG = {}


def _long_want(K, nbest, tol):
    """The restatement of the long case at `nbest` rows and tolerance `tol`, computed once per setting."""
    key = (K, nbest, tol)
    if key not in _LONG:
        lex, lm, x, tr, il = _long_case()
        _LONG[key] = beam_word_nbest_conf_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), K, nbest, INF, *W, tol)
    return _LONG[key]


def test_a_ring_of_four_wraps_many_times():
    """nbest = 2 at tol = 0: a ring of 4 slots on utterances with far more than 4 cells."""
    lex, lm, x, tr, il = _long_case()
    want = _long_want(64, 48, 0)
    assert _p2(2 * 2) == 4
    first_two = [len({(int(f), int(w)) for r in range(2) for f, w in zip(want["word_frames"][b, r], want["words"][b, r]) if f >= 0})
                 for b in range(4)]
    assert min(first_two) > 20
    _check(x, tr, lex, lm, il, 64, 2, what="ring of 4", want=want)


@pytest.mark.parametrize("nbest,tol", [(4, 1), (5, 1), (8, 3), (9, 3)])
def test_rows_times_window_at_a_power_of_two_and_one_row_above(nbest, tol):
    lex, lm, x, tr, il = _long_case()
    want = _long_want(64, 48, tol)
    need = nbest * (2 * tol + 2)
    assert (want["num_hyps"] >= 9).all() and ((need & (need - 1)) == 0) == (nbest in (4, 8))
    # several cells are open at once: some 2 tol + 2 neighbouring frames, what the ring holds at a step, have four or more
    got, _ = _check(x, tr, lex, lm, il, 64, nbest, tol=tol, what="power of two", want=want)
    f = got.word_frames[3].cpu().numpy()
    cells = sorted({(int(f[r, k]), int(got.words[3, r, k])) for r, k in zip(*np.nonzero(f >= 0))})
    fr = np.array([c[0] for c in cells])
    assert max(int(((fr >= t) & (fr < t + 2 * tol + 2)).sum()) for t in fr) >= 4


# ---------------------------------------------------------------------------------------------------------------- the sort
@pytest.mark.parametrize("nbest", [8, 30, 48])
def test_query_counts_below_at_and_above_the_sort_in_lds(nbest):
    """The utterance of 129 frames ends about 50 words per row: with 8 rows the network sorts 512 slots in LDS, with 30 rows the
    2048 slots that are the most LDS takes, with 48 rows 4096 slots in the workspace -- while the short utterances of the same
    call still sort in LDS."""
    lex, lm, x, tr, il = _long_case()
    want = _long_want(64, 48, 1)
    q = [int(want["word_lengths"][b, :nbest].sum()) for b in range(4)]
    assert (want["num_hyps"] >= 48).all()
    if nbest == 8:
        assert max(q) <= 512
    elif nbest == 30:
        assert SORT_LDS // 2 < q[3] <= SORT_LDS
    else:
        assert q[3] > SORT_LDS and min(q) <= SORT_LDS
    got, _ = _check(x, tr, lex, lm, il, 64, nbest, tol=1, what="sort", want=want)
    assert (got.word_lengths[3, :nbest] > 20).all()


@DTYPES
def test_wide_lexicon_with_64_rows_and_certain_filter_collisions(dtype):
    """300 words over a filter of 256 bits: words w and w + 256 share a bit.  T = 40, 64 rows."""
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(40, 2, 40, 37, dtype)
    il = torch.tensor([40, 37])
    got, want = _check(x * 0.5, tr * 0.25, lex, lm, il, 96, 64, 8.0, WW, tol=1, what="wide")
    assert lex.num_words > FILTER_BITS and (want["num_hyps"] >= 32).all()
    for b in range(2):
        mine = {w for _, w in want["cells"][b]}
        others = {w for w, _ in want["events"][b]} - mine
        assert {w % FILTER_BITS for w in others} & {w % FILTER_BITS for w in mine}, "an event passes the filter and finds no cell"
        assert len(want["cells"][b]) < want["queries"][b]


# ---------------------------------------------------------------------------------------------------------------- shapes
@DTYPES
@pytest.mark.parametrize("K", [63, 64, 65])
def test_source_sets_around_a_wavefront(K, dtype):
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(5, 2, 40, 33, dtype)
    info = {}
    got, want = _check(x * 0.25, tr * 0.25, lex, lm, torch.tensor([5, 4]), K, 10, INF, WW, tol=1, info=info, what="sizes")
    assert max(max(s) for s in info["sizes"]) == K
    assert any(len(u) == K for Ub in want["sets"] for u in Ub[:-1])        # a source set of exactly K pairs
    assert (want["num_hyps"] >= 3).all() and (want["word_confidences"] < 0.999)[want["word_frames"] >= 0].any()


def test_long_utterances_with_lengths_around_a_wavefront():
    lex, lm, x, tr, il = _long_case()
    for tol in (0, 64):
        want = _long_want(6, 4, tol)
        _check(x, tr, lex, lm, il, 6, 4, tol=tol, what="lengths", identities=tol == 0, want=want)
        assert (want["word_lengths"][:, :2] > 8).all() and (want["word_lengths"][3, :2] > 20).all() and (want["num_hyps"] >= 2).all()
        assert (want["word_frames"][:, 1, 0] >= 1).all()
        if tol == 64:
            assert want["word_confidences"][:, 1].max() > 5


@DTYPES
def test_a_beam_that_ends_mid_word_and_one_that_empties(dtype):
    lex, lm, x, tr = rescue_case(np.float32 if dtype == torch.float32 else np.float64)
    x = torch.from_numpy(np.concatenate([x, x, x], axis=1)).clone()
    x[1, 2, :] = -INF                                      # utterance 2: no candidate survives frame 1
    info = {}
    got, want = _check(x, torch.from_numpy(tr), lex, lm, torch.tensor([3, 1, 3]), ALL, 4, INF, (1.0, 0.0, 0.0), tol=2, info=info,
                       what="no end")
    assert info["sizes"][1] == [1] and info["sizes"][2][1] == 0        # one kept pair, mid-word; an empty beam
    for b in (1, 2):
        assert want["normalisers"][b] == -np.inf and got.num_hyps[b].item() == 0 and got.normalisers[b].item() == -INF
        assert (got.word_frames[b] == -1).all() and (got.word_confidences[b] == 0).all() and (got.word_lengths[b] == 0).all()
        assert (got.path[b] == -1).all() and (got.scores[b] == -INF).all()
    assert want["num_hyps"][0] >= 2 and 0.0 < want["word_confidences"][0, 1, 0] < 1.0


@DTYPES
def test_a_short_word_completed_twice_on_a_lower_row(dtype):
    lex, lm, x, tr = double_completion_case(np.float32 if dtype == torch.float32 else np.float64)
    x, tr = torch.from_numpy(x), torch.from_numpy(tr)
    above = []
    for tol in (0, 2):
        got, want = _check(x, tr, lex, lm, None, ALL, 8, INF, (1.0, 0.0, 0.0), tol=tol, what="twice")
        assert want["num_hyps"][0] >= 2
        above.append(bool((want["word_confidences"][0, 1:] > 1.2).any()))
        assert bool((got.word_confidences[0, 1:] > 1.2).any().item()) == above[-1]         # unclipped
    assert above == [False, True]


@DTYPES
@pytest.mark.parametrize("order", [1, 2])
def test_look_ahead_rows_with_plain_weights(order, dtype):
    A = _asg()
    lex, lm, x, tr, il, _, _ = grid_case(3, dtype)
    la = A.WordLookahead(lex, lm, order)
    differ = 0
    for K, theta in ((2, INF), (3, INF), (8, 2.0)):
        _, want = _check(x, tr, lex, lm, il, K, 8, theta, tol=1, la=la, what="look-ahead")
        plain = beam_word_nbest_conf_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), K, 8, theta, *W, 1)
        differ += want["sets"] != plain["sets"]
    assert differ == 3                                     # the regime: not the plain search's lattice


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_two_runs_give_identical_bits_and_groups_equal_one_call():
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(12, 6, 40, 36, torch.float32)
    il = torch.tensor([12, 3, 0, 1, 11, 7])
    a = _run(x * 0.25, tr, lex, lm, il, 300, 20, 6.0, WW, 2)
    assert torch.isfinite(a.normalisers[[0, 1, 4, 5]]).all() and (a.num_hyps[[0, 4, 5]] >= 5).all()
    assert ((a.word_confidences > 0) & (a.word_confidences < 0.99)).any()
    for _ in range(2):
        assert _bits(_run(x * 0.25, tr, lex, lm, il, 300, 20, 6.0, WW, 2)) == _bits(a)
    from torch_asg_amd.asg import native
    be = native()
    seen = []
    buf = be._buf
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    try:
        _run(x * 0.25, tr, lex, lm, il, 300, 20, 6.0, WW, 2)
        whole = max(seen)
        seen.clear()
        small = _run(x * 0.25, tr, lex, lm, il, 300, 20, 6.0, WW, 2, max_work_bytes=whole // 2)
        assert len(seen) == 1 and seen[0] < whole          # several groups of utterances through one smaller workspace
    finally:
        del be._buf
    assert _bits(small) == _bits(a)
    la = _asg().WordLookahead(lex, lm, 2)
    b = _run(x * 0.25, tr, lex, lm, il, 300, 20, 6.0, WW, 2, la)
    assert _bits(_run(x * 0.25, tr, lex, lm, il, 300, 20, 6.0, WW, 2, la, max_work_bytes=whole // 4)) == _bits(b)
    c = _run(x * 0.25, tr, lex, lm, il, 300, 20, 6.0, WW, 2, return_alignments=False)
    assert c.path is None and c.states is None and c.lm_states is None
    assert _bits([t for t in c if t is not None]) == _bits([t for n, t in zip(a._fields, a) if n not in ("path", "states", "lm_states")])


def test_capture_and_three_replays_on_fresh_emissions_and_lengths():
    A = _asg()
    lex, lm, _, tr, _, _, _ = grid_case(3, torch.float32)
    T, B, N = 7, 4, 5
    x = torch.zeros(T, B, N, device=DEV)
    trd = tr.to(DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)

    def step():
        return A.beam_decode_words_nbest_confidence(x, trd, lex, lm, il, 6, 4, 3.0, *W, 1, True)
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
        x.copy_(torch.randn(T, B, N, generator=gen))
        il.copy_(torch.tensor([T, 4 + seed % 2, 1, T - seed]))
        gr.replay()
        torch.cuda.synchronize()
        assert _bits(out) == _bits(step())
        want = beam_word_nbest_conf_ref(x.cpu().numpy(), tr.numpy(), lex, lm, il.cpu().numpy(), 6, 4, 3.0, *W, 1)
        assert np.array_equal(out.word_frames.cpu().numpy(), want["word_frames"])
        _close(out.word_confidences.cpu().numpy(), want["word_confidences"], torch.float32, "replay %d" % seed)


def test_the_neighbours_are_unchanged_after_an_nbest_confidence_call():
    A = _asg()
    lex, lm, x, tr, il, tg, tl = grid_case(3, torch.float32)
    xd, trd, ild, tgd, tld = x.to(DEV), tr.to(DEV), il.to(DEV), tg.to(DEV), tl.to(DEV)

    def others():
        out = list(A.beam_decode_words(xd, trd, lex, lm, ild, 6, 4.0, *W))
        out += [o for o in A.beam_decode_words_nbest(xd, trd, lex, lm, ild, 6, 3, 4.0, *W) if o is not None]
        out += list(A.beam_decode_words_confidence(xd, trd, lex, lm, ild, 6, 4.0, *W, 1))
        xg = xd.clone().requires_grad_(True)
        loss = A.beam_words_asg_loss(xg, tgd, trd, lex, lm, ild, tld, 6, 4.0, *W)
        loss[:2].sum().backward()
        out += [loss.detach(), xg.grad]
        return [o.cpu() for o in out]
    before = others()
    A.beam_decode_words_nbest_confidence(xd, trd, lex, lm, ild, 64, 5, 4.0, *W, 3)
    A.ASGLoss(5).to(DEV).beam_decode_words_nbest_confidence(xd, lex, lm, ild, 6, 3, 4.0, *W, frame_tolerance=1)
    for u, v in zip(before, others()):
        assert torch.equal(u, v)
    for bad in (dict(frame_tolerance=65), dict(frame_tolerance=-1), dict(nbest=8193)):
        kw = dict(beam_size=6, nbest=3, beam_threshold=4.0, frame_tolerance=0)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="asg_beam_words_nbest_confidence"):
            A.beam_decode_words_nbest_confidence(xd, trd, lex, lm, ild, **kw)
