"""GPU tests (-m gpu) of the word confidences and end frames of the word-LM beam decoder
(`torch_asg_amd.beam_decode_words_confidence`, csrc/asg_beam_word_conf.hip).  The decoder's eight fields are compared byte for
byte with the device's own `beam_decode_words`, the normalisers bit for bit with the device's `beam_words_full_score` without
targets; word_frames exactly and word_confidences within tests/test_hip_beam_word_loss.py's rule (float64 rtol = atol = 1e-9,
float32 tests/util.py::assert_close, the padding exact) with the numpy restatement (tests/beam_word_conf_ref.py, pinned on the
CPU by tests/test_beam_word_conf_cpu.py).  Every case first asserts, from the restatement, that its input is in the regime it
names."""
import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, small_lexicon
from beam_word_conf_ref import beam_word_conf_ref
from test_beam_word_conf_cpu import double_completion_case
from test_beam_word_la_cpu import rescue_case
from test_hip_beam_word_loss import ALL, DEV, DTYPES, INF, W, _close, _normal, grid_case, wide_lexicon_and_lm

pytestmark = pytest.mark.gpu
WW = (0.5, -0.2, 0.1)                                      # the weights of the wide cases
DECODE = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths")


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _d(t):
    return None if t is None else t.to(DEV)


def _run(x, tr, lex, lm, il, K, theta=INF, w=W, tol=0, la=None, **kw):
    r = _asg().beam_decode_words_confidence(_d(x), _d(tr), lex, lm, _d(il), K, theta, *w, tol, lookahead=la, **kw)
    torch.cuda.synchronize()
    return r


def _bits(ts):
    return [t.detach().cpu().numpy().tobytes() for t in ts]


def _check(x, tr, lex, lm, il, K, theta=INF, w=W, tol=0, la=None, info=None, what="", identities=True, **kw):
    """One call against the device's own decoder and normaliser (bits) and against the restatement (values) -> (got, want)."""
    A = _asg()
    T, B, _ = x.shape
    got = _run(x, tr, lex, lm, il, K, theta, w, tol, la, **kw)
    what = "%s K=%d theta=%s tol=%d order=%s" % (what, K, theta, tol, la and la.order)
    assert got.word_frames.shape == (B, T) and got.word_frames.dtype == torch.int64
    assert got.word_confidences.shape == (B, T) and got.word_confidences.dtype == x.dtype
    assert got.normalisers.shape == (B,) and got.normalisers.dtype == x.dtype
    if identities:
        dec = A.beam_decode_words(_d(x), _d(tr), lex, lm, _d(il), K, theta, *w, lookahead=la)
        for n in DECODE:
            assert torch.equal(getattr(got, n), getattr(dec, n)) and getattr(got, n).dtype == getattr(dec, n).dtype, (n, what)
        Z = A.beam_words_full_score(_d(x), _d(tr), lex, lm, _d(il), K, theta, *w, lookahead=la)
        assert _bits([got.normalisers]) == _bits([Z]), what
    want = beam_word_conf_ref(x.numpy(), tr.numpy(), lex, lm, None if il is None else il.numpy(), K, theta, *w, tol,
                              None if la is None else la.order, info)
    wf, cf = got.word_frames.cpu().numpy(), got.word_confidences.cpu().numpy()
    assert np.array_equal(got.word_lengths.cpu().numpy(), want["word_lengths"]), what
    assert np.array_equal(got.words.cpu().numpy(), want["words"]), what
    assert np.array_equal(wf, want["word_frames"]), what
    pad = np.arange(T)[None, :] >= want["word_lengths"][:, None]
    assert (cf[pad] == 0).all() and (wf[pad] == -1).all() and not np.isnan(cf).any(), what
    _close(cf, want["word_confidences"], x.dtype, "word_confidences " + what)
    _close(got.normalisers.cpu().numpy(), want["normalisers"], x.dtype, "normalisers " + what)
    return got, want


# ---------------------------------------------------------------------------------------------------------------- grid
@DTYPES
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_grid_of_beams_thresholds_and_tolerances(order, dtype):
    lex, lm, x, tr, il, _, _ = grid_case(order, dtype)
    unsure = moved = 0
    for K in (1, 3, 8, ALL):
        for theta in (INF, 2.0):
            base = None
            for tol in (0, 1, 3, 64):
                got, want = _check(x, tr, lex, lm, il, K, theta, tol=tol, what="grid", identities=tol == 0)
                assert want["normalisers"][3] == -np.inf and want["word_lengths"][2] == 1 and want["word_frames"][2, 0] == 1
                assert got.normalisers[3].item() == -INF and got.scores[3].item() == -INF and (got.word_frames[3] == -1).all()
                c = want["word_confidences"]
                if tol == 0:
                    base = c
                    unsure += int(((c > 0) & (c < 0.999)).sum())
                    if K == 1:
                        assert (c[want["word_frames"] >= 0] > 1 - 1e-12).all()
                else:
                    assert (c >= base - 1e-12).all()
                    moved += int((c > base + 1e-6).sum())
    assert unsure > 10 and moved > 10                      # confidences below 1, and windows that gather more than the frame


# ---------------------------------------------------------------------------------------------------------------- shapes
@DTYPES
@pytest.mark.parametrize("K", [32, 33, 63, 64, 65])
def test_source_sets_where_the_lanes_per_pair_halve_and_around_a_wavefront(K, dtype):
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(5, 2, 40, 33, dtype)
    info = {}
    got, want = _check(x * 0.25, tr * 0.25, lex, lm, torch.tensor([5, 4]), K, INF, WW, tol=1, info=info, what="sizes")
    assert max(max(s) for s in info["sizes"]) == K
    assert any(len(u) == K for Ub in want["sets"] for u in Ub[:-1])        # a source set of exactly K pairs
    assert (want["word_lengths"] >= 1).all() and (want["word_confidences"] < 0.999)[want["word_frames"] >= 0].any()


@DTYPES
def test_more_than_1024_pairs_in_a_frame(dtype):
    """The k0 loop of the pull takes a second pass over the source pairs."""
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(5, 2, 40, 33, dtype)
    _, want = _check(x * 0.25, tr * 0.25, lex, lm, torch.tensor([5, 4]), 1200, INF, WW, tol=0, what="wide")
    assert max(len(u) for Ub in want["sets"] for u in Ub[:-1]) > 1024 and (want["word_lengths"] >= 1).all()
    assert (want["word_confidences"] < 0.9)[want["word_frames"] >= 0].any()


@pytest.mark.parametrize("N", [141, 142])
def test_wide_alphabets_in_float64(N):
    """The transitions of the search leave LDS between these two alphabets at K = 8 (4096 + 16 K + 8 N^2 bytes against 160 KiB):
    both instantiations of the search with its end run."""
    A = _asg()
    words = [[i, (i * 7 + 3) % (N - 1)] for i in range(0, N - 1, 5) if i != (i * 7 + 3) % (N - 1)] + [[1], [2, 1]]
    lex = A.Lexicon(words, N, N - 1)
    lm = arpa_lm(len(words), 2, 73, keep=(1.0, 0.1))
    x, tr = _normal(4, 2, N, 40, torch.float64)
    _, want = _check(x, tr, lex, lm, torch.tensor([4, 3]), 8, INF, tol=1, what="N=%d" % N)
    assert (want["word_lengths"] >= 1).all()


def test_long_utterances_with_lengths_around_a_wavefront():
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 2, 65)
    x, tr = _normal(130, 4, 5, 41, torch.float64)
    x = x * 0.5
    for t in range(130):                                   # "0 1", separator, "2", separator, ...: two words every five frames
        x[t, :, [0, 1, 4, 2, 4][t % 5]] += 2.0
    il = torch.tensor([63, 64, 65, 129])
    for tol in (0, 64):
        _, want = _check(x, tr * 0.5, lex, lm, il, 6, INF, tol=tol, what="lengths", identities=tol == 0)
        assert (want["word_lengths"] > 8).all() and (want["word_lengths"][3] > 20)
        assert (want["word_frames"][:, 0] >= 1).all()
        if tol == 64:                                      # many words share one window: the scan of the open range, not one slot
            f = want["word_frames"][3, :want["word_lengths"][3]]
            assert max(int(((f >= t - 64) & (f <= t + 64)).sum()) for t in f) > 20 and want["word_confidences"].max() > 5


@DTYPES
def test_a_beam_that_ends_mid_word_and_one_that_empties(dtype):
    lex, lm, x, tr = rescue_case(np.float32 if dtype == torch.float32 else np.float64)
    x = torch.from_numpy(np.concatenate([x, x, x], axis=1)).clone()
    x[1, 2, :] = -INF                                      # utterance 2: no candidate survives frame 1
    info = {}
    got, want = _check(x, torch.from_numpy(tr), lex, lm, torch.tensor([3, 1, 3]), ALL, INF, (1.0, 0.0, 0.0), tol=2, info=info,
                       what="no end")
    assert info["sizes"][1] == [1] and info["sizes"][2][1] == 0        # one kept pair, mid-word; an empty beam
    for b in (1, 2):
        assert want["normalisers"][b] == -np.inf and got.scores[b].item() == -INF and got.normalisers[b].item() == -INF
        assert (got.word_frames[b] == -1).all() and (got.word_confidences[b] == 0).all() and got.word_lengths[b].item() == 0
        assert (got.path[b] == -1).all()
    assert 0.5 < want["word_confidences"][0, 0] < 1.0


@DTYPES
def test_a_short_word_completed_twice_inside_the_window(dtype):
    lex, lm, x, tr = double_completion_case(np.float32 if dtype == torch.float32 else np.float64)
    x, tr = torch.from_numpy(x), torch.from_numpy(tr)
    for tol, above in ((0, False), (1, False), (2, True)):
        got, want = _check(x, tr, lex, lm, None, ALL, INF, (1.0, 0.0, 0.0), tol=tol, what="twice")
        assert list(want["word_frames"][0, :2]) == [1, 3] and ((want["word_confidences"][0, :2] > 1.2).all() == above)
        assert (got.word_confidences[0, :2] > 1.2).all().item() == above       # unclipped


@DTYPES
@pytest.mark.parametrize("order", [1, 2])
def test_look_ahead_sets_with_plain_weights(order, dtype):
    A = _asg()
    lex, lm, x, tr, il, _, _ = grid_case(3, dtype)
    la = A.WordLookahead(lex, lm, order)
    differ = 0
    for K, theta in ((2, INF), (3, INF), (8, 2.0)):
        _, want = _check(x, tr, lex, lm, il, K, theta, tol=1, la=la, what="look-ahead")
        plain = beam_word_conf_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), K, theta, *W, 1)
        differ += want["sets"] != plain["sets"]
    assert differ == 3                                     # the regime: not the plain search's lattice
    # the rescued word of a beam of one: sure of it, and normalised by its plain score
    lex, lm, x, tr = rescue_case(np.float32 if dtype == torch.float32 else np.float64)
    got, want = _check(torch.from_numpy(x), torch.from_numpy(tr), lex, lm, None, 1, INF, (1.0, 0.0, 0.0),
                       la=A.WordLookahead(lex, lm, order), what="rescue")
    assert want["words"][0, 0] == 1 and abs(got.word_confidences[0, 0].item() - 1.0) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_two_runs_give_identical_bits_and_groups_equal_one_call():
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(12, 6, 40, 36, torch.float32)
    il = torch.tensor([12, 3, 0, 1, 11, 7])
    a = _run(x * 0.25, tr, lex, lm, il, 300, 6.0, WW, 2)
    assert torch.isfinite(a.normalisers[[0, 1, 4, 5]]).all() and (a.word_confidences > 0).sum() >= 5
    assert ((a.word_confidences > 0) & (a.word_confidences < 0.99)).any()
    for _ in range(2):
        assert _bits(_run(x * 0.25, tr, lex, lm, il, 300, 6.0, WW, 2)) == _bits(a)
    from torch_asg_amd.asg import native
    be = native()
    seen = []
    buf = be._buf
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    try:
        _run(x * 0.25, tr, lex, lm, il, 300, 6.0, WW, 2)
        per = max(seen) // 6
        seen.clear()
        small = _run(x * 0.25, tr, lex, lm, il, 300, 6.0, WW, 2, max_work_bytes=2 * per + per // 2)
        assert seen == [2 * per]                           # three groups of two utterances through one workspace
    finally:
        del be._buf
    assert _bits(small) == _bits(a)
    la = _asg().WordLookahead(lex, lm, 2)
    b = _run(x * 0.25, tr, lex, lm, il, 300, 6.0, WW, 2, la)
    assert _bits(_run(x * 0.25, tr, lex, lm, il, 300, 6.0, WW, 2, la, max_work_bytes=per)) == _bits(b)


def test_capture_and_three_replays_on_fresh_emissions_and_lengths():
    A = _asg()
    lex, lm, _, tr, _, _, _ = grid_case(3, torch.float32)
    T, B, N = 7, 4, 5
    x = torch.zeros(T, B, N, device=DEV)
    trd = tr.to(DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)

    def step():
        return A.beam_decode_words_confidence(x, trd, lex, lm, il, 6, 3.0, *W, 1)
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
        want = beam_word_conf_ref(x.cpu().numpy(), tr.numpy(), lex, lm, il.cpu().numpy(), 6, 3.0, *W, 1)
        assert np.array_equal(out.word_frames.cpu().numpy(), want["word_frames"])
        _close(out.word_confidences.cpu().numpy(), want["word_confidences"], torch.float32, "replay %d" % seed)


def test_the_neighbours_are_unchanged_after_a_confidence_call():
    A = _asg()
    lex, lm, x, tr, il, tg, tl = grid_case(3, torch.float32)
    xd, trd, ild, tgd, tld = x.to(DEV), tr.to(DEV), il.to(DEV), tg.to(DEV), tl.to(DEV)

    def others():
        out = list(A.beam_decode_words(xd, trd, lex, lm, ild, 6, 4.0, *W))
        out += [o for o in A.beam_decode_words_nbest(xd, trd, lex, lm, ild, 6, 3, 4.0, *W) if o is not None]
        xg = xd.clone().requires_grad_(True)
        loss = A.beam_words_asg_loss(xg, tgd, trd, lex, lm, ild, tld, 6, 4.0, *W)
        loss[:2].sum().backward()
        out += [loss.detach(), xg.grad]
        return [o.cpu() for o in out]
    before = others()
    A.beam_decode_words_confidence(xd, trd, lex, lm, ild, 64, 4.0, *W, 3)
    A.ASGLoss(5).to(DEV).beam_decode_words_confidence(xd, lex, lm, ild, 6, 4.0, *W, frame_tolerance=1)
    for u, v in zip(before, others()):
        assert torch.equal(u, v)
    with pytest.raises(RuntimeError, match="asg_beam_words_confidence"):
        A.beam_decode_words_confidence(xd, trd, lex, lm, ild, 6, 4.0, *W, 65)
    with pytest.raises(RuntimeError, match="asg_beam_words_confidence"):
        A.beam_decode_words_confidence(xd, trd, lex, lm, ild, 6, 4.0, *W, -1)
