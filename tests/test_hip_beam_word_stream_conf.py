"""GPU tests (-m gpu) of the lattice-keeping word-LM beam stream (`torch_asg_amd.BeamWordStream(..., keep_lattice=True)`;
csrc/asg_beam_word_stream_conf.hip).  `result_confidence(final=True)` is held BIT FOR BIT to the device's own
`beam_decode_words_confidence` on the whole utterance (with the stream's look-ahead, if it has one), for every chunking and every
placement of confidence calls; the prefix results are held to the numpy restatement tests/beam_word_stream_conf_ref.py under
tests/test_hip_beam_word_conf.py's rule (its `_close`: float64 rtol = atol = 1e-9, float32 util.assert_close; frames, integers
and padding exact); `result` and `result_nbest` are byte-equal to a plain `BeamWordStream` fed the same chunks.  Every case first
asserts from a restatement that its input is in the regime it names."""
import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, small_lexicon
from beam_word_conf_ref import beam_word_conf_ref
from beam_word_stream_conf_ref import BeamWordStreamConfRef
from test_beam_word_conf_cpu import double_completion_case
from test_beam_word_la_cpu import rescue_case
from test_hip_beam_word_loss import ALL, DEV, DTYPES, INF, W, _close, _normal, wide_lexicon_and_lm

pytestmark = pytest.mark.gpu
WW = (0.5, -0.2, 0.1)                                      # the weights of the wide cases (tests/test_hip_beam_word_conf.py's)
WL = (0.05, 0.05, 0.0)                                     # ... of the long cases: a frame adds about nothing to Z
WIDE = ("path", "tokens", "states", "lm_states", "words", "word_frames")
TEN = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths", "frames", "status")
LETTERS = [0.5, -1.0, 0.0, 2.0, -0.25]


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _np(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def _stream(tr, lex, lm, B, M, K, th=INF, w=W, keep=True, la=None):
    return _asg().BeamWordStream(tr.to(DEV), lex, lm, B, M, K, th, *w, dtype=tr.dtype, device=DEV, lookahead=la, keep_lattice=keep)


def _ref(tr, lex, lm, B, M, K, th=INF, w=W, la=None):
    return BeamWordStreamConfRef(tr.numpy(), lex, lm, B, M, K, th, *w, dtype=_np(tr.dtype), order=None if la is None else la.order)


def _chunks(x, lens, cuts):
    """x [T,B,N] with lengths lens in chunks of `cuts` frames -> [(chunk, chunk_lengths)]."""
    out, a = [], 0
    for n in cuts:
        out.append((x[a:a + n], torch.clamp(lens - a, 0, n)))
        a += n
    return out


def _split(x, lens, seed):
    """Two chunks of Tc = ceil(T / 2) frames in which slot b takes its first s_b frames from the first and the rest from the second:
    per-slot lengths inside one Tc."""
    T, B, N = x.shape
    Tc = (T + 1) // 2
    g = torch.Generator().manual_seed(seed)
    sp = torch.tensor([int(torch.randint(max(0, int(l) - Tc), min(int(l), Tc) + 1, (1,), generator=g)) for l in lens])
    c1, c2 = torch.zeros_like(x[:Tc]), torch.zeros_like(x[:Tc])
    for b in range(B):
        s, l = int(sp[b]), int(lens[b])
        c1[:s, b] = x[:s, b]
        c2[:l - s, b] = x[s:l, b]
    return [(c1, sp), (c2, lens - sp)]


def _feed(s, chunks, after=None):
    for i, (c, cl) in enumerate(chunks):
        s.advance(c.to(DEV), cl.to(DEV))
        if after is not None:
            after(i)


def _bits(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in ts if t is not None]


def _host(r):
    torch.cuda.synchronize()
    return {n: getattr(r, n).cpu().numpy() for n in r._fields}


def _equal_one_shot(got, one, T, what):
    """A stream result [B, M] against the device's one-shot result [B, T]: bits on the one-shot's columns, padding beyond."""
    g, o = _host(got), _host(one)
    for n in ("scores", "normalisers", "token_lengths", "word_lengths"):
        assert g[n].dtype == o[n].dtype and g[n].tobytes() == o[n].tobytes(), (what, n)
    for n in WIDE:
        assert np.array_equal(g[n][:, :T], o[n]) and (g[n][:, T:] == -1).all(), (what, n)
    assert np.ascontiguousarray(g["word_confidences"][:, :T]).tobytes() == o["word_confidences"].tobytes(), what
    assert (g["word_confidences"][:, T:] == 0).all(), what


def _equal_ref(got, want, dtype, what):
    """A stream result [B, M] against a restatement's [B, Tw], Tw <= M (the stream's, or the one-shot's over Tw frames):
    integers, frames and padding exact, the real fields under the rule."""
    g = _host(got)
    Tw = want["path"].shape[1]
    for n in WIDE:
        assert np.array_equal(g[n][:, :Tw], want[n]) and (g[n][:, Tw:] == -1).all(), (what, n)
    for n in ("token_lengths", "word_lengths") + (("frames", "status") if "frames" in want else ()):
        assert np.array_equal(g[n], want[n]), (what, n)
    cf = g["word_confidences"]
    behind = np.arange(cf.shape[1])[None, :] >= want["word_lengths"][:, None]
    assert (cf[behind] == 0).all() and not np.isnan(cf).any(), what
    _close(cf[:, :Tw], want["word_confidences"], dtype, "word_confidences %s" % (what,))
    for n in ("scores", "normalisers"):
        _close(g[n], want[n], dtype, "%s %s" % (n, what))


def _one_shot(x, tr, lex, lm, lens, K, th, tol, w=W, la=None):
    return _asg().beam_decode_words_confidence(x.to(DEV), tr.to(DEV), lex, lm, lens.to(DEV), K, th, *w, tol, lookahead=la)


def _grid(order, dtype):
    lex = small_lexicon(LETTERS)
    lm = arpa_lm(5, order, 60 + order, keep=(1.0, 0.5, 0.5))
    T, B = 24, 5
    x, tr = _normal(T, B, 5, 31, dtype)
    return lex, lm, x, tr, torch.tensor([T, 0, 1, 17, 9])


# ---------------------------------------------------------------------------------------------------------------- (a) the grid
@DTYPES
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_final_is_the_one_shot_call_bit_for_bit_for_every_chunking_and_placement(order, dtype):
    lex, lm, x, tr, lens = _grid(order, dtype)
    T, B, M = 24, 5, 26
    info = {}
    want = beam_word_conf_ref(x.numpy(), tr.numpy(), lex, lm, lens.numpy(), 3, INF, *W, 0, info=info)
    assert any(s == 3 for s in info["sizes"][0])                           # the beam of 3 prunes
    assert np.isfinite(want["normalisers"][[0, 2, 3, 4]]).all() and want["normalisers"][1] == -np.inf
    c = want["word_confidences"][want["word_frames"] >= 0]
    assert ((c > 0.01) & (c < 0.99)).any()                                 # words the lattice is not sure of
    if order == 3:                                                         # two histories on one q in a kept set
        assert any(len({q for _, q in u}) < len(u) for u in want["sets"][0])
    tols = (0, 1, 3, 64)
    chunkings = [_chunks(x, lens, [1] * T), _chunks(x, lens, [T]), _chunks(x, lens, [1, 7, 0, 16]), _split(x, lens, 5)]
    for K in (1, 3, 8, ALL):
        for th in (INF, 2.0):
            one = {tol: _one_shot(x, tr, lex, lm, lens, K, th, tol) for tol in tols}
            for ci, chunks in enumerate(chunkings):
                what = (order, K, th, ci)
                s = _stream(tr, lex, lm, B, M, K, th)                      # result_confidence only at the end
                _feed(s, chunks)
                for tol in tols:
                    _equal_one_shot(s.result_confidence(tol, final=True), one[tol], T, what + (tol, "end"))
                s = _stream(tr, lex, lm, B, M, K, th)                      # ... and after every chunk, both modes, every tolerance
                _feed(s, chunks, lambda i: s.result_confidence(tols[i % 4], final=bool(i % 2)))
                for tol in tols:
                    _equal_one_shot(s.result_confidence(tol, final=True), one[tol], T, what + (tol, "every"))


@DTYPES
@pytest.mark.parametrize("order", [1, 2])
def test_final_with_a_look_ahead_is_the_one_shot_call_with_that_look_ahead(order, dtype):
    A = _asg()
    lex, lm, x, tr, lens = _grid(3, dtype)
    T, B, M = 24, 5, 26
    la = A.WordLookahead(lex, lm, order)
    tols = (0, 1, 3, 64)
    chunkings = [_chunks(x, lens, [1] * T), _chunks(x, lens, [T]), _chunks(x, lens, [1, 7, 0, 16]), _split(x, lens, 5)]
    differ = 0
    for K, th in ((2, INF), (3, INF), (8, 2.0)):
        want = beam_word_conf_ref(x.numpy(), tr.numpy(), lex, lm, lens.numpy(), K, th, *W, 1, order=order)
        plain = beam_word_conf_ref(x.numpy(), tr.numpy(), lex, lm, lens.numpy(), K, th, *W, 1)
        differ += want["sets"] != plain["sets"]
        one = {tol: _one_shot(x, tr, lex, lm, lens, K, th, tol, la=la) for tol in tols}
        for ci, chunks in enumerate(chunkings):
            s = _stream(tr, lex, lm, B, M, K, th, la=la)
            _feed(s, chunks, (lambda i: s.result_confidence(tols[i % 4], final=bool(i % 2))) if ci % 2 == 0 else None)
            for tol in tols:
                _equal_one_shot(s.result_confidence(tol, final=True), one[tol], T, (order, K, th, ci, tol))
            _equal_ref(s.result_confidence(1, final=True), want, dtype, (order, K, th, ci, "ref"))
    assert differ == 3                                                     # the regime: not the plain search's lattice
    # the rescued word of a beam of one: sure of it
    lex, lm, xr, trr = rescue_case(_np(dtype))
    xr, trr = torch.from_numpy(xr), torch.from_numpy(trr)
    s = _stream(trr, lex, lm, 1, 3, 1, w=(1.0, 0.0, 0.0), la=A.WordLookahead(lex, lm, order))
    _feed(s, _chunks(xr, torch.tensor([3]), [2, 1]), lambda i: s.result_confidence(0))
    got = s.result_confidence(0, final=True)
    _equal_one_shot(got, _one_shot(xr, trr, lex, lm, torch.tensor([3]), 1, INF, 0, (1.0, 0.0, 0.0), A.WordLookahead(lex, lm, order)),
                    3, "rescue")
    assert got.words[0, 0].item() == 1 and abs(got.word_confidences[0, 0].item() - 1.0) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- (b), (c)
@DTYPES
@pytest.mark.parametrize("order", [None, 1, 2], ids=["plain", "la1", "la2"])
def test_prefix_results_after_every_chunk_and_the_plain_results_of_the_stream(order, dtype):
    A = _asg()
    lex = small_lexicon(LETTERS)
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    la = None if order is None else A.WordLookahead(lex, lm, order)
    T, B, M = 12, 4, 13
    x, tr = _normal(T, B, 5, 33, dtype)
    lens = torch.tensor([T, 0, 1, 7])
    for K, th in ((3, INF), (8, 2.0)):
        chunks = _chunks(x, lens, [1, 4, 0, 7])
        s, plain = _stream(tr, lex, lm, B, M, K, th, la=la), _stream(tr, lex, lm, B, M, K, th, keep=False, la=la)
        ref, full = _ref(tr, lex, lm, B, M, K, th, la=la), _ref(tr, lex, lm, B, M, ALL, INF, la=la)
        pruned = midword = 0
        for i, (c, cl) in enumerate(chunks):
            s.advance(c.to(DEV), cl.to(DEV))
            plain.advance(c.to(DEV), cl.to(DEV))
            ref.advance(c.numpy(), cl.numpy())
            full.advance(c.numpy(), cl.numpy())
            for tol in (0, 2):
                want = ref.result_confidence(tol, final=False)
                _equal_ref(s.result_confidence(tol, final=False), want, dtype, (order, K, th, i, tol))
                L = want["frames"]
                assert (want["word_frames"] < np.maximum(L, 1)[:, None]).all()      # no event at frame L in prefix mode
            last = want["path"][np.arange(B), np.maximum(L - 1, 0)]
            midword += int(((L > 0) & (last >= 0) & (last != lex.separator)).sum())
            pruned += ref.sizes()[0] != full.sizes()[0]                    # (by the beam or by the threshold)
            for final in (False, True):                                    # result and result_nbest: a plain stream's bytes
                assert _bits(s.result(final)) == _bits(plain.result(final))
                got = s.result_confidence(1, final=final)
                assert _bits([getattr(got, n) for n in TEN]) == _bits(plain.result(final))
                assert _bits(s._result_nbest(3, final, True)) == _bits(plain._result_nbest(3, final, True))
        assert pruned and midword                                          # a pruning beam; prefixes that end inside a word
        s.reset()
        plain.reset()
        assert _bits(s.result()) == _bits(plain.result())
    if la is not None:
        with pytest.raises(NotImplementedError):
            s.result_nbest(3)                                              # the public method keeps raising


# ---------------------------------------------------------------------------------------------------------------- (d) the shapes
def _both_modes(lex, lm, x, tr, lens, K, M, cuts, tols, w=W, what="", calls=(), th=INF):
    """One stream over `cuts`, confidence calls after the chunks in `calls`: final against the one-shot call's bits and, with the
    prefix, against the restatement -> the restatement."""
    dtype, T, B = x.dtype, x.shape[0], x.shape[1]
    s, ref = _stream(tr, lex, lm, B, M, K, th, w), _ref(tr, lex, lm, B, M, K, th, w)
    for i, (c, cl) in enumerate(_chunks(x, lens, cuts)):
        s.advance(c.to(DEV), cl.to(DEV))
        ref.advance(c.numpy(), cl.numpy())
        if i in calls:
            s.result_confidence(tols[0], final=False)
    for tol in tols:
        got = s.result_confidence(tol, final=True)
        _equal_one_shot(got, _one_shot(x, tr, lex, lm, lens, K, th, tol, w), T, (what, tol))
        _equal_ref(got, ref.result_confidence(tol, final=True), dtype, (what, tol, "final"))
        _equal_ref(s.result_confidence(tol, final=False), ref.result_confidence(tol, final=False), dtype, (what, tol, "prefix"))
    return ref


@DTYPES
@pytest.mark.parametrize("K", [32, 33, 63, 64, 65])
def test_kept_sets_around_the_subgroup_steps_and_the_bitonic_power_of_two(K, dtype):
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(5, 2, 40, 33, dtype)
    ref = _both_modes(lex, lm, x * 0.25, tr * 0.25, torch.tensor([5, 4]), K, 5, [2, 3], (1,), WW, "sizes", calls=(0,))
    sizes = ref.sizes()
    assert max(max(z) for z in sizes) == K and sum(z == K for b in range(2) for z in sizes[b][:-1]) >= 2
    r = ref.result_confidence(1, final=True)
    assert (r["word_lengths"] >= 1).all() and (r["word_confidences"] < 0.999)[r["word_frames"] >= 0].any()


@DTYPES
def test_more_than_1024_kept_pairs_in_a_frame(dtype):
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(5, 2, 40, 33, dtype)
    ref = _both_modes(lex, lm, x * 0.25, tr * 0.25, torch.tensor([5, 4]), 1200, 6, [3, 2], (0,), WW, "wide", calls=(0,))
    assert max(z for b in range(2) for z in ref.sizes()[b][:-1]) > 1024
    r = ref.result_confidence(0, final=True)
    assert (r["word_lengths"] >= 1).all() and (r["word_confidences"] < 0.9)[r["word_frames"] >= 0].any()


@pytest.mark.parametrize("N", [141, 142])
def test_wide_alphabets_in_float64_on_both_layouts_of_the_frame(N):
    """The transitions of the search leave LDS between these two alphabets at K = 8 (4096 + 16 K + 8 N^2 bytes against 160 KiB):
    both instantiations of the advance run."""
    A = _asg()
    words = [[i, (i * 7 + 3) % (N - 1)] for i in range(0, N - 1, 5) if i != (i * 7 + 3) % (N - 1)] + [[1], [2, 1]]
    lex = A.Lexicon(words, N, N - 1)
    lm = arpa_lm(len(words), 2, 73, keep=(1.0, 0.1))
    x, tr = _normal(4, 2, N, 40, torch.float64)
    ref = _both_modes(lex, lm, x, tr, torch.tensor([4, 3]), 8, 4, [1, 3], (1,), W, "N=%d" % N, calls=(0,))
    assert (4096 + 16 * 8 + 8 * N * N <= 160 * 1024) == (N == 141)
    assert (ref.result_confidence(1, final=True)["word_lengths"] >= 1).all()


def test_lengths_around_a_wavefront_with_many_words_in_one_window():
    lex = small_lexicon(LETTERS)
    lm = arpa_lm(5, 2, 65)
    x, tr = _normal(130, 4, 5, 41, torch.float64)
    x = x * 0.5
    for t in range(130):                                   # "0 1", separator, "2", separator, ...: two words every five frames
        x[t, :, [0, 1, 4, 2, 4][t % 5]] += 2.0
    ref = _both_modes(lex, lm, x, tr * 0.5, torch.tensor([63, 64, 65, 129]), 6, 130, [40, 90], (0, 64), W, "M=130", calls=(0,))
    r = ref.result_confidence(64, final=True)
    assert (r["word_lengths"] > 8).all() and r["word_lengths"][3] > 20
    f = r["word_frames"][3, :r["word_lengths"][3]]
    assert max(int(((f >= t - 64) & (f <= t + 64)).sum()) for t in f) > 20 and r["word_confidences"].max() > 5


def _one_letter_case(T, B, dtype, seed):
    """Three one-letter words and the separator; the emissions favour letter, separator, letter, separator, ... by 6, and the
    weights are small: a word every two frames, and the running sums stay small."""
    A = _asg()
    lex = A.Lexicon([[0], [1], [2]], 4, 3)
    lm = arpa_lm(3, 2, 67)
    g = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(T, B, 4, generator=g, dtype=torch.float64) - 6.0
    letters = torch.randint(0, 3, (T, B), generator=g)
    for t in range(T):
        for b in range(B):
            x[t, b, int(letters[t, b]) if t % 2 == 0 else 3] = 0.0
    return lex, lm, x.to(dtype), torch.zeros(4, 4, dtype=dtype)


@DTYPES
def test_the_ring_wraps_behind_word_256(dtype):
    lex, lm, x, tr = _one_letter_case(600, 2, dtype, 16)
    ref = _both_modes(lex, lm, x, tr, torch.tensor([600, 560]), 4, 600, [200, 400], (0, 64), WL, "M=600")
    r = ref.result_confidence(0, final=True)
    assert np.abs(r["normalisers"]).max() < 32                             # the running sums did stay small
    assert int(r["word_lengths"][0]) > 257 and int(r["word_lengths"][1]) > 257               # a word index above 256


# ---------------------------------------------------------------------------------------------------------------- (e)
@DTYPES
def test_a_catch_up_that_starts_at_frame_0_at_frame_1_and_at_the_last_frame(dtype):
    lex = small_lexicon(LETTERS)
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    T, B = 9, 3
    x, tr = _normal(T, B, 5, 35, dtype)
    lens = torch.tensor([T, T, 6])
    one = _one_shot(x, tr, lex, lm, lens, 6, 4.0, 1)
    ref = _ref(tr, lex, lm, B, T, 6, 4.0)
    ref.advance(x.numpy(), lens.numpy())
    assert any(z == 6 for z in ref.sizes()[0])
    for calls in ((), (0,), (0, 1), (1,)):          # ranges [0, 9); [0, 1) [1, 9); [0, 1) [1, 8) [8, 9); [0, 8) [8, 9)
        s = _stream(tr, lex, lm, B, T, 6, 4.0)
        _feed(s, _chunks(x, lens, [1, T - 2, 1]), lambda i: s.result_confidence(0, final=True) if i in calls else None)
        _equal_one_shot(s.result_confidence(1, final=True), one, T, calls)
        _equal_one_shot(s.result_confidence(1, final=True), one, T, calls)                    # caught up: nothing to do


@DTYPES
def test_a_beam_that_empties_inside_a_chunk_on_its_first_and_on_its_last_frame(dtype):
    lex = small_lexicon(LETTERS)
    lm = arpa_lm(5, 2, 9)
    x, tr = _normal(8, 3, 5, 18, dtype)
    lens = torch.tensor([8, 8, 3])
    x[4:, 0] = -INF                                                        # slot 0: every candidate of frame 4 is -inf
    ref = _ref(tr, lex, lm, 3, 8, 3)
    ref.advance(x.numpy(), lens.numpy())
    assert ref.sizes()[0][3] == 3 and ref.sizes()[0][4:] == [0, 0, 0, 0]
    one = _one_shot(x, tr, lex, lm, lens, 3, INF, 2)
    for cuts in ([8], [2, 6], [4, 4], [5, 3]):                             # frame 4: inside, inside, first, last of its chunk
        s = _stream(tr, lex, lm, 3, 8, 3)
        _feed(s, _chunks(x, lens, cuts), lambda i: s.result_confidence(2, final=False))
        got = s.result_confidence(2, final=True)
        _equal_one_shot(got, one, 8, cuts)
        _equal_ref(got, ref.result_confidence(2, final=True), dtype, cuts)
        pre = s.result_confidence(2, final=False)
        _equal_ref(pre, ref.result_confidence(2, final=False), dtype, (cuts, "prefix"))
        assert pre.scores[0].item() == -INF and pre.normalisers[0].item() == -INF and pre.word_lengths[0].item() == 0
        assert (pre.word_frames[0] == -1).all() and (pre.word_confidences[0] == 0).all() and (pre.path[0] == -1).all()
        assert not torch.isnan(pre.word_confidences).any()


@DTYPES
@pytest.mark.parametrize("order", [None, 2], ids=["plain", "la2"])
def test_the_plain_stream_and_the_lattice_keeping_one_run_one_advance(order, dtype):
    """The two states are advanced by ONE kernel text (csrc/asg_beam_word_stream.hip, with and without the keep policy, with and
    without the look-ahead flag): for the same chunks `result(final=False)`, `result(final=True)` and the two best of the n-best
    list are the same bytes, at the smallest shape that reaches every branch of the shared loop.  A two-word lexicon (0 1 and 2,
    separator 3: N = 4) with a bigram; B = 3, max_frames = 6, beam_size = 3, a finite threshold; chunks of 1, 2 and 4 frames with
    per-slot lengths (1, 1, 1), (2, 2, 1), (4, 4, 2).  Checked with tests/beam_word_stream_ref.py and
    tests/beam_word_la_stream_ref.py (through the restatement that derives from them), and asserted below from it: slots 0 and 1
    are offered 7 > 6 frames, take 3 of the last chunk's 4 and set `status`; slot 2 takes 4 frames and does not; slot 1, whose
    emissions are -inf from frame 2 on, keeps 2, 3, 0, 0, 0, 0 pairs -- its beam empties on the second frame of the second chunk
    and skips the third chunk from its first frame, the only slot whose beam empties --, and slots 0 and 2 keep 2 pairs in frame
    0, 3 in every later frame, and have a finite best prefix after every chunk."""
    A = _asg()
    B, M, K, th = 3, 6, 3, 6.0
    lex = A.Lexicon([[0, 1], [2]], 4, 3)
    lm = arpa_lm(2, 2, 7)
    la = None if order is None else A.WordLookahead(lex, lm, order)
    x, tr = _normal(7, B, 4, 41, dtype)
    x[2:, 1] = -INF
    chunks = [(x[0:1], torch.tensor([1, 1, 1])), (x[1:3], torch.tensor([2, 2, 1])), (x[3:7], torch.tensor([4, 4, 2]))]
    ref = _ref(tr, lex, lm, B, M, K, th, la=la)
    s, plain = _stream(tr, lex, lm, B, M, K, th, la=la), _stream(tr, lex, lm, B, M, K, th, keep=False, la=la)
    for i, (c, cl) in enumerate(chunks):
        ref.advance(c.numpy(), cl.numpy())
        for st in (s, plain):
            st._fed = 0                                    # (the host's bound counts offered frames; the device's clamp is the subject)
            st.advance(c.to(DEV), cl.to(DEV))
        assert np.isfinite(ref.result(False)["scores"]).tolist() == [True, i < 1, True]
        for final in (False, True):
            a, b = s.result(final), plain.result(final)
            assert _bits(a) == _bits(b), (i, final)
            assert torch.isfinite(a.scores).cpu().numpy().tolist() == np.isfinite(ref.result(final)["scores"]).tolist()
            assert _bits(s._result_nbest(2, final, True)) == _bits(plain._result_nbest(2, final, True)), (i, final)
    assert ref.sizes() == [[2, 3, 3, 3, 3, 3], [2, 3, 0, 0, 0, 0], [2, 3, 3, 3]]
    got, want = s.result(), ref.result()
    assert got.frames.tolist() == [6, 6, 4] == want["frames"].tolist() and got.status.tolist() == [1, 1, 0] == want["status"].tolist()
    conf = s.result_confidence(1, final=False)             # (the catch-up reads the kept counts of the skipped frames: 0)
    assert conf.normalisers[1].item() == -INF and torch.isfinite(conf.normalisers[[0, 2]]).all()


@DTYPES
def test_the_end_rule_at_the_last_frame_the_unfinished_word_and_the_double_completion(dtype):
    lex, lm, x, tr = rescue_case(_np(dtype))                               # 0, 1 | 2, separator
    x, tr = torch.from_numpy(x), torch.from_numpy(tr)
    w = (1.0, 0.0, 0.0)
    s, ref = _stream(tr, lex, lm, 1, 3, ALL, w=w), _ref(tr, lex, lm, 1, 3, ALL, w=w)
    s.advance(x[:2].to(DEV))
    ref.advance(x[:2].numpy())
    pre, fin = s.result_confidence(0, final=False), s.result_confidence(0, final=True)      # the same state, mid-word
    want = ref.result_confidence(0, final=True)
    assert want["word_lengths"][0] == 1 and want["word_frames"][0, 0] == 2 and 0.5 < want["word_confidences"][0, 0] < 1.0
    _equal_ref(fin, want, dtype, "end rule")
    _equal_ref(pre, ref.result_confidence(0, final=False), dtype, "mid-word")
    assert pre.word_lengths[0].item() == 0 and (pre.word_frames == -1).all() and (pre.word_confidences == 0).all()
    assert pre.token_lengths[0].item() == 2 and torch.isfinite(pre.normalisers).all()
    _equal_one_shot(fin, _one_shot(x[:2], tr, lex, lm, torch.tensor([2]), ALL, INF, 0, w), 2, "end rule")
    lex, lm, x, tr = double_completion_case(_np(dtype))
    x, tr = torch.from_numpy(x), torch.from_numpy(tr)
    for tol, above in ((0, False), (1, False), (2, True)):
        ref = _both_modes(lex, lm, x, tr, torch.tensor([4]), ALL, 4, [3, 1], (tol,), w, "twice", calls=(0,))
        for final in (False, True):
            r = ref.result_confidence(tol, final=final)
            assert list(r["word_frames"][0, :2]) == [1, 3] and ((r["word_confidences"][0, :2] > 1.2).all() == above)


# ---------------------------------------------------------------------------------------------------------------- (f) the stream
@DTYPES
def test_a_masked_reset_in_mid_stream(dtype):
    lex = small_lexicon(LETTERS)
    lm = arpa_lm(5, 3, 7)
    x, tr = _normal(8, 3, 5, 37, dtype)
    full = torch.tensor([8, 8, 8])
    s = _stream(tr, lex, lm, 3, 8, 4)
    s.advance(x[:3].to(DEV))
    s.result_confidence(0)
    s.advance(x[3:5].to(DEV))
    s.reset(torch.tensor([0, 1, 0]))
    s.advance(x[5:8].to(DEV))
    got = _host(s.result_confidence(1, final=True))
    whole = _host(_one_shot(x, tr, lex, lm, full, 4, INF, 1))
    tail = _host(_one_shot(x[5:8], tr, lex, lm, torch.tensor([3, 3, 3]), 4, INF, 1))
    assert list(got["frames"]) == [8, 3, 8]
    for b, (o, T) in enumerate([(whole, 8), (tail, 3), (whole, 8)]):
        for n in ("scores", "normalisers", "token_lengths", "word_lengths"):
            assert got[n][b].tobytes() == o[n][b].tobytes(), (b, n)
        for n in WIDE:
            assert np.array_equal(got[n][b, :T], o[n][b]) and (got[n][b, T:] == -1).all(), (b, n)
        assert got["word_confidences"][b, :T].tobytes() == o["word_confidences"][b].tobytes()
        assert (got["word_confidences"][b, T:] == 0).all()


def test_capture_with_three_replays_that_reach_and_pass_max_frames():
    lex = small_lexicon(LETTERS)
    lm = arpa_lm(5, 3, 7)
    Tc, B, N, M = 3, 3, 5, 8
    _, tr = _normal(Tc, B, N, 23, torch.float32)
    s, twin = _stream(tr, lex, lm, B, M, 6, 3.0), _stream(tr, lex, lm, B, M, 6, 3.0)
    x = torch.zeros(Tc, B, N, device=DEV)
    cl = torch.full((B,), Tc, dtype=torch.int64, device=DEV)

    def step(st):
        st.advance(x, cl)
        return st.result_confidence(1, final=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(s)                                            # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    s.reset()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = step(s)
    lengths = ([3, 3, 1], [3, 3, 0], [3, 2, 2])            # slot 0 is offered 9 > 8 frames, slot 1 reaches 8 exactly
    for k, seed in enumerate((1, 2, 3)):
        gen = torch.Generator().manual_seed(seed)
        x.copy_(torch.randn(Tc, B, N, generator=gen))
        cl.copy_(torch.tensor(lengths[k]))
        gr.replay()
        twin._fed = 0                                      # (the host's bound counts offered frames; the replays pass it by design)
        assert _bits(out) == _bits(step(twin)), k
    torch.cuda.synchronize()
    assert out.frames.tolist() == [8, 8, 3] and out.status.tolist() == [1, 0, 0]
    assert torch.isfinite(out.normalisers).all() and not torch.isnan(out.word_confidences).any()
    fin = s.result_confidence(1, final=True)
    assert _bits(fin) == _bits(twin.result_confidence(1, final=True)) and fin.status.tolist() == [1, 0, 0]


def test_two_runs_give_identical_bits():
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(12, 4, 40, 36, torch.float32)
    lens = torch.tensor([12, 3, 0, 11])

    def run():
        s = _stream(tr, lex, lm, 4, 12, 300, 6.0, WW)
        outs = []
        _feed(s, _chunks(x * 0.25, lens, [5, 0, 7]), lambda i: outs.extend(_bits(s.result_confidence(2, final=bool(i % 2)))))
        return outs + _bits(s.result_confidence(2, final=True))
    a = run()
    assert a == run() == run()


def test_the_neighbours_are_unchanged_after_the_calls():
    A = _asg()
    lex = small_lexicon(LETTERS)
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(9, 4, 5, 24, torch.float32)
    il = torch.tensor([9, 0, 1, 6])
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)

    def others():
        out = list(A.beam_decode_words(xd, trd, lex, lm, ild, 6, 4.0, *W))
        out += list(A.beam_decode_words_confidence(xd, trd, lex, lm, ild, 6, 4.0, *W, 2))
        p = _stream(tr, lex, lm, 4, 9, 6, 4.0, keep=False)
        p.advance(xd[:4], torch.clamp(ild, 0, 4))
        out += list(p.result())
        p.advance(xd[4:], torch.clamp(ild - 4, 0, 5))
        out += list(p.result(final=True)) + [o for o in p.result_nbest(3, True) if o is not None]
        return [o.cpu() for o in out]
    before = others()
    s = A.ASGLoss(5).to(DEV).beam_word_stream(lex, lm, 4, 9, 6, 4.0, *W, keep_lattice=True)
    s.advance(xd, ild)
    s.result_confidence(3)
    s.result_confidence(0, final=True)
    for u, v in zip(before, others()):
        assert torch.equal(u, v)
    for bad in (65, 1 << 40):
        with pytest.raises(RuntimeError, match="asg_beam_word_conf_stream_confidence"):
            s.result_confidence(bad)
    with pytest.raises(ValueError):
        s.result_confidence(-1)
    with pytest.raises(RuntimeError, match="keep_lattice"):
        _stream(tr, lex, lm, 4, 9, 6, keep=False).result_confidence()
    with pytest.raises(RuntimeError, match="asg_beam_word_conf_stream"):   # a beam the plain stream takes, beyond the lattice's LDS
        _stream(tr, lex, lm, 1, 2, 8180)
    assert _stream(tr, lex, lm, 1, 2, 8180, keep=False).beam_size == 8180
