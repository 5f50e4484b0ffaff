"""CPU tests that pin the numpy restatement of the lattice-keeping word-LM beam stream (tests/beam_word_stream_conf_ref.py) before
the GPU tests compare the kernels with it: `final=True` against tests/beam_word_conf_ref.py on the whole utterance, byte for byte,
for every way of cutting the utterance and of placing `result_confidence` calls between the chunks, with and without a
look-ahead; the prefix mode against the enumeration of all label paths inside the kept sets; the properties the specification
states; the edge cases of a stream.  No kernel is launched."""
import itertools

import numpy as np
import pytest

from beam_word_cases import arpa_lm, small_lexicon, without_unigrams
from beam_word_conf_ref import beam_word_conf_ref
from beam_word_la_stream_ref import BeamWordLaStreamRef
from beam_word_loss_ref import word_model
from beam_word_stream_conf_ref import BeamWordStreamConfRef
from beam_word_stream_ref import NAMES, BeamWordStreamRef
from test_beam_word_conf_cpu import double_completion_case
from test_beam_word_la_cpu import rescue_case
from test_beam_word_loss_cpu import _emissions, _lse, _pair_seq
from test_beam_word_stream_cpu import _prefix_score

INF = float("inf")
ALL = 10_000
KW = dict(lm_weight=0.7, word_score=-0.4, token_score=0.3)
W = (0.7, -0.4, 0.3)
WIDE = ("path", "tokens", "states", "lm_states", "words", "word_frames")
LETTERS = [0.5, -1.0, 0.0, 2.0, -0.25]


def _stream(tr, lex, lm, B, M, K, th=INF, dt=np.float64, order=None, w=W):
    return BeamWordStreamConfRef(tr, lex, lm, B, M, K, th, *w, dtype=dt, order=order)


def _cuts(kind, T, rng):
    if kind == "ones":
        return [1] * T
    if kind == "one":
        return [T]
    cuts, left = [], T
    while left:
        n = int(rng.integers(0, min(left, 4) + 1))                        # empty chunks too
        cuts.append(n)
        left -= n
    return cuts + [0]


def _feed(s, x, lens, cuts, calls, tol=0):
    """The utterances x [T,B,N] with lengths `lens` through stream s in chunks of `cuts` frames; result_confidence after the chunks
    whose index is in `calls` (final and prefix alternate, so that neither mode's call changes what the other finds)."""
    a = 0
    for i, n in enumerate(cuts):
        s.advance(x[a:a + n], np.clip(lens - a, 0, n))
        a += n
        if i in calls:
            s.result_confidence(tol, final=bool(i % 2))


def _same(got, want, T, what):
    """A stream result (width M >= T) against beam_word_conf_ref's (width T): byte for byte on the columns, padding beyond."""
    for n in ("scores", "normalisers", "token_lengths", "word_lengths"):
        assert got[n].dtype == want[n].dtype and got[n].tobytes() == want[n].tobytes(), (what, n)
    for n in WIDE:
        assert np.array_equal(got[n][:, :T], want[n]) and (got[n][:, T:] == -1).all(), (what, n)
    assert got["word_confidences"][:, :T].tobytes() == want["word_confidences"].tobytes(), what
    assert (got["word_confidences"][:, T:] == 0).all(), what


def _slot(r, b):
    return {n: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for n, v in r.items()}


# ---------------------------------------------------------------------------------------------------------------- final = True
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_final_equals_the_one_shot_confidences_for_every_cut_and_every_placement_of_calls(order, dt):
    lex = small_lexicon(LETTERS)
    lm = arpa_lm(5, order, 60 + order, keep=(1.0, 0.5, 0.5))
    T, B, M = 7, 3, 9
    x, tr = _emissions(T, B, 5, 11 + order, dt)
    lens = np.array([T, 0, 4])
    rng = np.random.default_rng(11)
    checked = unsure = 0
    for K in (1, 3, 8, ALL):
        for th in (INF, 2.0):
            want = {tol: beam_word_conf_ref(x, tr, lex, lm, lens, K, th, *W, tol) for tol in (0, 1, 5)}
            c = want[0]["word_confidences"]
            unsure += int(((c > 0) & (c < 0.999)).sum())
            for kind, calls in (("ones", "every"), ("one", "none"), ("random", "some"), ("random", "every")):
                cuts = _cuts(kind, T, rng)
                at = {"none": set(), "every": set(range(len(cuts))), "some": set(range(1, len(cuts), 2))}[calls]
                s = _stream(tr, lex, lm, B, M, K, th, dt)
                _feed(s, x, lens, cuts, at)
                for tol in (0, 1, 5):
                    got = s.result_confidence(tol, final=True)
                    _same(got, want[tol], T, (order, K, th, kind, calls, tol))
                    assert np.array_equal(got["frames"], lens) and (got["status"] == 0).all()
                    assert got["sets"] == want[tol]["sets"]
                    checked += 1
    assert checked == 4 * 2 * 4 * 3 and unsure > 5


@pytest.mark.parametrize("order", [1, 2])
def test_look_ahead_streams_equal_the_one_shot_with_the_same_look_ahead(order):
    lex, lm, x, tr = rescue_case(np.float64)
    plain = beam_word_conf_ref(x, tr, lex, lm, None, 1)
    want = beam_word_conf_ref(x, tr, lex, lm, None, 1, order=order)
    assert plain["words"][0, 0] == 0 and want["words"][0, 0] == 1 and want["sets"] != plain["sets"]      # the rescued word
    for cuts, calls in (([1, 1, 1], {0, 1, 2}), ([3], set()), ([2, 0, 1], {1})):
        s = _stream(tr, lex, lm, 1, 4, 1, order=order, w=(1.0, 0.0, 0.0))
        _feed(s, x, np.array([3]), cuts, calls)
        got = s.result_confidence(0, final=True)
        _same(got, want, 3, (order, cuts))
        assert abs(got["word_confidences"][0, 0] - 1.0) < 1e-12 and got["sets"] == want["sets"]
    # a grid where the look-ahead search keeps other pairs than the plain one, pruned
    lex = small_lexicon(LETTERS)
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    x, tr = _emissions(7, 3, 5, 14)
    lens = np.array([7, 5, 1])
    differ = 0
    rng = np.random.default_rng(5)
    for K, th in ((2, INF), (3, INF), (8, 2.0)):
        want = beam_word_conf_ref(x, tr, lex, lm, lens, K, th, *W, 1, order=order)
        differ += want["sets"] != beam_word_conf_ref(x, tr, lex, lm, lens, K, th, *W, 1)["sets"]
        for kind in ("ones", "one", "random"):
            cuts = _cuts(kind, 7, rng)
            s = _stream(tr, lex, lm, 3, 8, K, th, order=order)
            _feed(s, x, lens, cuts, set(range(0, len(cuts), 2)), tol=1)
            _same(s.result_confidence(1, final=True), want, 7, (order, K, th, kind))
            la = BeamWordLaStreamRef(tr, lex, lm, order, 3, 8, K, th, *W, dtype=np.float64)
            _feed_plain(la, x, lens, cuts)
            for final in (False, True):                                    # the search is the look-ahead stream's
                r, p = s.result_confidence(0, final=final), la.result(final)
                assert all(np.array_equal(r[n], p[n]) for n in NAMES)
    assert differ >= 2


def _feed_plain(s, x, lens, cuts):
    a = 0
    for n in cuts:
        s.advance(x[a:a + n], np.clip(lens - a, 0, n))
        a += n


# ---------------------------------------------------------------------------------------------------------------- prefix mode
@pytest.mark.parametrize("order", [2, 3])
def test_prefix_events_are_the_sum_over_exactly_the_label_paths_inside_the_kept_sets(order):
    lex = small_lexicon(LETTERS)
    lm = without_unigrams(arpa_lm(5, order, 3 + order), {2})
    T, N = 5, 5
    x, tr = _emissions(T, 1, N, 31 + order)
    m = word_model(lex, lm, np.float64, **KW)
    sep = m.sep
    pruned = midword = 0
    for K in (ALL, 1, 2, 3, 8):
        s = _stream(tr, lex, lm, 1, T, K)
        for L in range(1, T + 1):                                         # cut after every frame
            s.advance(x[L - 1:L])
            res = {tol: s.result_confidence(tol, final=False) for tol in (0, 1, 5)}
            sets = [set(tuple(p) for p in u) for u in res[0]["sets"][0]]
            assert len(sets) == L
            inside, total = [], 0
            for labels in itertools.product(range(N), repeat=L):          # all 5^L label paths (3125 at L = 5)
                v = _prefix_score(x[:L, 0], tr, lex, lm, labels, *W)
                if not v > -np.inf:
                    continue
                seq = _pair_seq(m, labels)
                total += 1
                if all(p in sets[t] for t, p in enumerate(seq)):
                    ev = [(int(m.wos[m.state[seq[t - 1][1]]]), t) for t in range(1, L) if labels[t] == sep and labels[t - 1] != sep]
                    inside.append((float(v), labels, ev))
            pruned += len(inside) < total
            assert inside                                                  # (the kept sets hold at least the best prefix)
            Z = _lse([v for v, _, _ in inside])
            assert np.allclose(res[0]["normalisers"][0], Z, rtol=1e-9, atol=1e-9), (K, L)
            direct = {}
            for v, _, ev in inside:                                        # P(w, t) directly, no end term
                for key in ev:
                    direct[key] = direct.get(key, 0.0) + np.exp(v - Z)
            got = res[0]["events"][0]
            assert set(got) == set(direct) and all(1 <= t <= L - 1 for _, t in got)
            for key, v in direct.items():
                assert abs(got[key] - v) < 1e-9, (K, L, key)
            best = max(inside, key=lambda it: it[0])
            nw = int(res[0]["word_lengths"][0])
            assert nw == len(best[2]) and [w for w, _ in best[2]] == list(res[0]["words"][0, :nw])
            assert np.allclose(res[0]["scores"][0], best[0], rtol=1e-9, atol=1e-9)
            midword += int(m.state[_pair_seq(m, best[1])[-1][1]] != 0 and best[1][-1] != sep)
            plain = s.result(False)
            for tol in (0, 1, 5):
                r = res[tol]
                assert all(np.array_equal(r[n], plain[n]) for n in NAMES)  # the hypothesis is result(final=False)'s
                assert [t for _, t in best[2]] == list(r["word_frames"][0, :nw]) and (r["word_frames"][0, nw:] == -1).all()
                assert (r["word_confidences"][0, nw:] == 0).all()
                for k, (w, tk) in enumerate(best[2]):
                    want = sum(v for (w2, t), v in direct.items() if w2 == w and abs(t - tk) <= tol)
                    assert abs(r["word_confidences"][0, k] - want) < 1e-9, (K, L, tol, k)
    assert pruned >= 3 and midword >= 3                                    # prefixes that end inside a word: no event for it


@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("order", [2, 3])
def test_the_bounds_at_tolerance_0_and_the_single_path_of_a_beam_of_1(order, final):
    lex = small_lexicon(LETTERS)
    lm = arpa_lm(5, order, 60 + order, keep=(1.0, 0.5, 0.5))
    T, B = 9, 4
    x, tr = _emissions(T, B, 5, 5)
    seen = below = 0
    for K in (1, 4, 16):
        s = _stream(tr, lex, lm, B, T, K)
        for a in range(0, T, 3):
            s.advance(x[a:a + 3])
            r = s.result_confidence(0, final=final)
            for b in range(B):
                nw, Z = int(r["word_lengths"][b]), r["normalisers"][b]
                if not np.isfinite(r["scores"][b]):
                    assert nw == 0
                    continue
                seen += 1
                assert np.isfinite(Z) and r["scores"][b] <= Z + 1e-9
                c = r["word_confidences"][b, :nw]
                assert (c >= np.exp(r["scores"][b] - Z) - 1e-9).all() and (c <= 1 + 1e-9).all()
                below += int((c < 0.999).sum())
                f = r["word_frames"][b, :nw]
                assert (np.diff(f) > 0).all() and (f >= 1).all() and (f <= (a + 3 if final else a + 2)).all()
                if K == 1:                                                 # one path: it is sure of itself, and Z is its score
                    assert np.allclose(c, 1.0, rtol=1e-9) and np.allclose(Z, r["scores"][b], rtol=1e-9, atol=1e-9)
    assert seen > 10 and below > 5


# ---------------------------------------------------------------------------------------------------------------- edge cases
def test_no_frame_one_frame_and_an_emptied_beam():
    lex, lm = small_lexicon(LETTERS), arpa_lm(5, 2, 9)
    x, tr = _emissions(6, 3, 5, 9)
    s = _stream(tr, lex, lm, 3, 6, 3)
    for final in (False, True):                                            # L = 0
        r = s.result_confidence(2, final=final)
        assert (r["scores"] == -INF).all() and (r["normalisers"] == -INF).all()
        assert (r["token_lengths"] == 0).all() and (r["word_lengths"] == 0).all()
        assert all((r[n] == -1).all() for n in WIDE) and (r["word_confidences"] == 0).all() and (r["frames"] == 0).all()
    s.advance(x[:1], np.array([1, 0, 1]))                                  # L = 1 in slots 0 and 2
    r = s.result_confidence(0, final=False)
    assert list(r["word_lengths"]) == [0, 0, 0] and list(r["token_lengths"]) == [1, 0, 1]       # one frame: no separator edge yet
    assert np.isfinite(r["normalisers"][[0, 2]]).all() and r["normalisers"][1] == -INF and r["events"][0] == {}
    r = s.result_confidence(0, final=True)                                 # ... and with the end rule a one-letter word at frame 1
    assert list(r["word_lengths"]) == [1, 0, 1] and r["word_frames"][0, 0] == 1 and 0 < r["word_confidences"][0, 0] <= 1
    x[3:, 0] = -INF                                                        # slot 0: every candidate of frame 3 is -inf
    s.advance(x[1:])
    for final in (False, True):
        r = s.result_confidence(1, final=final)
        assert s.sizes()[0][2] > 0 and s.sizes()[0][3:] == [0, 0, 0]
        assert r["scores"][0] == -INF and r["normalisers"][0] == -INF and r["word_lengths"][0] == 0
        assert (r["word_frames"][0] == -1).all() and (r["word_confidences"][0] == 0).all() and (r["path"][0] == -1).all()
        assert np.isfinite(r["normalisers"][1:]).all() and not np.isnan(r["word_confidences"]).any()


def test_a_prefix_that_ends_mid_word_and_a_final_word_by_the_end_rule_on_the_same_state():
    lex, lm, x, tr = rescue_case(np.float64)                               # 0, 1 | 2, separator
    s = _stream(tr, lex, lm, 1, 3, ALL, w=(1.0, 0.0, 0.0))
    s.advance(x[:2])                                                       # two frames: inside the first word
    pre = s.result_confidence(0, final=False)
    assert pre["word_lengths"][0] == 0 and (pre["word_frames"] == -1).all() and (pre["word_confidences"] == 0).all()
    assert pre["events"][0] == {} and np.isfinite(pre["normalisers"][0]) and pre["path"][0, 1] != lex.separator
    assert pre["token_lengths"][0] == 2
    fin = s.result_confidence(0, final=True)                               # the same state: the end rule closes the word at t = L
    assert fin["word_lengths"][0] == 1 and fin["word_frames"][0, 0] == 2 and set(t for _, t in fin["events"][0]) == {2}
    assert 0.5 < fin["word_confidences"][0, 0] < 1.0
    _same(fin, beam_word_conf_ref(x[:2], tr, lex, lm, None, ALL), 2, "opened")
    s.advance(x[2:])                                                       # the separator: the word is a separator word now
    pre = s.result_confidence(0, final=False)
    assert pre["word_lengths"][0] == 1 and pre["word_frames"][0, 0] == 2 and set(t for _, t in pre["events"][0]) == {2}
    assert 0.5 < pre["word_confidences"][0, 0] < 1.0
    _same(s.result_confidence(0, final=True), beam_word_conf_ref(x, tr, lex, lm, None, ALL), 3, "closed")


def test_a_short_word_completed_twice_inside_the_window_counts_twice():
    lex, lm, x, tr = double_completion_case()
    for final in (False, True):
        s = _stream(tr, lex, lm, 1, 4, ALL, w=(1.0, 0.0, 0.0))
        s.advance(x[:3])
        s.result_confidence(2, final=final)
        s.advance(x[3:])
        r0, r1, r2 = (s.result_confidence(tol, final=final) for tol in (0, 1, 2))
        assert list(r0["path"][0]) == [0, 1, 0, 1] and list(r0["words"][0, :2]) == [0, 0]
        assert list(r0["word_frames"][0, :2]) == [1, 3]
        assert (r1["word_confidences"][0, :2] <= 1 + 1e-12).all()          # |1 - 3| = 2: the windows do not meet
        c = r2["word_confidences"][0, :2]
        assert (c > 1.2).all() and (c <= 2 + 1e-12).all()                  # an expected count, unclipped
        if final:
            for tol, r in ((0, r0), (1, r1), (2, r2)):
                _same(r, beam_word_conf_ref(x, tr, lex, lm, None, ALL, INF, frame_tolerance=tol), 4, tol)


def test_a_masked_reset_in_mid_stream_takes_apos_back_in_the_chosen_slots_only():
    lex, lm = small_lexicon(LETTERS), arpa_lm(5, 3, 7)
    x, tr = _emissions(8, 3, 5, 13, np.float32)
    s = _stream(tr, lex, lm, 3, 8, 4, dt=np.float32)
    s.advance(x[:3])
    s.result_confidence(0)
    assert [sl.apos for sl in s.slots] == [3, 3, 3]
    s.advance(x[3:5])
    s.reset(np.array([0, 1, 0]))
    assert [sl.apos for sl in s.slots] == [3, 0, 3] and [sl.pos for sl in s.slots] == [5, 0, 5]
    s.advance(x[5:8])
    got = s.result_confidence(1, final=True)
    assert [sl.apos for sl in s.slots] == [8, 3, 8]
    whole = beam_word_conf_ref(x, tr, lex, lm, None, 4, INF, *W, 1)
    tail = beam_word_conf_ref(x[5:8], tr, lex, lm, None, 4, INF, *W, 1)
    for b, (ref, T) in enumerate([(whole, 8), (tail, 3), (whole, 8)]):
        _same(_slot(got, b), _slot(ref, b), T, b)


def test_the_clamp_at_max_frames_and_the_status_word():
    lex, lm = small_lexicon(LETTERS), arpa_lm(5, 2, 9)
    x, tr = _emissions(9, 2, 5, 15)
    s = _stream(tr, lex, lm, 2, 6, 4)
    s.advance(x[:4], np.array([4, 2]))
    s.advance(x[4:9], np.array([5, 4]))                                    # slot 0: 4 + 5 > 6 frames, slot 1: 2 + 4 = 6 exactly
    r = s.result_confidence(2, final=True)
    assert list(r["frames"]) == [6, 6] and list(r["status"]) == [1, 0]
    x1 = np.concatenate([x[:2, 1], x[4:8, 1]])[:, None]
    for b, xb in ((0, x[:6, 0:1]), (1, x1)):
        want = beam_word_conf_ref(xb, tr, lex, lm, None, 4, INF, *W, 2)
        _same(_slot(r, b), want, 6, b)


def test_result_confidence_leaves_the_search_alone():
    lex, lm = small_lexicon(LETTERS), arpa_lm(5, 3, 7)
    x, tr = _emissions(7, 2, 5, 17, np.float32)
    a = _stream(tr, lex, lm, 2, 7, 5, 3.0, np.float32)
    b = BeamWordStreamRef(tr, lex, lm, 2, 7, 5, 3.0, *W, dtype=np.float32)
    for lo in range(0, 7, 2):
        a.advance(x[lo:lo + 2])
        b.advance(x[lo:lo + 2])
        for final in (False, True):
            a.result_confidence(1, final=final)
        for sa, sb in zip(a.slots, b.slots):                               # pos, the set, the back-pointers
            assert sa.pos == sb.pos and sa.A == sb.A and sa.back == sb.back and sa.kept == sb.kept
        for final in (False, True):
            u, v = a.result(final), b.result(final)
            assert all(np.array_equal(u[n], v[n]) for n in NAMES)
