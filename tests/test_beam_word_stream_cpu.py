"""CPU tests of streaming beam decoding with a lexicon and a word LM: the test-side restatement with explicit carried state
(tests/beam_word_stream_ref.py) against the one-shot restatement (tests/beam_word_ref.py) byte for byte, per-frame set sizes
included, for every way of cutting an utterance into chunks; the best prefix hypothesis against an enumeration of all label
paths scored without any end term; result() leaving the state alone, masked reset, the clamp at max_frames and `status`, a
threshold changed between chunks -- no kernel is launched here."""
import copy
import itertools

import numpy as np
import pytest

from beam_word_cases import arpa_lm, eighths, integers, small_lexicon
from beam_word_ref import beam_word_ref, fold_lm
from beam_word_stream_ref import NAMES, BeamWordStreamRef
from graph_decode_ref import fold

LW, WS, TS = 0.7, -0.4, 0.3
ONE = NAMES[:8]
ALL = 1024                                                 # more than every pair of the small cases
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


def _case(T, B, N, seed, dtype, integer=False):
    rng = np.random.default_rng(seed)
    if integer:
        x = rng.integers(-2, 3, size=(T, B, N)).astype(dtype)
        tr = np.zeros((N, N), dtype)
    else:
        x = rng.normal(size=(T, B, N)).astype(dtype)
        tr = rng.normal(size=(N, N)).astype(dtype)
    il = rng.integers(0, T + 1, size=B)
    il[0] = T
    if B > 1:
        il[1] = 0
    if B > 2:
        il[2] = 1
    return x, tr, il


def _feed(s, x, il, cuts, **kw):
    """Advance by the chunks x[t0:t1] for consecutive cuts; slot b takes the frames below il[b]."""
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        s.advance(x[t0:t1], np.clip(il - t0, 0, t1 - t0), **kw)


def _same_as_one_shot(res, one, T, what):
    """res: a stream result over max_frames >= T columns; one: the one-shot decode over T columns.  Bytes, not values."""
    for n in ("scores", "token_lengths", "word_lengths"):
        assert res[n].dtype == one[n].dtype and res[n].tobytes() == one[n].tobytes(), (n, what)
    for n in ("path", "tokens", "states", "lm_states", "words"):
        assert res[n].dtype == np.int64 and np.array_equal(res[n][:, :T], one[n]) and (res[n][:, T:] == -1).all(), (n, what)


def _chunkings(T, rng):
    yield "ones", list(range(T + 1))
    yield "whole", [0, T]
    for i in range(2):
        inner = np.sort(rng.integers(0, T + 1, size=int(rng.integers(2, 6))))
        cuts = [0] + inner.tolist() + [T]
        if i == 0:
            cuts = [0, 0] + cuts[1:] + [T]                   # chunks of no frames at both ends
        yield "random%d" % i, cuts


@DTYPES
@pytest.mark.parametrize("weights", ["eighths", "integers"])
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_any_chunking_equals_the_one_shot_restatement(order, weights, dtype):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = (eighths if weights == "eighths" else integers)(arpa_lm(5, order, 60 + order, keep=(1.0, 0.5, 0.5)))
    T, B, M = 7, 4, 9
    x, tr, il = _case(T, B, 5, 11 + order, dtype, integer=weights == "integers")
    rng = np.random.default_rng(7)
    shared = 0
    for K in (1, 3, 8, ALL):
        for theta in (np.inf, 2.0, 0.0):
            info = {}
            one = beam_word_ref(x, tr, lex, lm, il, K, theta, LW, WS, TS, info=info)
            shared += sum(len({q for _, q in kept}) < len(kept) for kl in info["kept"] for kept in kl)
            for name, cuts in _chunkings(T, rng):
                s = BeamWordStreamRef(tr, lex, lm, B, M, K, theta, LW, WS, TS, dtype)
                _feed(s, x, il, cuts)
                what = (name, cuts, K, theta)
                _same_as_one_shot(s.result(final=True), one, T, what)
                assert s.sizes() == info["sizes"] and s.cands() == info["cands"] and s.kept() == info["kept"], what
                assert (s.tie_cuts, s.src_ties) == (info["tie_cuts"], info["src_ties"]), what
                r = s.result(final=True)
                assert r["frames"].tolist() == il.tolist() and (r["status"] == 0).all(), what
    assert shared > 0                                      # some frame kept two pairs with one q and different h


def _prefix_score(xb, tr, lexicon, lm, labels, lm_weight, word_score, token_score):
    """The value of one label sequence as a PREFIX -- the specification's adds, no final weight, no LM end -- or -inf if the
    lexicon or the LM rejects it; written apart from the search."""
    dt = xb.dtype.type
    g = lexicon.graph
    sep, wos = lexicon.separator, lexicon.word_of_state
    present, arcw, _ = fold(g.next, g.weight, g.final, dt, 1.0, token_score)
    lw, bw, _ = fold_lm(lm, dt, lm_weight, word_score)
    ninf = dt(-np.inf)
    l0 = int(labels[0])
    if not present[0, l0]:
        return ninf
    s, h = int(g.next[0, l0]), lm.start
    v = dt(arcw[0, l0] + xb[0, l0])
    for t in range(1, len(labels)):
        i, j = int(labels[t]), int(labels[t - 1])
        if i == j:
            v = dt(dt(v + tr[i, i]) + xb[t, i])
            continue
        if not present[s, i]:
            return ninf
        c = dt(dt(v + tr[i, j]) + arcw[s, i])
        if i == sep:
            a, w = dt(0), int(wos[s])
            while lm.find(h, w) < 0:
                if lm.backoff[h] < 0:
                    return ninf
                a, h = dt(a + bw[h]), int(lm.backoff[h])
            k = lm.find(h, w)
            h, c = int(lm.next[k]), dt(c + dt(a + lw[k]))
        s = int(g.next[s, i])
        v = dt(c + xb[t, i])
    return v


@DTYPES
def test_the_prefix_result_is_the_best_of_all_label_paths_without_an_end_term(dtype):
    from torch_asg_amd import Lexicon
    lex = Lexicon([[0], [0, 1], [1, 2, 0], [2]], 4, 3, [0.25, -0.5, 1.0, 0.0])
    lm = eighths(arpa_lm(4, 2, 81, keep=(1.0, 0.6)))
    rng = np.random.default_rng(3)
    T, B = 5, 2
    x = rng.normal(size=(T, B, 4)).astype(dtype)
    tr = rng.normal(size=(4, 4)).astype(dtype)
    s = BeamWordStreamRef(tr, lex, lm, B, T, ALL, np.inf, LW, WS, TS, dtype)
    midword = 0
    for t in range(T):
        s.advance(x[t:t + 1])
        r = s.result(final=False)
        for b in range(B):
            best, arg = dtype(-np.inf), None
            with np.errstate(invalid="ignore"):
                for labels in itertools.product(range(4), repeat=t + 1):
                    v = _prefix_score(x[:, b], tr, lex, lm, labels, LW, WS, TS)
                    if v > best:
                        best, arg = v, labels
            assert r["scores"][b].tobytes() == best.tobytes(), (t, b)
            assert _prefix_score(x[:, b], tr, lex, lm, r["path"][b, :t + 1], LW, WS, TS).tobytes() == best.tobytes()
            # the words are those of the separator edges alone: no final word, whatever node the prefix ends in
            p = r["path"][b, :t + 1]
            nsep = int(((p[1:] == 3) & (p[:-1] != 3)).sum())
            assert r["word_lengths"][b] == nsep and (r["words"][b, nsep:] == -1).all()
            st = r["states"][b, t]
            midword += int(st != 0 and lex.word_of_state[st] < 0)
    assert midword > 0                                     # a prefix that ends mid-word is a valid prefix


def test_result_leaves_the_state_alone_and_masked_reset_restarts_a_slot():
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    T, B = 8, 3
    x, tr, _ = _case(T, B, 5, 21, np.float32)
    il = np.array([T, T, T])
    a = BeamWordStreamRef(tr, lex, lm, B, T, 4, 3.0, LW, WS, TS)
    b = BeamWordStreamRef(tr, lex, lm, B, T, 4, 3.0, LW, WS, TS)
    for t in range(T):
        a.advance(x[t:t + 1])
        b.advance(x[t:t + 1])
        before = copy.deepcopy(a.slots)
        a.result(final=False), a.result(final=True)
        for u, v in zip(before, a.slots):
            assert (u.pos, u.overflow, u.A, u.back) == (v.pos, v.overflow, v.A, v.back)
    ra, rb = a.result(True), b.result(True)
    for n in NAMES:
        assert ra[n].tobytes() == rb[n].tobytes()
    # slot 1 starts again after 3 frames and sees x[3:] as a new utterance; slots 0 and 2 go on
    s = BeamWordStreamRef(tr, lex, lm, B, T, 4, 3.0, LW, WS, TS)
    s.advance(x[:3])
    s.reset(np.array([0, 1, 0]))
    assert [sl.pos for sl in s.slots] == [3, 0, 3]
    s.advance(x[3:])
    got = s.result(True)
    whole = beam_word_ref(x, tr, lex, lm, il, 4, 3.0, LW, WS, TS)
    tail = beam_word_ref(x[3:], tr, lex, lm, il - 3, 4, 3.0, LW, WS, TS)
    assert got["frames"].tolist() == [T, T - 3, T]
    for n in ONE:
        assert np.array_equal(got[n][0], whole[n][0]) and np.array_equal(got[n][2], whole[n][2]), n
        if got[n].ndim == 2:
            assert np.array_equal(got[n][1, :T - 3], tail[n][1]) and (got[n][1, T - 3:] == -1).all(), n
        else:
            assert got[n][1] == tail[n][1], n
    s.reset()
    r = s.result(True)
    assert (r["scores"] == -np.inf).all() and (r["frames"] == 0).all() and (r["path"] == -1).all()


def test_the_clamp_at_max_frames_sets_status_and_keeps_the_first_frames():
    lex = small_lexicon()
    lm = arpa_lm(5, 2, 64)
    T, B, M = 9, 3, 6
    x, tr, _ = _case(T, B, 5, 22, np.float64)
    s = BeamWordStreamRef(tr, lex, lm, B, M, 5, np.inf, LW, WS, TS, np.float64)
    s.advance(x[:4], np.array([4, 2, 0]))
    assert s.result()["status"].tolist() == [0, 0, 0]
    s.advance(x[4:], np.array([5, 4, 5]))                  # slot 0: 4 + 5 > 6; slot 1: 2 + 4 == 6; slot 2: 5 <= 6
    r = s.result(True)
    assert r["frames"].tolist() == [6, 6, 5] and r["status"].tolist() == [1, 0, 0]
    x0 = np.concatenate([x[:4, 0], x[4:6, 0]])
    x1 = np.concatenate([x[:2, 1], x[4:8, 1]])
    x2 = np.concatenate([x[4:9, 2], x[:1, 2]])
    one = beam_word_ref(np.stack([x0, x1, x2], 1), tr, lex, lm, np.array([6, 6, 5]), 5, np.inf, LW, WS, TS)
    _same_as_one_shot(r, one, M, "clamp")
    s.advance(x[:1])                                       # everything is full or fills up; status is sticky
    r = s.result(True)
    assert r["frames"].tolist() == [6, 6, 6] and r["status"].tolist() == [1, 1, 0]
    s.reset(np.array([1, 0, 0]))
    assert s.result()["status"].tolist() == [0, 1, 0]


def test_a_threshold_changed_between_chunks_applies_to_the_frames_of_its_call():
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 2, 65)
    T, B = 8, 2
    x, tr, _ = _case(T, B, 5, 23, np.float32)
    il = np.array([T, T])
    thetas = [np.inf] * 3 + [0.75] * 5                     # per frame
    outs = []
    for cuts in ([0, 3, 8], [0, 1, 3, 4, 8], list(range(T + 1))):
        s = BeamWordStreamRef(tr, lex, lm, B, T, 6, np.inf, LW, WS, TS)
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            assert len(set(thetas[t0:t1])) == 1
            s.advance(x[t0:t1], beam_threshold=thetas[t0])
        outs.append((s.result(True), s.sizes()))
    for r, sz in outs[1:]:
        assert sz == outs[0][1]
        for n in NAMES:
            assert r[n].tobytes() == outs[0][0][n].tobytes(), n
    wide = beam_word_ref(x, tr, lex, lm, il, 6, np.inf, LW, WS, TS, info=(iw := {}))
    tight = beam_word_ref(x, tr, lex, lm, il, 6, 0.75, LW, WS, TS, info=(it := {}))
    assert wide is not None and tight is not None
    sz = outs[0][1]
    assert [z[:3] for z in sz] == [z[:3] for z in iw["sizes"]]             # the first frames ran with no threshold
    assert sz != iw["sizes"] and sz != it["sizes"]                          # and the change of threshold is seen
