"""CPU tests of streaming beam decoding: the test-side restatement with explicit carried state (tests/beam_stream_ref.py)
against the one-shot restatement (tests/beam_decode_ref.py) for every way of cutting an utterance into chunks, the best prefix
hypothesis against exhaustive enumeration, result() leaving the state alone, masked reset, the clamp at max_frames -- no kernel
is launched here."""
import copy
import itertools

import numpy as np
import pytest

from beam_decode_ref import beam_decode_ref
from beam_stream_ref import BeamStreamRef
from graph_decode_ref import path_score_graph

LW, TS = 0.8, -0.5


def _tg():
    from torch_asg_amd import TokenGraph
    return TokenGraph


def _ngram(N, order, seed, holes=False):
    rng = np.random.default_rng(seed)
    lp = np.log(rng.dirichlet(np.ones(N + 1), size=(N + 1,) * (order - 1))) if order > 1 else np.log(rng.dirichlet(np.ones(N + 1)))
    if holes:
        lp[rng.random(size=lp.shape) < 0.2] = -np.inf
    return _tg().from_ngram(lp)


def _random_graph(S, N, seed):
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, S // 2, size=(S, N))
    nxt[rng.random(size=(S, N)) < 0.3] = -1
    w = rng.normal(size=(S, N))
    f = rng.normal(size=S)
    f[rng.random(size=S) < 0.3] = -np.inf
    return _tg()(nxt, w, f, start=0)


def _lexicon(seed):
    rng = np.random.default_rng(seed)
    N, sep = 8, 7
    words = []
    while len(words) < 30:
        w = rng.integers(0, sep, size=int(rng.integers(1, 5))).tolist()
        if all(a != b for a, b in zip(w, w[1:])):
            words.append(w)
    return _tg().from_lexicon(words, N, sep, rng.normal(size=len(words)))


GRAPHS = {
    "random": lambda: _random_graph(30, 12, 4),
    "bigram8": lambda: _ngram(8, 2, 2, holes=True),
    "trigram6": lambda: _ngram(6, 3, 3, holes=True),
    "lexicon": lambda: _lexicon(5),
}


def _case(T, B, N, seed, dtype, integer=False):
    rng = np.random.default_rng(seed)
    if integer:
        x = rng.integers(-2, 3, size=(T, B, N)).astype(dtype)
        tr = rng.integers(-1, 2, size=(N, N)).astype(dtype)
    else:
        x = rng.normal(size=(T, B, N))
        x = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(dtype)
        tr = rng.normal(size=(N, N)).astype(dtype)
    il = rng.integers(0, T + 1, size=B)
    il[0] = T
    if B > 1:
        il[1] = 0
    if B > 2:
        il[2] = 1
    return x, tr, il


def _stream(g, tr, B, max_frames, K, theta, dtype):
    return BeamStreamRef(tr, g.next, g.weight, g.final, g.start, B, max_frames, K, theta, LW, TS, dtype)


def _feed(s, x, il, cuts):
    """Advance by the chunks x[t0:t1] for consecutive cuts; slot b takes the frames below il[b]."""
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        s.advance(x[t0:t1], np.clip(il - t0, 0, t1 - t0))


def _same_as_one_shot(res, one, T, what):
    """res: a stream result over max_frames >= T columns; one: the one-shot decode over T columns.  Bytes, not values."""
    sc, path, tok, tl, st = res[:5]
    assert sc.dtype == one[0].dtype and sc.tobytes() == one[0].tobytes(), what
    assert tl.tobytes() == one[3].tobytes(), what
    for got, want in ((path, one[1]), (tok, one[2]), (st, one[4])):
        assert got.dtype == np.int64 and np.array_equal(got[:, :T], want) and (got[:, T:] == -1).all(), what


def _chunkings(T, rng):
    yield "ones", list(range(T + 1))
    yield "whole", [0, T]
    for i in range(3):
        inner = np.sort(rng.integers(0, T + 1, size=int(rng.integers(2, 8))))
        cuts = [0] + inner.tolist() + [T]
        if i == 0:
            cuts = [0, 0] + cuts[1:] + [T]                   # chunks of no frames at both ends
        yield "random%d" % i, cuts


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_any_chunking_equals_the_one_shot_decode(name, dtype):
    g = GRAPHS[name]()
    Q = g.compile_host(np.float32)["Q"]
    T, B = 20, 5
    rng = np.random.default_rng(77)
    zero_chunks = False
    for integer in (False, True):
        x, tr, il = _case(T, B, g.N, 41 + integer, dtype, integer)
        for K in (1, 3, 8, Q):
            for theta in (np.inf, 2.0, 0.0):
                sizes = []
                one = beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, il, K, theta, LW, TS, sizes=sizes)
                for cname, cuts in _chunkings(T, rng):
                    zero_chunks |= any(a == b for a, b in zip(cuts[:-1], cuts[1:]))
                    s = _stream(g, tr, B, T + 3, K, theta, dtype)
                    _feed(s, x, il, cuts)
                    res = s.result(final=True)
                    what = "%s K=%d theta=%s %s" % (name, K, theta, cname)
                    _same_as_one_shot(res, one, T, what)
                    assert np.array_equal(res[5], il) and not res[6].any(), what
                    # the sets themselves, not only the winner (beam_decode_ref reports no sizes for an utterance of no frames)
                    assert [z for z in s.sizes() if z] == sizes, what
    assert zero_chunks


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_prefix_result_against_exhaustive_enumeration(seed, dtype):
    """With a full beam, result(final=False) after frame t is the best score over ALL label sequences of t+1 frames, the final
    weight left out; result(final=True) the best with it."""
    rng = np.random.default_rng(500 + seed)
    for _ in range(6):
        T, N, S = int(rng.integers(1, 6)), int(rng.integers(2, 5)), int(rng.integers(1, 5))
        nxt = rng.integers(0, S, size=(S, N))
        nxt[rng.random(size=(S, N)) < 0.25] = -1
        w = rng.normal(size=(S, N))
        f = rng.normal(size=S)
        f[rng.random(size=S) < 0.3] = -np.inf
        x = rng.normal(size=(T, 1, N)).astype(dtype)
        tr = rng.normal(size=(N, N)).astype(dtype)
        s = BeamStreamRef(tr, nxt, w, f, 0, 1, T, S * N, np.inf, 0.5, -0.3, dtype)
        for t in range(T):
            s.advance(x[t:t + 1])
            for final, fin in ((False, np.zeros(S)), (True, f)):
                sc, path = s.result(final)[:2]
                scored = [(path_score_graph(x[:t + 1, 0], tr, nxt, w, fin, p, 0, 0.5, -0.3)[0], p)
                          for p in itertools.product(range(N), repeat=t + 1)]
                best = max(v for v, _ in scored)
                assert sc[0] == best
                if best > -np.inf:
                    assert best == dict((p, v) for v, p in scored)[tuple(path[0, :t + 1])]      # the path has that score
                    assert (path[0, t + 1:] == -1).all()
                else:
                    assert (path[0] == -1).all()


def test_result_does_not_change_the_state():
    g = GRAPHS["trigram6"]()
    T, B = 16, 3
    x, tr, il = _case(T, B, g.N, 45, np.float32)
    il[:] = T
    one = beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, il, 4, 3.0, LW, TS)
    s = _stream(g, tr, B, T, 4, 3.0, np.float32)
    for t in range(T):
        s.advance(x[t:t + 1])
        before = copy.deepcopy(s.slots)
        a = s.result(final=False)
        b = s.result(final=True)
        c = s.result(final=False)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, c))
        for u, v in zip(before, s.slots):
            assert (u.pos, u.overflow, u.sizes) == (v.pos, v.overflow, v.sizes)
            assert np.array_equal(u.aq, v.aq) and np.array_equal(u.av, v.av) and len(u.history) == len(v.history)
        assert (a[5] == t + 1).all() and (b[5] == t + 1).all()
        # the prefix score is the largest value of the stored set
        assert all(a[0][i] == (v.av.max() if v.aq.size else -np.inf) for i, v in enumerate(s.slots))
    _same_as_one_shot(s.result(final=True), one, T, "after the partial results")


def test_masked_reset_restarts_only_the_chosen_slots():
    g = GRAPHS["bigram8"]()
    T, B = 14, 3
    x, tr, _ = _case(T, B, g.N, 46, np.float64)
    y, _, _ = _case(T, B, g.N, 47, np.float64)
    K, theta = 3, 4.0
    s = _stream(g, tr, B, T, K, theta, np.float64)
    s.advance(x[:6])
    s.reset(np.array([0, 1, 0]))
    assert [v.pos for v in s.slots] == [6, 0, 6]
    # slot 1 starts the utterance y[:, 1] while slots 0 and 2 go on with x
    mixed = x[6:].copy()
    mixed[:, 1] = y[:T - 6, 1]
    s.advance(mixed)
    res = s.result(final=True)
    assert res[5].tolist() == [T, T - 6, T]
    want_x = beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, None, K, theta, LW, TS)
    want_y = beam_decode_ref(y[:T - 6], tr, g.next, g.weight, g.final, g.start, None, K, theta, LW, TS)
    for b, (want, L) in enumerate(((want_x, T), (want_y, T - 6), (want_x, T))):
        assert res[0][b].tobytes() == want[0][b].tobytes() and res[3][b] == want[3][b]
        for i in (1, 2, 4):
            assert np.array_equal(res[i][b, :L], want[i][b]) and (res[i][b, L:] == -1).all()
    s.reset()
    assert all(v.pos == 0 and v.aq.size == 0 and not v.history for v in s.slots)
    assert not (s.result()[0] > -np.inf).any()


def test_frames_beyond_max_frames_are_dropped_and_reported():
    g = GRAPHS["random"]()
    T, B, M = 12, 2, 9
    x, tr, _ = _case(T, B, g.N, 48, np.float32)
    want = beam_decode_ref(x[:M], tr, g.next, g.weight, g.final, g.start, None, 4, np.inf, LW, TS)
    s = _stream(g, tr, B, M, 4, np.inf, np.float32)
    s.advance(x[:M], np.array([M, M - 1]))                    # slot 0 reaches max_frames exactly
    res = s.result(final=True)
    assert res[5].tolist() == [M, M - 1] and res[6].tolist() == [0, 0]
    s.advance(x[M - 1:M + 1], np.array([1, 2]))               # one frame too many for each
    res = s.result(final=True)
    assert res[5].tolist() == [M, M] and res[6].tolist() == [1, 1]
    assert res[0][0].tobytes() == want[0][0].tobytes() and np.array_equal(res[1][0], want[1][0])
    assert res[0][1].tobytes() == want[0][1].tobytes() and np.array_equal(res[1][1], want[1][1])
    s.advance(x[:0])                                          # a chunk of no frames cuts nothing
    s.reset(np.array([1, 0]))
    assert s.result()[6].tolist() == [0, 1]                   # the word is sticky until the slot is reset


def test_transition_and_threshold_may_change_between_chunks():
    g = GRAPHS["bigram8"]()
    T = 10
    x, tr, _ = _case(T, 1, g.N, 49, np.float32)
    tr2 = (tr * np.float32(0.5)).astype(np.float32)
    s = _stream(g, tr, 1, T, 3, np.inf, np.float32)
    s.advance(x[:4])
    s.advance(x[4:], transition=tr2, beam_threshold=1.0)
    # the same frames through two one-frame-at-a-time streams with the values switched at frame 4
    r = _stream(g, tr, 1, T, 3, np.inf, np.float32)
    for t in range(T):
        r.advance(x[t:t + 1], transition=tr if t < 4 else tr2, beam_threshold=np.inf if t < 4 else 1.0)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(s.result(True), r.result(True)))
    assert s.sizes() == r.sizes()
