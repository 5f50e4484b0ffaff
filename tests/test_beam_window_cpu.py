"""CPU tests of windowed streaming beam decoding: the restatement with explicit carried state and a ring of W rows
(tests/beam_window_ref.py) against the one-shot restatement (tests/beam_decode_ref.py) and the unbounded stream
(tests/beam_stream_ref.py) -- search identity, chunk invariance and exactness of the committed prefix (the three required
properties of include/asg_hip.h::asg_beam_window_advance), the convergence frame of every commit attempt against a brute-force
backtrace of every survivor, and the regimes by name: convergence with the ring wrapped, forced commits, a window that never
forces, a beam that empties after a commit -- no kernel is launched here."""
import numpy as np
import pytest

from beam_decode_ref import beam_decode_ref
from beam_stream_ref import BeamStreamRef
from beam_window_ref import BeamWindowRef, two_component_emissions, two_components_automaton

LW, TS = 0.8, -0.5
WP = [(1, 1), (2, 1), (2, 2), (5, 1), (5, 3), (5, 5), (16, 1), (16, 3), (16, 16)]       # W in {1, 2, 5, 16} x P in {1, 3, W}, P <= W


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


def two_components(N=6):
    return _tg()(*two_components_automaton(N), start=0)


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
    il = rng.integers(2, T + 1, size=B)
    il[0] = T
    if B > 1:
        il[1] = 1
    return x, tr, il


class _Checked(BeamWindowRef):
    """The restatement with the convergence frame of every attempt checked against brute force: every slot of the current set
    backtraced on its own down to `base`, c = the latest frame at which all those paths are in one state."""

    def _attempt(self, v, out):
        paths = np.stack([self._walk(v, int(q), v.pos - 1, v.base) for q in v.aq])        # [|A|][pos - base]
        same = np.nonzero((paths == paths[0]).all(0))[0]
        want = v.base + int(same[-1]) if same.size else None
        # (ancestries that have met stay together: the frames on which all agree are a prefix)
        assert same.size == 0 or same.tolist() == list(range(same[-1] + 1))
        super()._attempt(v, out)
        assert v.attempts[-1][2] == want, (v.attempts[-1], want)


def _window(g, tr, B, W, P, K, theta, dtype, cls=_Checked):
    return cls(tr, g.next, g.weight, g.final, g.start, B, W, P, K, theta, LW, TS, dtype)


def _run(s, x, il, cuts):
    """Advance by the chunks x[t0:t1]; slot b takes the frames below il[b].  -> per slot the concatenation of everything advance
    returned (path, states, tokens), and per call (cut, base, carry, status, committed so far) of every slot."""
    B = x.shape[1]
    cat = [([], [], []) for _ in range(B)]
    trace = []
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        n = np.clip(il - t0, 0, t1 - t0)
        np_, ns, nt, nf, nl = s.advance(x[t0:t1], n)
        assert np_.shape == (B, s.W + t1 - t0) and np_.dtype == np.int64
        for b in range(B):
            assert (np_[b, nf[b]:] == -1).all() and (ns[b, nf[b]:] == -1).all() and (nt[b, nl[b]:] == -1).all()
            cat[b][0].extend(np_[b, :nf[b]]); cat[b][1].extend(ns[b, :nf[b]]); cat[b][2].extend(nt[b, :nl[b]])
        trace.append((t1, [(v.pos, v.base, v.carry, v.status, len(cat[b][0]), len(cat[b][2])) for b, v in enumerate(s.slots)]))
    return cat, trace


def _chunkings(T, rng):
    yield "whole", [0, T]
    for i in range(2):
        inner = np.sort(rng.integers(0, T + 1, size=int(rng.integers(2, 8))))
        cuts = [0] + inner.tolist() + [T]
        if i == 0:
            cuts = [0, 0] + cuts[1:] + [T]                   # chunks of no frames at both ends
        yield "random%d" % i, cuts


def _check_exact(cat, res, one, il, what):
    """Property 3 for the slots without a forced commit and with a finite one-shot score."""
    sc, path, tok, tl, st, frames, committed, status = res
    n = 0
    for b in range(len(il)):
        L = int(il[b])
        assert frames[b] == L and committed[b] == len(cat[b][0]), what
        if status[b] & 1 or not one[0][b] > -np.inf:
            continue
        n += 1
        tail = L - committed[b]
        assert cat[b][0] + path[b, :tail].tolist() == one[1][b, :L].tolist() and (path[b, tail:] == -1).all(), what
        assert cat[b][1] + st[b, :tail].tolist() == one[4][b, :L].tolist() and (st[b, tail:] == -1).all(), what
        assert cat[b][2] + tok[b, :tl[b]].tolist() == one[2][b, :one[3][b]].tolist() and (tok[b, tl[b]:] == -1).all(), what
    return n


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_search_identity_chunk_invariance_and_exactness(name, dtype):
    g = GRAPHS[name]()
    Q = g.compile_host(np.float32)["Q"]
    T, B = 20, 3
    rng = np.random.default_rng(78)
    exact = forced = wrapped = 0
    turn = 0
    for integer in (False, True):
        x, tr, il = _case(T, B, g.N, 51 + integer, dtype, integer)
        for K in (1, 3, 8, Q):
            for theta in (np.inf, 2.0, 0.0):
                one = beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, il, K, theta, LW, TS)
                un = BeamStreamRef(tr, g.next, g.weight, g.final, g.start, B, T, K, theta, LW, TS, dtype)
                un.advance(x, il)
                prefix = un.result(False)[0]
                chunkings = list(_chunkings(T, rng))
                for W, P in WP:
                    what = "%s K=%d theta=%s W=%d P=%d" % (name, K, theta, W, P)
                    s = _window(g, tr, B, W, P, K, theta, dtype)
                    cat, trace = _run(s, x, il, list(range(T + 1)))            # frame by frame: the state at every pos
                    at = dict(trace)
                    res = s.result(True)
                    # 1. the search is the one-shot's and the unbounded stream's
                    assert res[0].tobytes() == one[0].tobytes() and s.result(False)[0].tobytes() == prefix.tobytes(), what
                    # 3. committed + tail = the one-shot decode
                    exact += _check_exact(cat, res, one, il, what)
                    forced += int((res[7] & 1).sum())
                    wrapped += sum(1 for b in range(B) if il[b] > W and not res[7][b] & 1)
                    if W - P >= T:
                        assert not res[7].any() & 1
                    # 2. another chunking: the same state at every pos it stops at, the same output in the end
                    cname, cuts = chunkings[turn % len(chunkings)]
                    turn += 1
                    r = _window(g, tr, B, W, P, K, theta, dtype, BeamWindowRef)
                    cat2, trace2 = _run(r, x, il, cuts)
                    for t1, state in trace2:
                        assert state == at[t1] if t1 else all(v[:5] == (0, 0, -1, 0, 0) for v in state), (what, cname, t1)
                    assert cat2 == cat and all(a.tobytes() == b.tobytes() for a, b in zip(r.result(True), res)), (what, cname)
    assert exact > 100 and forced > 0 and wrapped > 0


def test_convergence_with_the_ring_wrapped():
    """K = 1: the set has one slot, so c = pos-1 at every attempt and nothing is ever forced, for any W; and peaky emissions
    -- one label ahead by more than the threshold -- with a wide beam."""
    g = _ngram(6, 2, 7)                                        # no holes: the greedy path has a finite end
    T, B = 60, 2
    x, tr, il = _case(T, B, g.N, 61, np.float32)
    il[:] = T
    for W, P in ((4, 1), (4, 3), (8, 8)):
        s = _window(g, tr, B, W, P, 1, np.inf, np.float32)
        cat, _ = _run(s, x, il, [0, 7, 8, 30, 60])
        res = s.result(True)
        one = beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, il, 1, np.inf, LW, TS)
        for v in s.slots:
            assert v.pos > 5 * W and v.status == 0 and v.base == T // P * P                 # the regime: wrapped, never forced
            assert all(c == pos - 1 and F == 0 for pos, _, c, F in v.attempts) and len(v.attempts) == T // P
        assert res[0].tobytes() == one[0].tobytes()
        assert _check_exact(cat, res, one, il, "K=1 W=%d" % W) == B
    peak = np.full((T, B, g.N), -30.0, np.float32)
    lab = np.random.default_rng(3).integers(0, g.N, size=(T, B))
    np.put_along_axis(peak, lab[..., None], 0.0, -1)
    tr0 = np.zeros_like(tr)
    s = _window(g, tr0, B, 8, 2, 8, 10.0, np.float32)
    cat, _ = _run(s, peak, il, [0, 1, 2, 33, 60])
    one = beam_decode_ref(peak, tr0, g.next, g.weight, g.final, g.start, il, 8, 10.0, LW, TS)
    finite = [b for b in range(B) if one[0][b] > -np.inf]
    assert finite
    for b in finite:
        assert s.slots[b].pos == T > 8 and s.slots[b].status == 0 and s.slots[b].base > T - 8
    assert _check_exact(cat, s.result(True), one, il, "peaky") == len(finite)


@pytest.mark.parametrize("K", [2, 4])
def test_two_components_force_every_full_window(K):
    g = two_components()
    T, B, W, P = 30, 2, 8, 2
    x = two_component_emissions(T, B, g.N, np.float64)
    tr = np.zeros((g.N, g.N))
    il = np.array([T, T - 3])
    s = _window(g, tr, B, W, P, K, np.inf, np.float64)
    cat, trace = _run(s, x, il, [0, 5, 6, 17, 30])
    for b, v in enumerate(s.slots):
        # the regime: no attempt ever converged, and from the first full window on every attempt forced P frames
        assert v.status == 1 and all(c is None for _, _, c, _ in v.attempts)
        assert [F for pos, _, _, F in v.attempts if pos > W - P] == [P] * sum(1 for pos, _, _, _ in v.attempts if pos > W - P)
        assert v.base == v.pos // P * P - (W - P) == len(cat[b][0])
    # the same outputs for another chunking (property 4), and the scores are still the one-shot's (property 1)
    r = _window(g, tr, B, W, P, K, np.inf, np.float64, BeamWindowRef)
    cat2, _ = _run(r, x, il, list(range(T + 1)))
    assert cat2 == cat and all(a.tobytes() == b.tobytes() for a, b in zip(r.result(True), s.result(True)))
    one = beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, il, K, np.inf, LW, TS)
    assert s.result(True)[0].tobytes() == one[0].tobytes() and (one[0] > -np.inf).all()
    # a forced prefix is a path of the automaton all the same: committed + tail has the length of the utterance
    res = s.result(True)
    assert [len(cat[b][0]) + int((res[1][b] >= 0).sum()) for b in range(B)] == il.tolist()


def test_a_window_that_can_hold_the_utterance_never_forces():
    g = GRAPHS["random"]()
    Q = g.compile_host(np.float32)["Q"]
    T, B = 20, 3
    x, tr, il = _case(T, B, g.N, 63, np.float64)
    one = beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, il, Q, np.inf, LW, TS)
    for W, P in ((T + 1, 1), (T + 4, 4), (2 * T, T)):
        assert W - P >= T
        s = _window(g, tr, B, W, P, Q, np.inf, np.float64)
        cat, _ = _run(s, x, il, [0, 3, 3, 11, 20])
        res = s.result(True)
        assert not res[7].any() and all(F == 0 for v in s.slots for _, _, _, F in v.attempts)
        assert res[0].tobytes() == one[0].tobytes()
        assert _check_exact(cat, res, one, il, "W=%d" % W) == int((one[0] > -np.inf).sum()) > 0


def test_a_beam_that_empties_after_a_commit():
    g = _ngram(6, 2, 7)
    T, B, K, W, P = 14, 2, 3, 4, 2
    x, tr, _ = _case(T, B, g.N, 65, np.float32)
    x[9] = -np.inf                                            # nothing survives frame 9
    il = np.array([T, 8])
    s = _window(g, tr, B, W, P, K, np.inf, np.float32)
    cat, trace = _run(s, x, il, [0, 6, 12, 14])
    v = s.slots[0]
    before = dict(trace)[6][0]
    assert before[1] > 0 and v.base >= before[1] and v.aq.size == 0 and v.pos == T        # committed, then emptied
    assert max(pos for pos, _, _, _ in v.attempts) <= 9                                   # no attempt on an empty set
    res = s.result(True)
    assert res[0][0] == -np.inf and (res[1][0] == -1).all() and res[3][0] == 0 and res[7][0] & 2
    assert res[6][0] == v.base == len(cat[0][0]) and res[5][0] == T                      # what was committed stays committed
    assert res[0][1] > -np.inf and not res[7][1] & 2
    # the committed frames are a prefix of what the search held before it emptied
    un = BeamStreamRef(tr, g.next, g.weight, g.final, g.start, 1, T, K, np.inf, LW, TS, np.float32)
    un.advance(x[:9, :1])
    if not v.status & 1:
        assert cat[0][0] == un.result(False)[1][0, :v.base].tolist()


def test_reset_and_result_leave_the_rest_alone():
    g = GRAPHS["trigram6"]()
    T, B = 16, 3
    x, tr, il = _case(T, B, g.N, 67, np.float32)
    il[:] = T
    s = _window(g, tr, B, 5, 2, 4, 3.0, np.float32)
    s.advance(x[:7])
    a = s.result(False)
    b = s.result(True)
    assert all(u.tobytes() == w.tobytes() for u, w in zip(a, s.result(False))) and (b[5] == 7).all()
    s.reset(np.array([0, 1, 0]))
    assert [(v.pos, v.base, v.carry, v.status) for v in s.slots][1] == (0, 0, -1, 0) and s.slots[0].pos == 7
    r = s.result()
    assert r[0][1] == -np.inf and r[5].tolist() == [7, 0, 7] and r[6][1] == 0
    out = s.advance(x[:0])                                    # a chunk of no frames: the empty outputs
    assert out[0].shape == (B, 5) and (out[0] == -1).all() and not out[3].any() and not out[4].any()
