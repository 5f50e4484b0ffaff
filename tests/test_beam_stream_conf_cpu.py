"""CPU tests that pin the numpy restatement of the lattice-keeping beam stream (tests/beam_stream_conf_ref.py) before the GPU tests
compare the kernels with it: `final=True` against tests/beam_conf_ref.py on the whole utterance, byte for byte, for every way of
cutting the utterance and of placing `result_confidence` calls between the chunks; the prefix mode against the enumeration of all
label paths inside the kept sets; the properties the specification states; the edge cases of a stream.  No kernel is launched."""
import itertools

import numpy as np
import pytest

from beam_conf_ref import beam_conf_ref, start_frames, window_confidences
from beam_loss_cases import GRAPHS, _lexicon, _ngram, _random_graph
from beam_stream_conf_ref import BeamStreamConfRef
from beam_stream_ref import BeamStreamRef
from graph_decode_ref import path_score_graph
from graph_loss_ref import Composed, _lse
from test_beam_loss_cpu import _path_states

INF = float("inf")
W = (0.8, 0.2)                                                             # lm_weight, token_score
NAMES = ["unigram", "trigram_holes", "random", "lexicon"]                 # the four automata of tests/beam_loss_cases.py
SMALL = {                                                                  # ... over N = 4 tokens, so that every path can be enumerated
    "unigram": lambda: _ngram(4, 1, 1),
    "trigram_holes": lambda: _ngram(4, 3, 3, holes=True),
    "random": lambda: _random_graph(8, 4, 4),
    "lexicon": lambda: _lexicon(4, 12, 5, maxlen=3),
}
WIDE = ("path", "tokens", "states", "token_frames")


def _emissions(T, B, N, seed, dt=np.float64, scale=1.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.normal(size=(T, B, N))).astype(dt), (0.5 * rng.normal(size=(N, N))).astype(dt)


def _stream(g, tr, B, M, K, th=INF, dt=np.float64):
    return BeamStreamConfRef(tr, g.next, g.weight, g.final, g.start, B, M, K, th, *W, dtype=dt)


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
    """A stream result (width M >= T) against beam_conf_ref's (width T): byte for byte on the columns, padding beyond."""
    for n in ("scores", "normalisers", "token_lengths"):
        assert got[n].dtype == want[n].dtype and got[n].tobytes() == want[n].tobytes(), (what, n)
    for n in WIDE:
        assert np.array_equal(got[n][:, :T], want[n]) and (got[n][:, T:] == -1).all(), (what, n)
    assert got["token_confidences"][:, :T].tobytes() == want["token_confidences"].tobytes(), what
    assert (got["token_confidences"][:, T:] == 0).all(), what


# ---------------------------------------------------------------------------------------------------------------- final = True
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("name", NAMES)
def test_final_equals_the_one_shot_confidences_for_every_cut_and_every_placement_of_calls(name, dt):
    g = GRAPHS[name]()
    Q = Composed(g.next, g.weight, g.final, g.start, *W).Q
    T, B, M = 8, 3, 10
    x, tr = _emissions(T, B, g.N, 7, dt)
    lens = np.array([T, 0, 5])
    rng = np.random.default_rng(11)
    checked = 0
    for K in (1, 3, 8, Q):
        for th in (INF, 2.0):
            want = beam_conf_ref(x, tr, g.next, g.weight, g.final, g.start, lens, K, th, *W, 0)
            if K == 3 and th == INF:                                       # the windows of another tolerance, once directly
                w5 = beam_conf_ref(x, tr, g.next, g.weight, g.final, g.start, lens, K, th, *W, 5)
                assert w5["token_confidences"].tobytes() == window_confidences(want, lens, 5).tobytes()
            for kind, calls in (("ones", "every"), ("one", "none"), ("random", "some"), ("random", "every")):
                cuts = _cuts(kind, T, rng)
                at = {"none": set(), "every": set(range(len(cuts))), "some": set(range(1, len(cuts), 2))}[calls]
                s = _stream(g, tr, B, M, K, th, dt)
                _feed(s, x, lens, cuts, at)
                for tol in (0, 1, 5):
                    got = s.result_confidence(tol, final=True)
                    ref = dict(want, token_confidences=window_confidences(want, lens, tol))
                    _same(got, ref, T, (name, K, th, kind, calls, tol))
                    assert np.array_equal(got["frames"], lens) and (got["status"] == 0).all()
                    checked += 1
    assert checked == 4 * 2 * 4 * 3


# ---------------------------------------------------------------------------------------------------------------- prefix mode
@pytest.mark.parametrize("name", sorted(SMALL))
def test_prefix_events_are_the_sum_over_exactly_the_label_paths_inside_the_kept_sets(name):
    g = SMALL[name]()
    T, N = 5, 4
    x, tr = _emissions(T, 1, N, 41)
    comp = Composed(g.next, g.weight, g.final, g.start, *W)
    zero = np.zeros_like(np.asarray(g.final, np.float64))                 # a prefix ends anywhere with weight 0
    pruned = 0
    for K in (10_000, 1, 2, 3, 8):
        s = _stream(g, tr, 1, T, K)
        for L in range(1, T + 1):                                         # cut after every frame
            s.advance(x[L - 1:L])
            res = {tol: s.result_confidence(tol, final=False) for tol in (0, 1, 5)}
            sets = [set(int(q) for q in u) for u in res[0]["sets"][0]]
            assert len(sets) == L
            inside, total = [], 0
            for labels in itertools.product(range(N), repeat=L):          # all 4^L label paths (1024 at L = 5)
                qs = _path_states(labels, g.next, comp.present, g.start, comp)
                if qs is None:
                    continue
                v = path_score_graph(x[:L, 0], tr, g.next, g.weight, zero, labels, g.start, *W)[0]
                if v > -np.inf:
                    total += 1
                    if all(q in sets[t] for t, q in enumerate(qs)):
                        inside.append((v, labels))
            pruned += len(inside) < total
            if not inside:
                assert res[0]["normalisers"][0] == -np.inf and res[0]["scores"][0] == -np.inf
                continue
            Z = _lse([v for v, _ in inside])
            assert np.allclose(res[0]["normalisers"][0], Z, rtol=1e-9, atol=1e-9), (K, L)
            direct = np.zeros((L, N))
            for v, labels in inside:
                for t in start_frames(labels):
                    direct[t, labels[t]] += np.exp(v - Z)
            assert np.allclose(res[0]["events"][0], direct, rtol=1e-9, atol=1e-9), (K, L)
            assert np.allclose(direct[0].sum(), 1.0, rtol=1e-9)           # sum_i P(i, 0) = 1
            best = max(inside, key=lambda it: it[0])
            sk = start_frames(best[1])
            n = int(res[0]["token_lengths"][0])
            assert n == len(sk) and [best[1][t] for t in sk] == list(res[0]["tokens"][0, :n])
            assert np.allclose(res[0]["scores"][0], best[0], rtol=1e-9, atol=1e-9)
            plain = s.result(False)
            for tol in (0, 1, 5):
                r = res[tol]
                for f, v in zip(("scores", "path", "tokens", "token_lengths", "states", "frames", "status"), plain):
                    assert np.array_equal(r[f], v)                         # the hypothesis is result(final=False)'s
                assert list(r["token_frames"][0, :n]) == sk and (r["token_frames"][0, n:] == -1).all()
                assert (r["token_confidences"][0, n:] == 0).all()
                for k, t0 in enumerate(sk):
                    w = direct[max(0, t0 - tol):min(L - 1, t0 + tol) + 1, best[1][t0]].sum()
                    assert np.allclose(r["token_confidences"][0, k], w, rtol=1e-9, atol=1e-9), (K, L, tol, k)
    assert pruned >= 3


@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_the_bounds_at_tolerance_0_the_starts_at_frame_0_and_the_single_path_of_a_beam_of_1(name, final):
    g = GRAPHS[name]()
    T, B = 9, 4
    x, tr = _emissions(T, B, g.N, 5)
    seen = 0
    for K in (1, 4, 16):
        s = _stream(g, tr, B, T, K)
        for a in range(0, T, 3):
            s.advance(x[a:a + 3])
            r = s.result_confidence(0, final=final)
            for b in range(B):
                n, Z = int(r["token_lengths"][b]), r["normalisers"][b]
                if not np.isfinite(r["scores"][b]):
                    assert n == 0
                    continue
                seen += 1
                assert np.isfinite(Z) and r["scores"][b] <= Z + 1e-9
                c = r["token_confidences"][b, :n]
                assert (c >= np.exp(r["scores"][b] - Z) - 1e-9).all() and (c <= 1 + 1e-9).all()
                assert np.allclose(r["events"][b][0].sum(), 1.0, rtol=1e-9)
                if K == 1:                                                 # one path: it is sure of itself
                    assert np.allclose(c, 1.0, rtol=1e-9) and np.allclose(Z, r["scores"][b], rtol=1e-9, atol=1e-9)
    assert seen > 10


# ---------------------------------------------------------------------------------------------------------------- edge cases
def test_no_frame_one_frame_an_emptied_beam_and_an_end_without_a_final_weight():
    g = GRAPHS["unigram"]()
    x, tr = _emissions(6, 3, g.N, 9)
    s = _stream(g, tr, 3, 6, 3)
    for final in (False, True):                                            # L = 0
        r = s.result_confidence(2, final=final)
        assert (r["scores"] == -INF).all() and (r["normalisers"] == -INF).all() and (r["token_lengths"] == 0).all()
        assert all((r[n] == -1).all() for n in WIDE) and (r["token_confidences"] == 0).all() and (r["frames"] == 0).all()
    s.advance(x[:1], np.array([1, 0, 1]))                                  # L = 1 in slots 0 and 2
    r = s.result_confidence(0, final=False)
    assert list(r["token_lengths"]) == [1, 0, 1] and r["token_frames"][0, 0] == 0 and r["normalisers"][1] == -INF
    assert np.isfinite(r["normalisers"][[0, 2]]).all() and not np.isnan(r["token_confidences"]).any()
    x[3:, 0] = -INF                                                        # slot 0: every candidate of frame 3 is -inf
    s.advance(x[1:])
    for final in (False, True):
        r = s.result_confidence(1, final=final)
        assert s.sizes()[0][2] > 0 and s.sizes()[0][3:] == [0, 0, 0]
        assert r["scores"][0] == -INF and r["normalisers"][0] == -INF and r["token_lengths"][0] == 0
        assert (r["token_frames"][0] == -1).all() and (r["token_confidences"][0] == 0).all()
        assert np.isfinite(r["normalisers"][1:]).all() and not np.isnan(r["token_confidences"]).any()
    # three tokens or more end in the state that rejects: no finite END, but prefixes there are
    nxt = np.array([[1, 1, 1], [2, 2, 2], [2, 2, 2]])
    fin = np.array([0.0, 0.5, -np.inf])
    xs = np.full((6, 1, 3), -9.0)
    for t, i in enumerate([0, 1, 2, 0, 0, 1]):
        xs[t, 0, i] = 0.0
    d = BeamStreamConfRef(np.zeros((3, 3)), nxt, np.zeros((3, 3)), fin, 0, 1, 6, 2, INF, *W, dtype=np.float64)
    d.advance(xs)
    r = d.result_confidence(0, final=True)
    assert d.sizes()[0][5] > 0 and r["normalisers"][0] == -INF and r["scores"][0] == -INF and r["token_lengths"][0] == 0
    assert (r["token_confidences"] == 0).all()
    r = d.result_confidence(0, final=False)
    assert np.isfinite(r["normalisers"][0]) and r["token_lengths"][0] >= 3


def test_a_masked_reset_in_mid_stream_takes_apos_back_in_the_chosen_slots_only():
    g = GRAPHS["random"]()
    x, tr = _emissions(8, 3, g.N, 13, np.float32)
    s = _stream(g, tr, 3, 8, 4, dt=np.float32)
    s.advance(x[:3])
    s.result_confidence(0)
    assert [sl.apos for sl in s.slots] == [3, 3, 3]
    s.advance(x[3:5])
    s.reset(np.array([0, 1, 0]))
    assert [sl.apos for sl in s.slots] == [3, 0, 3] and [sl.pos for sl in s.slots] == [5, 0, 5]
    s.advance(x[5:8])
    got = s.result_confidence(1, final=True)
    assert [sl.apos for sl in s.slots] == [8, 3, 8]
    whole = beam_conf_ref(x, tr, g.next, g.weight, g.final, g.start, None, 4, INF, *W, 1)
    tail = beam_conf_ref(x[5:8], tr, g.next, g.weight, g.final, g.start, None, 4, INF, *W, 1)
    for b, (ref, T) in enumerate([(whole, 8), (tail, 3), (whole, 8)]):
        one = {n: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for n, v in got.items()}
        _same(one, {n: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for n, v in ref.items()}, T, b)


def test_the_clamp_at_max_frames_and_the_status_word():
    g = GRAPHS["unigram"]()
    x, tr = _emissions(9, 2, g.N, 15)
    s = _stream(g, tr, 2, 6, 4)
    s.advance(x[:4], np.array([4, 2]))
    s.advance(x[4:9], np.array([5, 4]))                                    # slot 0: 4 + 5 > 6 frames, slot 1: 2 + 4 = 6 exactly
    r = s.result_confidence(2, final=True)
    assert list(r["frames"]) == [6, 6] and list(r["status"]) == [1, 0]
    x1 = np.concatenate([x[:2, 1], x[4:8, 1]])[:, None]
    for b, xb in ((0, x[:6, 0:1]), (1, x1)):
        want = beam_conf_ref(xb, tr, g.next, g.weight, g.final, g.start, None, 4, INF, *W, 2)
        one = {n: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for n, v in r.items()}
        _same(one, want, 6, b)


def test_result_confidence_leaves_the_search_alone():
    g = GRAPHS["trigram_holes"]()
    x, tr = _emissions(7, 2, g.N, 17, np.float32)
    a = _stream(g, tr, 2, 7, 5, 3.0, np.float32)
    b = BeamStreamRef(tr, g.next, g.weight, g.final, g.start, 2, 7, 5, 3.0, *W, dtype=np.float32)
    for lo in range(0, 7, 2):
        a.advance(x[lo:lo + 2])
        b.advance(x[lo:lo + 2])
        for final in (False, True):
            a.result_confidence(1, final=final)
        for sa, sb in zip(a.slots, b.slots):                               # pos, the set, the back-pointers
            assert sa.pos == sb.pos and np.array_equal(sa.aq, sb.aq) and np.array_equal(sa.av, sb.av)
            assert all(np.array_equal(u[0], v[0]) and (u[1] is v[1] is None or np.array_equal(u[1], v[1]))
                       for u, v in zip(sa.history, sb.history))
        for final in (False, True):
            for u, v in zip(a.result(final), b.result(final)):
                assert np.array_equal(u, v)
