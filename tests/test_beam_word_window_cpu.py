"""CPU tests of windowed streaming beam decoding with a lexicon and a word LM: the restatement with explicit carried state and
rings of W rows (tests/beam_word_window_ref.py) against the one-shot restatement (tests/beam_word_ref.py) and the unbounded
stream (tests/beam_word_stream_ref.py) -- search identity, chunk invariance and exactness of the committed prefix, words
included (the required properties of include/asg_hip.h::asg_beam_word_window_advance), the convergence frame of every commit
attempt against a brute-force backtrace of every survivor, the word regimes by name (a separator edge on a commit boundary, on a
call boundary, on the boundary of the tail; a word over three commits; a final word behind an empty tail; two histories on one
product state) and the window regimes on pairs (the ring wrapped, forced commits, a window that never forces, a beam that
empties after a commit).  Every regime is asserted from the restatement's own records before anything is compared -- no kernel
is launched here."""
import numpy as np
import pytest

from beam_word_cases import arpa_lm, eighths, integers, small_lexicon
from beam_word_ref import beam_word_ref
from beam_word_stream_ref import BeamWordStreamRef
from beam_word_window_ref import BeamWordWindowRef
from torch_asg_amd import BeamWordWindowStream as SUBJECT  # noqa: F401  (what the restatement restates)

LW, WS, TS = 0.7, -0.4, 0.3
ALL = 1024                                                 # more than every pair of the small cases
SEP = 4                                                    # the small lexicon's separator
WP = [(1, 1), (2, 1), (2, 2), (5, 1), (5, 3), (5, 5), (16, 1), (16, 3), (16, 16)]       # W in {1, 2, 5, 16} x P in {1, 3, W}, P <= W
WIDE = ("path", "states", "lm_states", "tokens", "words")
SCORES = [0.5, -1.0, 0.0, 2.0, -0.25]


def case(T, B, N, seed, dtype, integer=False):
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


class Recording(BeamWordWindowRef):
    """The restatement that also records the kept pairs of every attempt: `sets` [(pos, sorted pairs)] per slot."""

    def _attempt(self, v, out):
        if not hasattr(v, "sets"):
            v.sets = []
        v.sets.append((v.pos, sorted(p for p, _ in v.A)))
        super()._attempt(v, out)


class Checked(Recording):
    """... with the convergence frame of every attempt checked against brute force: every pair of the current set backtraced
    on its own down to `base`, c = the latest frame at which all those paths hold one pair."""

    def _attempt(self, v, out):
        paths = [self._walk(v, p, v.pos - 1, v.base) for p, _ in v.A]                    # [|A|][pos - base]
        same = [i for i in range(len(paths[0])) if all(pa[i] == paths[0][i] for pa in paths)]
        want = v.base + same[-1] if same else None
        # (ancestries that have met stay together: the frames on which all agree are a prefix)
        assert same == list(range(len(same)))
        super()._attempt(v, out)
        assert v.attempts[-1][2] == want, (v.attempts[-1], want)


def window(lex, lm, tr, B, W, P, K, theta, dtype, cls=Checked):
    return cls(tr, lex, lm, B, W, P, K, theta, LW, WS, TS, dtype)


def run(s, x, il, cuts):
    """Advance by the chunks x[t0:t1]; slot b takes the frames below il[b].  -> per slot the concatenation of everything advance
    returned (the five lists in WIDE's order), per call (cut, state of every slot), and per call and slot (base before the call,
    the call's new path)."""
    B = x.shape[1]
    cat = [tuple([] for _ in WIDE) for _ in range(B)]
    trace, calls = [], []
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        n = np.clip(il - t0, 0, t1 - t0)
        before = [v.base for v in s.slots]
        out = s.advance(x[t0:t1], n)
        np_, ns, nl, nt, nw, nf, tl, wl = out
        for a in out[:5]:
            assert a.shape == (B, s.W + t1 - t0) and a.dtype == np.int64
        for b in range(B):
            for i, (a, m) in enumerate(zip(out[:5], (nf[b], nf[b], nf[b], tl[b], wl[b]))):
                # (forced commits splice paths: the state before a separator may then be no word end, and its word -1)
                assert (a[b, m:] == -1).all() and ((a[b, :m] >= 0).all() or s.slots[b].status & 1)
                cat[b][i].extend(a[b, :m].tolist())
        calls.append([(before[b], np_[b, :nf[b]].tolist()) for b in range(B)])
        trace.append((t1, [(v.pos, v.base, v.carry, v.carry_state, v.status) + tuple(len(c) for c in cat[b])
                           for b, v in enumerate(s.slots)]))
    return cat, trace, calls


def chunkings(T, rng):
    yield "whole", [0, T]
    for i in range(2):
        inner = np.sort(rng.integers(0, T + 1, size=int(rng.integers(2, 8))))
        cuts = [0] + inner.tolist() + [T]
        if i == 0:
            cuts = [0, 0] + cuts[1:] + [T]                   # chunks of no frames at both ends
        yield "random%d" % i, cuts


def check_exact(cat, res, one, il, what):
    """Property 3 for the slots without a forced commit and with a finite one-shot score -> how many there were."""
    n = 0
    for b in range(len(il)):
        L = int(il[b])
        assert res["frames"][b] == L and res["committed"][b] == len(cat[b][0]), what
        if res["status"][b] & 1 or not one["scores"][b] > -np.inf:
            continue
        n += 1
        tail = L - res["committed"][b]
        for i, name in enumerate(WIDE[:3]):
            assert cat[b][i] + res[name][b, :tail].tolist() == one[name][b, :L].tolist(), (name, what)
            assert (res[name][b, tail:] == -1).all(), (name, what)
        for i, name, ln in ((3, "tokens", "token_lengths"), (4, "words", "word_lengths")):
            m = res[ln][b]
            assert cat[b][i] + res[name][b, :m].tolist() == one[name][b, :one[ln][b]].tolist(), (name, what)
            assert (res[name][b, m:] == -1).all(), (name, what)
    return n


def same_results(a, b):
    return all(a[n].dtype == b[n].dtype and a[n].tobytes() == b[n].tobytes() for n in a)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("weights", ["eighths", "integers"])
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_search_identity_chunk_invariance_and_exactness(order, weights, dtype):
    lex = small_lexicon(SCORES)
    lm = (eighths if weights == "eighths" else integers)(arpa_lm(5, order, 60 + order, keep=(1.0, 0.5, 0.5)))
    T, B = 12, 4
    x, tr, il = case(T, B, 5, 11 + order, dtype, integer=weights == "integers")
    rng = np.random.default_rng(78)
    exact = forced = wrapped = words = turn = 0
    for K in (1, 3, 8, ALL):
        for theta in (np.inf, 2.0, 0.0):
            one = beam_word_ref(x, tr, lex, lm, il, K, theta, LW, WS, TS)
            un = BeamWordStreamRef(tr, lex, lm, B, T, K, theta, LW, WS, TS, dtype)
            un.advance(x, il)
            prefix = un.result(False)["scores"]
            cks = list(chunkings(T, rng))
            for W, P in WP:
                what = "K=%d theta=%s W=%d P=%d" % (K, theta, W, P)
                s = window(lex, lm, tr, B, W, P, K, theta, dtype)
                cat, trace, _ = run(s, x, il, list(range(T + 1)))              # frame by frame: the state at every pos
                at = dict(trace)
                res = s.result(True)
                # 1. the search is the one-shot's and the unbounded stream's
                assert res["scores"].tobytes() == one["scores"].tobytes(), what
                assert s.result(False)["scores"].tobytes() == prefix.tobytes(), what
                # 3. committed + tail = the one-shot decode, words included
                exact += check_exact(cat, res, one, il, what)
                forced += int((res["status"] & 1).sum())
                wrapped += sum(1 for b in range(B) if il[b] > W and not res["status"][b] & 1)
                words += sum(len(c[4]) for c in cat)
                if W - P >= T:
                    assert not (res["status"] & 1).any(), what
                # 2. another chunking: the same state at every pos it stops at, the same output in the end
                cname, cuts = cks[turn % len(cks)]
                turn += 1
                r = window(lex, lm, tr, B, W, P, K, theta, dtype, BeamWordWindowRef)
                cat2, trace2, _ = run(r, x, il, cuts)
                for t1, state in trace2:
                    if t1:
                        assert state == at[t1], (what, cname, t1)
                    else:
                        assert all(v == (0, 0, -1, -1, 0, 0, 0, 0, 0, 0) for v in state), (what, cname)
                assert cat2 == cat and same_results(r.result(True), res) and same_results(r.result(False), s.result(False)), \
                    (what, cname)
    assert exact > 100 and forced > 0 and wrapped > 0 and words > 0


# ---- the word regimes.  The case: the small lexicon under a trigram, a beam of 3, a window of 8 committed every 2 frames, and
# K = 1 with P = 1 where every frame is a commit of its own.
def word_case(seed, T=24, dtype=np.float32):
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5)))
    x, tr, _ = case(T, 1, 5, seed, dtype)
    x[:, :, SEP] += 1.0                                      # (short words: many separator edges)
    return lex, lm, x, tr, np.array([T])


def edge_frames(path):
    """The frames t >= 1 of a label path that hold the separator behind another label."""
    return [t for t in range(1, len(path)) if path[t] == SEP and path[t - 1] != SEP]


SEED_BOUNDARY, SEED_TAIL, SEED_THREE, SEED_FINAL, SEED_SHARED = 9, 3, 2, 1, 1     # (seeds at which the restatement shows the regime)


def test_a_separator_edge_on_a_commit_boundary_and_on_a_call_boundary():
    lex, lm, x, tr, il = word_case(SEED_BOUNDARY)
    T = int(il[0])
    one = beam_word_ref(x, tr, lex, lm, il, 3, np.inf, LW, WS, TS)
    outs = []
    for cuts in ([0, T], list(range(T + 1))):
        s = window(lex, lm, tr, 1, 8, 2, 3, np.inf, np.float32)
        cat, _, calls = run(s, x, il, cuts)
        v = s.slots[0]
        path = cat[0][0]
        starts = [f0 for f0, _ in v.commits if f0 in edge_frames(path)]
        assert v.status == 0 and starts                      # the regime: a segment begins with the separator of an edge
        if len(cuts) == 2:
            # ... inside one call, behind an earlier segment of the same call: the word comes from carry_state
            assert len(v.commits) > 1 and all(f0 > v.commits[0][0] for f0 in starts)
        else:
            # ... and as the first frame a call commits: the carries crossed a kernel boundary
            firsts = [base for (base, new), in calls if new and base in starts]
            assert firsts
        assert check_exact(cat, s.result(True), one, il, cuts) == 1
        outs.append(cat)
    assert outs[0] == outs[1]
    assert len(outs[0][0][4]) >= len(starts) > 0


def test_a_separator_edge_on_the_first_frame_of_the_tail():
    lex, lm, x, tr, il = word_case(SEED_TAIL)
    T = int(il[0])
    s = window(lex, lm, tr, 1, 8, 2, 3, np.inf, np.float32, Recording)
    un = BeamWordStreamRef(tr, lex, lm, 1, T, 3, np.inf, LW, WS, TS, np.float32)
    hits = 0
    cat = tuple([] for _ in WIDE)
    for t in range(T):
        out = s.advance(x[t:t + 1])
        un.advance(x[t:t + 1])
        for i in range(5):
            cat[i].extend(out[i][0, :out[(5, 5, 5, 6, 7)[i]][0]].tolist())
        v = s.slots[0]
        r = s.result(False)
        if v.base >= 1 and v.base < v.pos and r["path"][0, 0] == SEP and v.carry != SEP:
            hits += 1                                        # the regime: the tail begins with the separator of an edge
            assert r["words"][0, 0] == lex.word_of_state[v.carry_state] >= 0
        if not v.status & 1:                                 # committed + tail = the unbounded stream's prefix, words included
            u = un.result(False)
            for i, (name, ln) in enumerate((("path", None), ("states", None), ("lm_states", None), ("tokens", "token_lengths"),
                                            ("words", "word_lengths"))):
                m = v.pos - v.base if ln is None else r[ln][0]
                full = v.pos if ln is None else u[ln][0]
                assert cat[i] + r[name][0, :m].tolist() == u[name][0, :full].tolist(), (t, name)
    assert hits > 0 and s.slots[0].status == 0


def test_a_word_whose_frames_span_three_commits():
    lex, lm, x, tr, il = word_case(SEED_THREE)
    T = int(il[0])
    x[:, :, SEP] -= 2.0                                      # (long words)
    one = beam_word_ref(x, tr, lex, lm, il, 3, 1.0, LW, WS, TS)
    s = window(lex, lm, tr, 1, 4, 1, 3, 1.0, np.float32)
    cat, _, _ = run(s, x, il, [0, 5, 6, T])
    v = s.slots[0]
    path = cat[0][0]
    spans = []
    for e in edge_frames(path):
        w0 = e
        while w0 > 0 and path[w0 - 1] != SEP:
            w0 -= 1                                          # the word's first frame
        spans.append(len({i for i, (f0, f1) in enumerate(v.commits) if f0 <= e and f1 >= w0}))
    assert v.status == 0 and spans and max(spans) >= 3       # the regime
    assert len(cat[0][4]) == len(spans)
    assert check_exact(cat, s.result(True), one, il, "three") == 1


def test_a_final_word_with_everything_else_committed():
    lex, lm, x, tr, il = word_case(SEED_FINAL, T=9)
    T = int(il[0])
    one = beam_word_ref(x, tr, lex, lm, il, 1, np.inf, LW, WS, TS)
    s = window(lex, lm, tr, 1, 4, 1, 1, np.inf, np.float32)
    cat, _, _ = run(s, x, il, [0, 4, T])
    v = s.slots[0]
    res, pre = s.result(True), s.result(False)
    # the regime: nothing is left in the tail, and the path ends in a word-end node
    assert v.base == v.pos == T and v.status == 0 and lex.word_of_state[cat[0][1][-1]] >= 0
    assert (res["path"] == -1).all() and res["token_lengths"][0] == 0 and res["scores"][0] > -np.inf
    assert res["word_lengths"][0] == 1 and res["words"][0, 0] == lex.word_of_state[cat[0][1][-1]]
    assert pre["word_lengths"][0] == 0 and (pre["words"] == -1).all()                     # no final word in a prefix
    assert check_exact(cat, res, one, il, "final") == 1


def test_two_histories_on_one_product_state_do_not_converge():
    lex, lm, x, tr, il = word_case(SEED_SHARED)
    T = int(il[0])
    one = beam_word_ref(x, tr, lex, lm, il, 2, np.inf, LW, WS, TS)
    s = window(lex, lm, tr, 1, 8, 1, 2, np.inf, np.float32)
    cat, _, _ = run(s, x, il, [0, 3, T])
    v = s.slots[0]
    # the regime: an attempt whose survivors all sit in ONE product state with different histories, and which did not commit up
    # to its last frame -- a scan over product states would have
    shared = [(pos, c) for (pos, pairs), (pos2, _, c, _) in zip(v.sets, v.attempts)
              if len(pairs) > 1 and len({q for _, q in pairs}) == 1]
    assert shared and all(c is None or c < pos - 1 for pos, c in shared)
    assert check_exact(cat, s.result(True), one, il, "shared") == (0 if v.status & 1 else 1)


# ---- the window regimes, on pairs
def test_convergence_with_the_ring_wrapped():
    """K = 1: the set has one slot, so c = pos-1 at every attempt and nothing is ever forced, for any W; and peaky emissions
    -- one label ahead by more than the threshold -- with a wide beam."""
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 2, 62, keep=(1.0, 1.0)))
    T, B = 60, 2
    x, tr, il = case(T, B, 5, 61, np.float32)
    il[:] = T
    for W, P in ((4, 1), (4, 3), (8, 8)):
        s = window(lex, lm, tr, B, W, P, 1, np.inf, np.float32)
        cat, _, _ = run(s, x, il, [0, 7, 8, 30, 60])
        res = s.result(True)
        one = beam_word_ref(x, tr, lex, lm, il, 1, np.inf, LW, WS, TS)
        for v in s.slots:
            assert v.pos > 5 * W and v.status == 0 and v.base == T // P * P                 # the regime: wrapped, never forced
            assert all(c == pos - 1 and F == 0 for pos, _, c, F in v.attempts) and len(v.attempts) == T // P
        assert res["scores"].tobytes() == one["scores"].tobytes()
        check_exact(cat, res, one, il, "K=1 W=%d" % W)
        assert sum(len(c[4]) for c in cat) > 0
    # peaky: the words 0, 2 and 0 1 spelled out, every label far ahead in its frames
    labs = [0, 0, 4, 2, 4, 4, 0, 1, 1, 4, 2, 2, 4, 0, 4] * 4
    peak = np.full((T, B, 5), -30.0, np.float32)
    peak[np.arange(T), :, labs] = 0.0
    tr0 = np.zeros_like(tr)
    s = window(lex, lm, tr0, B, 8, 2, 8, 10.0, np.float32)
    cat, _, _ = run(s, peak, il, [0, 1, 2, 33, 60])
    one = beam_word_ref(peak, tr0, lex, lm, il, 8, 10.0, LW, WS, TS)
    assert (one["scores"] > -np.inf).all() and one["path"][0].tolist() == labs
    for v in s.slots:
        assert v.pos == T > 8 and v.status == 0 and v.base > T - 8
    assert check_exact(cat, s.result(True), one, il, "peaky") == B


def test_forced_commits_keep_the_specified_outputs():
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 2, 62, keep=(1.0, 0.6)))
    T, B, W, P = 30, 2, 6, 2
    x, tr, _ = case(T, B, 5, 64, np.float64)
    x *= 0.05                                                # flat emissions: the hypotheses stay apart
    il = np.array([T, T - 3])
    s = window(lex, lm, tr * 0.05, B, W, P, ALL, np.inf, np.float64)
    cat, _, _ = run(s, x, il, [0, 5, 6, 17, 30])
    for b, v in enumerate(s.slots):
        assert v.status == 1 and sum(F for _, _, _, F in v.attempts) > 0                 # the regime
        assert v.pos - v.base <= W - P + v.pos % P and v.base == len(cat[b][0])
    # the same outputs for another chunking (property 4), and the scores are still the one-shot's (property 1)
    r = window(lex, lm, tr * 0.05, B, W, P, ALL, np.inf, np.float64, BeamWordWindowRef)
    cat2, _, _ = run(r, x, il, list(range(T + 1)))
    assert cat2 == cat and same_results(r.result(True), s.result(True)) and same_results(r.result(False), s.result(False))
    one = beam_word_ref(x, tr * 0.05, lex, lm, il, ALL, np.inf, LW, WS, TS)
    res = s.result(True)
    assert res["scores"].tobytes() == one["scores"].tobytes() and (one["scores"] > -np.inf).all()
    # a forced prefix is a path of the lexicon all the same: committed + tail has the length of the utterance
    assert [len(cat[b][0]) + int((res["path"][b] >= 0).sum()) for b in range(B)] == il.tolist()


def test_a_window_that_can_hold_the_utterance_never_forces():
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5)))
    T, B = 14, 3
    x, tr, il = case(T, B, 5, 63, np.float64)
    one = beam_word_ref(x, tr, lex, lm, il, ALL, np.inf, LW, WS, TS)
    for W, P in ((T + 1, 1), (T + 4, 4), (2 * T, T)):
        assert W - P >= T
        s = window(lex, lm, tr, B, W, P, ALL, np.inf, np.float64)
        cat, _, _ = run(s, x, il, [0, 3, 3, 11, T])
        res = s.result(True)
        assert not res["status"].any() and all(F == 0 for v in s.slots for _, _, _, F in v.attempts)
        assert res["scores"].tobytes() == one["scores"].tobytes()
        assert check_exact(cat, res, one, il, "W=%d" % W) == int((one["scores"] > -np.inf).sum()) > 0


def test_a_beam_that_empties_after_a_commit():
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 2, 62, keep=(1.0, 1.0)))
    T, B, K, W, P = 14, 2, 3, 4, 2
    x, tr, _ = case(T, B, 5, 65, np.float32)
    x[9] = -np.inf                                            # nothing survives frame 9
    il = np.array([T, 8])
    s = window(lex, lm, tr, B, W, P, K, np.inf, np.float32)
    cat, trace, _ = run(s, x, il, [0, 6, 12, 14])
    v = s.slots[0]
    before = dict(trace)[6][0]
    assert before[1] > 0 and v.base >= before[1] and not v.A and v.pos == T               # committed, then emptied
    assert max(pos for pos, _, _, _ in v.attempts) <= 9                                   # no attempt on an empty set
    res = s.result(True)
    assert res["scores"][0] == -np.inf and res["token_lengths"][0] == 0 and res["word_lengths"][0] == 0 and res["status"][0] & 2
    assert all((res[n][0] == -1).all() for n in WIDE)
    assert res["committed"][0] == v.base == len(cat[0][0]) and res["frames"][0] == T      # what was committed stays committed
    assert res["scores"][1] > -np.inf and not res["status"][1] & 2
    # the committed frames are a prefix of what the search held before it emptied
    un = BeamWordStreamRef(tr, lex, lm, 1, T, K, np.inf, LW, WS, TS, np.float32)
    un.advance(x[:9, :1])
    if not v.status & 1:
        assert cat[0][0] == un.result(False)["path"][0, :v.base].tolist()


def test_reset_and_result_leave_the_rest_alone():
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5)))
    T, B = 16, 3
    x, tr, _ = case(T, B, 5, 67, np.float32)
    s = window(lex, lm, tr, B, 5, 2, 4, 3.0, np.float32)
    s.advance(x[:7])
    a = s.result(False)
    b = s.result(True)
    assert same_results(a, s.result(False)) and (b["frames"] == 7).all()
    s.reset(np.array([0, 1, 0]))
    v = s.slots[1]
    assert (v.pos, v.base, v.carry, v.carry_state, v.status) == (0, 0, -1, -1, 0) and s.slots[0].pos == 7
    r = s.result()
    assert r["scores"][1] == -np.inf and r["frames"].tolist() == [7, 0, 7] and r["committed"][1] == 0
    out = s.advance(x[:0])                                    # a chunk of no frames: the empty outputs
    assert all(o.shape == (B, 5) and (o == -1).all() for o in out[:5]) and not any(o.any() for o in out[5:])
