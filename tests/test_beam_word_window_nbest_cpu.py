"""CPU tests of the n best hypotheses of the windowed word-LM beam stream: the restatement over the window's carried state
(tests/beam_word_window_nbest_ref.py) against the n-best restatement of the GROWING stream (tests/beam_word_nbest_ref.py,
tests/beam_word_la_nbest_ref.py) fed the same frames and against the window's own one-best (tests/beam_word_window_ref.py,
tests/beam_word_la_stream_ref.py) -- the required properties of include/asg_hip.h::asg_beam_word_window_nbest at every position a
chunking stops at.  Every regime is asserted from the restatements' own records before anything is compared; no kernel is launched
here."""
import numpy as np
import pytest

from beam_word_cases import arpa_lm, eighths, integers, small_lexicon
from beam_word_la_nbest_ref import BeamWordLaNbestStreamRef
from beam_word_la_stream_ref import BeamWordLaWindowRef
from beam_word_nbest_ref import BeamWordNbestStreamRef
from beam_word_window_nbest_ref import SEQS, word_window_nbest
from beam_word_window_ref import BeamWordWindowRef
from torch_asg_amd import BeamWordWindowNbest as SUBJECT  # noqa: F401  (what the restatement restates)

LW, WS, TS = 0.7, -0.4, 0.3
ALL = 1024                                                 # more than every pair of the small cases
SEP = 4                                                    # the small lexicon's separator
WP = [(8, 2), (16, 4), (5, 5)]
SCORES = [0.5, -1.0, 0.0, 2.0, -0.25]
T = 40
SHARED = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths")


def emissions(T, B, seed, dtype, integer=False):
    rng = np.random.default_rng(seed)
    if integer:
        x = rng.integers(-2, 3, size=(T, B, 5)).astype(dtype)
        tr = np.zeros((5, 5), dtype)
    else:
        x = rng.normal(size=(T, B, 5)).astype(dtype)
        tr = rng.normal(size=(5, 5)).astype(dtype)
    il = rng.integers(T // 2, T + 1, size=B)
    il[0] = T
    return x, tr, il


def language(order, weights):
    """A bigram with missing pairs or a trigram, the weights in eighths or integers (ties exist)."""
    keep = (1.0, 0.5) if order == 2 else (1.0, 0.5, 0.5)
    return (eighths if weights == "eighths" else integers)(arpa_lm(5, order, 60 + order, keep=keep))


def pair_of_streams(lex, lm, tr, B, W, P, K, theta, dtype, la=None, frames=T):
    """The window restatement and the growing n-best restatement it is held to."""
    if la is None:
        return (BeamWordWindowRef(tr, lex, lm, B, W, P, K, theta, LW, WS, TS, dtype),
                BeamWordNbestStreamRef(tr, lex, lm, B, frames, K, theta, LW, WS, TS, dtype))
    return (BeamWordLaWindowRef(tr, lex, lm, la, B, W, P, K, theta, LW, WS, TS, dtype),
            BeamWordLaNbestStreamRef(tr, lex, lm, la, B, frames, K, theta, LW, WS, TS, dtype))


def chunkings(T, rng):
    inner = np.sort(rng.integers(0, T + 1, size=int(rng.integers(3, 8)))).tolist()
    return [("ones", list(range(T + 1))), ("whole", [0, T]), ("random", [0, 0] + inner + [inner[-1], T])]


def drive(win, grow, x, il, cuts):
    """Feed both by the chunks x[t0:t1]; -> after every chunk (t1, per slot the five lists of everything `advance` committed)."""
    cat = [[[] for _ in SEQS] for _ in range(win.B)]
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        n = np.clip(il - t0, 0, t1 - t0)
        out = win.advance(x[t0:t1], n)
        grow.advance(x[t0:t1], n)
        np_, ns, nl, nt, nw, nf, tl, wl = out
        for b in range(win.B):
            for i, (a, m) in enumerate(zip((np_, ns, nl, nt, nw), (nf[b], nf[b], nf[b], tl[b], wl[b]))):
                cat[b][i].extend(a[b, :m].tolist())
        yield t1, cat


def check(win, grow, cat, nbests, seen, what):
    """Everything the issue asks at one position, prefix and final; `seen` counts the regimes met."""
    s = win.s
    for final in (False, True):
        want = grow.result_nbest(max(nbests), final)
        one = win.result(final)
        cands = [grow.search.candidates(g, final) if g.pos else [] for g in grow.slots]
        for nb in nbests:
            got = word_window_nbest(win, nb, final)
            # scores and num_hyps: the growing stream's, byte for byte
            assert got["scores"].tobytes() == np.ascontiguousarray(want["scores"][:, :nb]).tobytes(), what
            assert got["num_hyps"].tobytes() == np.minimum(want["num_cands"], nb).tobytes(), what
            for n in ("frames", "committed", "status"):
                assert got[n].tobytes() == one[n].tobytes(), (n, what)
            for b, v in enumerate(win.slots):
                nh = int(got["num_hyps"][b])
                tail = v.pos - v.base if nh else 0
                recs = got["records"][b]
                assert len(recs) == nh
                for r in range(nb):
                    lens = dict(path=tail, states=tail, lm_states=tail, tokens=int(got["token_lengths"][b, r]),
                                words=int(got["word_lengths"][b, r]))
                    if r >= nh:
                        assert got["scores"][b, r] == -np.inf and not lens["tokens"] and not lens["words"], what
                        assert all((got[n][b, r] == -1).all() for n in SEQS), what
                        continue
                    assert all((got[n][b, r, lens[n]:] == -1).all() and (got[n][b, r, :lens[n]] >= 0).all() or v.status & 1
                               for n in SEQS), what
                    assert recs[r]["pair"] == cands[b][r][1] and recs[r]["tail"] == tail
                    if not v.status & 1:                     # commits + tail of every row: the growing stream's row
                        full = dict(path=v.pos, states=v.pos, lm_states=v.pos, tokens=int(want["token_lengths"][b, r]),
                                    words=int(want["word_lengths"][b, r]))
                        for i, n in enumerate(SEQS):
                            assert cat[b][i] + got[n][b, r, :lens[n]].tolist() == want[n][b, r, :full[n]].tolist(), (n, r, what)
                        seen["exact"] += 1
                    else:                                    # still exactly its chain
                        pairs = win._walk(v, cands[b][r][1], v.pos - 1, v.base)
                        out = ([], [], [], [], [])
                        win._append(v.carry, v.carry_state, pairs, out)
                        h, q = cands[b][r][1]
                        if final and s.state[q] != 0:
                            out[4].append(int(s.wos[s.state[q]]))
                        for n, o in zip(("path", "states", "lm_states", "tokens", "words"), out):
                            assert got[n][b, r, :lens[n]].tolist() == o, (n, r, what)
                        seen["forced"] += 1
                    seen["sep0_late"] += int(r > 0 and recs[r]["sep0"])
                    seen["empty_tail"] += int(tail == 0)
                    seen["final_word_behind_empty_tail"] += int(tail == 0 and final and lens["words"] == 1)
                qs = {}
                for rec in recs:
                    qs.setdefault(rec["pair"][1], set()).add(rec["pair"][0])
                seen["one_q_two_histories"] += int(any(len(hs) > 1 for hs in qs.values()))
                seen["emptied"] += int(got["status"][b] & 2 != 0)
                seen["pos0"] += int(v.pos == 0)
                # row 0: the window's own one-best
                for n in SHARED:
                    assert np.ascontiguousarray(got[n][b, 0]).tobytes() == np.ascontiguousarray(one[n][b]).tobytes(), (n, what)
    return seen


def new_seen():
    return dict(exact=0, forced=0, sep0_late=0, empty_tail=0, final_word_behind_empty_tail=0, one_q_two_histories=0, emptied=0,
                pos0=0)


# (every LM with both kinds of weights, each dtype under both LMs and both kinds of weights: the dtypes alternate over the four)
@pytest.mark.parametrize("order,weights,dtype", [(2, "eighths", np.float32), (2, "integers", np.float64), (3, "eighths", np.float64),
                                                 (3, "integers", np.float32)],
                         ids=["bigram-eighths-f32", "bigram-integers-f64", "trigram-eighths-f64", "trigram-integers-f32"])
def test_the_grid_at_every_position_a_chunking_stops_at(order, weights, dtype):
    lex, lm = small_lexicon(SCORES), language(order, weights)
    B = 2
    x, tr, il = emissions(T, B, 11 + order, dtype, integer=weights == "integers")
    rng = np.random.default_rng(78 + order)
    seen = new_seen()
    turn = 0
    for K in (1, 3, 8, ALL):
        for theta in (np.inf, 2.0, 0.0):
            cks = chunkings(T, rng)
            for W, P in WP:
                # (the three chunkings take turns over the grid: every K, every threshold and every (W, P) meets each of them)
                cname, cuts = cks[turn % 3]
                turn += 1
                what = "K=%d theta=%s W=%d P=%d %s" % (K, theta, W, P, cname)
                win, grow = pair_of_streams(lex, lm, tr, B, W, P, K, theta, dtype)
                check(win, grow, None, (1,), seen, what)                      # pos == 0
                for t1, cat in drive(win, grow, x, il, cuts):
                    # (frame by frame: the longest list at every position, the four sizes at every fourth and at the end)
                    few = cname == "ones" and t1 % 4 and t1 < T
                    check(win, grow, cat, (K + 5,) if few else (1, 2, K, K + 5), seen, what + " t=%d" % t1)
            turn += 1                                                          # (... and every (W, P) another one each time)
    assert seen["exact"] > 1000 and seen["forced"] > 0 and seen["sep0_late"] > 0 and seen["empty_tail"] > 0 and seen["pos0"] > 0
    assert seen["one_q_two_histories"] > 0


@pytest.mark.parametrize("la,dtype", [(1, np.float32), (2, np.float64)], ids=["1-f32", "2-f64"])
def test_the_same_with_look_ahead(la, dtype):
    """Against BeamWordLaNbestStreamRef: prefix scores are without the estimate, the forced commit follows v - L."""
    lex, lm = small_lexicon(SCORES), language(3, "eighths")
    B = 2
    x, tr, il = emissions(T, B, 21 + la, dtype)
    rng = np.random.default_rng(5 + la)
    seen = new_seen()
    for K, theta in ((1, np.inf), (3, 2.0), (ALL, np.inf)):
        cks = chunkings(T, rng)
        for i, (W, P) in enumerate(WP):
            cname, cuts = cks[i]
            what = "la=%d K=%d theta=%s W=%d P=%d %s" % (la, K, theta, W, P, cname)
            win, grow = pair_of_streams(lex, lm, tr, B, W, P, K, theta, dtype, la)
            for t1, cat in drive(win, grow, x, il, cuts):
                check(win, grow, cat, (1, 2, K, K + 5), seen, what + " t=%d" % t1)
    assert seen["exact"] > 100 and seen["forced"] > 0 and seen["empty_tail"] > 0


def word_case(seed, T=24, B=1, dtype=np.float32):
    lex, lm = small_lexicon(SCORES), language(3, "eighths")
    x, tr, _ = emissions(T, B, seed, dtype)
    x[:, :, SEP] += 1.0                                      # (short words: many separator edges)
    return lex, lm, x, tr, np.full(B, T)


def test_a_separator_edge_on_the_first_tail_frame_of_a_later_row_and_two_rows_on_one_state():
    lex, lm, x, tr, il = word_case(3)
    win, grow = pair_of_streams(lex, lm, tr, 1, 8, 2, 8, np.inf, np.float32, frames=24)
    late = shared = 0
    for t1, cat in drive(win, grow, x, il, list(range(25))):
        for final in (False, True):
            got = word_window_nbest(win, 8, final)
            recs = got["records"][0]
            # the regimes, from the restatement's records: column 0 of a row r > 0 is a separator behind the committed label,
            # and its word is the carried state's; two rows end in one product state with different histories
            hit = [r for r, rec in enumerate(recs) if r > 0 and rec["sep0"]]
            v = win.slots[0]
            for r in hit:
                assert got["path"][0, r, 0] == SEP and v.carry not in (SEP, -1) and got["words"][0, r, 0] == win.s.wos[v.carry_state]
            late += len(hit)
            qs = [rec["pair"][1] for rec in recs]
            shared += int(len(set(qs)) < len(qs))
        check(win, grow, cat, (8,), new_seen(), "t=%d" % t1)
    assert late > 0 and shared > 0


def test_a_final_word_behind_an_empty_tail():
    """K = 1, P = 1: every frame is committed at once, so base == pos at every call; a path that stands in a word-end node has
    its word in row 0 and nothing else."""
    lex, lm, x, tr, il = word_case(1)
    win, grow = pair_of_streams(lex, lm, tr, 1, 4, 1, 1, np.inf, np.float32, frames=24)
    seen = new_seen()
    for t1, cat in drive(win, grow, x, il, list(range(25))):
        v = win.slots[0]
        assert v.base == v.pos == t1                           # the regime
        check(win, grow, cat, (1, 3), seen, "t=%d" % t1)
    assert seen["final_word_behind_empty_tail"] > 0 and seen["forced"] == 0


def test_forced_commits_leave_every_row_its_own_chain():
    lex, lm = small_lexicon(SCORES), language(2, "eighths")
    x, tr, _ = emissions(30, 2, 64, np.float64)
    x *= 0.05                                                # flat emissions: the hypotheses stay apart
    il = np.array([30, 27])
    win, grow = pair_of_streams(lex, lm, tr * 0.05, 2, 6, 2, ALL, np.inf, np.float64, frames=30)
    seen = new_seen()
    for t1, cat in drive(win, grow, x, il, [0, 5, 6, 17, 30]):
        check(win, grow, cat, (1, 7, ALL), seen, "t=%d" % t1)
    assert all(v.status == 1 and sum(F for _, _, _, F in v.attempts) > 0 for v in win.slots) and seen["forced"] > 0


def test_a_beam_that_empties_pos_zero_and_a_masked_reset():
    lex, lm = small_lexicon(SCORES), language(2, "eighths")
    x, tr, _ = emissions(14, 3, 65, np.float32)
    x[9, 0] = -np.inf                                          # nothing survives frame 9 in slot 0
    il = np.array([14, 8, 0])
    win, grow = pair_of_streams(lex, lm, tr, 3, 4, 2, 3, np.inf, np.float32, frames=14)
    seen = new_seen()
    for t1, cat in drive(win, grow, x, il, [0, 6, 12, 14]):
        check(win, grow, cat, (1, 3, 8), seen, "t=%d" % t1)
    got = word_window_nbest(win, 3, True)
    assert got["status"][0] & 2 and got["num_hyps"].tolist()[0::2] == [0, 0] and got["num_hyps"][1] > 0          # the regimes
    assert got["frames"].tolist() == [14, 8, 0] and seen["emptied"] > 0 and seen["pos0"] > 0
    assert (got["scores"][0] == -np.inf).all() and all((got[n][0] == -1).all() and (got[n][2] == -1).all() for n in SEQS)
    # a masked reset in mid-stream: the slot starts over, the others go on; then all of them run on
    mask = np.array([1, 0, 0])
    win.reset(mask)
    grow.reset(mask)
    got = word_window_nbest(win, 3, False)
    assert got["frames"].tolist() == [0, 8, 0] and got["num_hyps"][0] == 0 and got["committed"][0] == 0
    cat = None
    x2, _, _ = emissions(10, 3, 66, np.float32)
    for t1, cat in drive(win, grow, x2, np.array([10, 0, 10]), [0, 4, 10]):
        pass
    # (slot 1 committed frames before this second drive: only the slots that began with it are held to the growing stream)
    for final in (False, True):
        got, want = word_window_nbest(win, 3, final), grow.result_nbest(3, final)
        assert got["scores"].tobytes() == want["scores"].tobytes() and got["num_hyps"].tobytes() == want["num_hyps"].tobytes()
        for b in (0, 2):
            v = win.slots[b]
            assert v.pos == 10 and got["num_hyps"][b] > 0
            if not v.status & 1:
                for r in range(int(got["num_hyps"][b])):
                    assert cat[b][0] + got["path"][b, r, :v.pos - v.base].tolist() == want["path"][b, r, :10].tolist()


def test_the_state_is_only_read():
    lex, lm, x, tr, il = word_case(5, B=2)
    win, grow = pair_of_streams(lex, lm, tr, 2, 8, 2, 8, 3.0, np.float32, frames=24)
    for _ in drive(win, grow, x, il, [0, 13]):
        pass
    before = [(v.pos, v.base, v.carry, v.carry_state, v.status, list(v.A), list(v.ring)) for v in win.slots]
    a = word_window_nbest(win, 5, True)
    b = word_window_nbest(win, 5, False)
    assert before == [(v.pos, v.base, v.carry, v.carry_state, v.status, list(v.A), list(v.ring)) for v in win.slots]
    a2 = word_window_nbest(win, 5, True)
    assert all(np.asarray(a[n]).tobytes() == np.asarray(a2[n]).tobytes() for n in a if n != "records")
    assert a["scores"].tobytes() != b["scores"].tobytes()
