"""CPU tests of the n best hypotheses of the two token-graph beam streams: the test-side restatement over the streams' carried
state (tests/beam_stream_nbest_ref.py) against the one-shot n-best restatement (tests/beam_nbest_ref.py) for every way of
cutting an utterance into chunks, the prefix mode against exhaustive enumeration, row 0 against result(), the state left alone,
masked reset, the empty cases, and the window's rows as commits + tail -- no kernel is launched here."""
import copy
import itertools

import numpy as np
import pytest

import torch_asg_amd
from beam_loss_cases import GRAPHS
from beam_nbest_ref import beam_nbest_ref
from beam_stream_nbest_ref import _candidates, stream_nbest, window_nbest
from beam_stream_ref import BeamStreamRef
from beam_window_ref import BeamWindowRef, chain_automaton, two_component_emissions, two_components_automaton
from graph_decode_ref import fold, product

LW, TS = 0.8, -0.5


def test_the_public_surface_has_the_two_methods():
    A = torch_asg_amd
    assert callable(A.BeamStream.result_nbest) and callable(A.BeamWindowStream.result_nbest)
    assert A.BeamStreamNbest._fields == ("scores", "graph_scores", "tokens", "token_lengths", "num_hyps", "path", "states", "frames",
                                         "status")
    assert A.BeamWindowNbest._fields == ("scores", "tokens", "token_lengths", "num_hyps", "path", "states", "frames", "committed",
                                         "status")
    assert "BeamStreamNbest" in A.__all__ and "BeamWindowNbest" in A.__all__


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
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        s.advance(x[t0:t1], np.clip(il - t0, 0, t1 - t0))


def _chunkings(T, rng):
    yield "ones", list(range(T + 1))
    yield "whole", [0, T]
    for i in range(2):
        inner = np.sort(rng.integers(0, T + 1, size=int(rng.integers(2, 6))))
        cuts = [0] + inner.tolist() + [T]
        if i == 0:
            cuts = [0, 0] + cuts[1:] + [T]                   # chunks of no frames at both ends
        yield "random%d" % i, cuts


def _same_as_one_shot(got, one, T, what):
    """got: stream_nbest's tuple over max_frames >= T columns; one: beam_nbest_ref's over T columns.  The seven shared arrays
    (scores, graph_scores, tokens, token_lengths, num_hyps, path, states), bytes and not values."""
    sc, gs, tok, tl, nh, path, st = got[:7]
    osc, _, ogs, otok, otl, onh, opath, ost = one
    for a, b in ((sc, osc), (gs, ogs), (tl, otl), (nh, onh)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what
    for a, b in ((tok, otok), (path, opath), (st, ost)):
        assert a.dtype == np.int64 and a[..., :T].tobytes() == np.ascontiguousarray(b).tobytes() and (a[..., T:] == -1).all(), what


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_final_rows_equal_the_one_shot_nbest_for_any_chunking(name, dtype):
    g = GRAPHS[name]()
    Q = g.compile_host(np.float32)["Q"]
    T, B = 12, 4
    rng = np.random.default_rng(78)
    zero_chunks, short, several = False, False, False
    for integer in (False, True):
        x, tr, il = _case(T, B, g.N, 51 + integer, dtype, integer)
        for K in (1, 3, 8, Q):
            for theta in (np.inf, 2.0, 0.0):
                ones = {nb: beam_nbest_ref(x, tr, g.next, g.weight, g.final, g.start, il, K, nb, theta, LW, TS)
                        for nb in (1, 2, K, K + 5)}
                for cname, cuts in _chunkings(T, rng):
                    zero_chunks |= any(a == b for a, b in zip(cuts[:-1], cuts[1:]))
                    s = _stream(g, tr, B, T + 3, K, theta, dtype)
                    _feed(s, x, il, cuts)
                    for nb, one in ones.items():
                        got = stream_nbest(s, nb, True)
                        what = "%s K=%d theta=%s nbest=%d %s" % (name, K, theta, nb, cname)
                        _same_as_one_shot(got, one, T, what)
                        assert np.array_equal(got[7], il) and not got[8].any(), what
                        short |= bool((got[4] < nb).any())
                        several |= bool((got[4] > 1).any())
    assert zero_chunks and short and several


def _enumerate_prefixes(xb, tr, nxt, w, start, lw, ts):
    """Every label path of xb's frames through the composed lattice, WITHOUT a final weight -> {(label, state) at the last
    frame: the best (value, labels, states, graph part)}; the sums formed in the order the specification gives."""
    T, N = xb.shape
    dt = xb.dtype.type
    present, arcw, _ = fold(nxt, w, np.zeros(nxt.shape[0]), dt, lw, ts)
    best = {}
    for labels in itertools.product(range(N), repeat=T):
        i = labels[0]
        if not present[start, i]:
            continue
        s = int(nxt[start, i])
        v, g = arcw[start, i] + xb[0, i], arcw[start, i]
        sts, ok = [s], True
        for t in range(1, T):
            i, j = labels[t], labels[t - 1]
            if i == j:
                v = (v + tr[i, i]) + xb[t, i]
            else:
                if not present[s, i]:
                    ok = False
                    break
                v = ((v + tr[i, j]) + arcw[s, i]) + xb[t, i]
                g = g + arcw[s, i]
                s = int(nxt[s, i])
            sts.append(s)
        if not ok or not v > -np.inf:
            continue
        key = (labels[-1], s)
        if key not in best or v > best[key][0]:
            best[key] = (v, labels, sts, g)
    return best


@pytest.mark.parametrize("seed", range(3))
def test_the_prefix_rows_against_exhaustive_enumeration(seed):
    """T = 5, N = 4: the 1024 label paths.  With the whole beam every kept state's v is the best prefix value of its state, the
    rows are the states in (v descending, q ascending) order, and graph_scores is the enumeration's own sum."""
    rng = np.random.default_rng(600 + seed)
    T, N, S = 5, 4, 4
    nxt = rng.integers(0, S, size=(S, N))
    nxt[rng.random(size=(S, N)) < 0.2] = -1
    w = rng.normal(size=(S, N))
    f = rng.normal(size=S)
    f[rng.random(size=S) < 0.3] = -np.inf
    x = rng.normal(size=(T, 1, N))
    tr = rng.normal(size=(N, N))
    present, _, _ = fold(nxt, w, f, np.float64, 0.5, -0.3)
    label, state, _, _, Q = product(nxt, present)
    number = {(int(i), int(s)): q for q, (i, s) in enumerate(zip(label, state))}
    s = BeamStreamRef(tr, nxt, w, f, 0, 1, T, Q + 1, np.inf, 0.5, -0.3, np.float64)
    rows = 0
    for t in range(T):
        s.advance(x[t:t + 1])
        best = _enumerate_prefixes(x[:t + 1, 0], tr, nxt, w, 0, 0.5, -0.3)
        ranked = sorted(best.items(), key=lambda kv: (-kv[1][0], number[kv[0]]))
        nb = Q + 2
        sc, gs, tok, tl, nh, path, st, fr, su = stream_nbest(s, nb, False)
        assert nh[0] == len(ranked) == s.slots[0].aq.size and fr[0] == t + 1 and su[0] == 0
        rows += len(ranked)
        for r, (_, (v, labels, sts, g)) in enumerate(ranked):
            assert sc[0, r] == v and gs[0, r] == g
            assert path[0, r, :t + 1].tolist() == list(labels) and st[0, r, :t + 1].tolist() == sts
            assert (path[0, r, t + 1:] == -1).all() and (st[0, r, t + 1:] == -1).all()
            toks = [k for k, _ in itertools.groupby(labels)]
            assert tl[0, r] == len(toks) and tok[0, r, :len(toks)].tolist() == toks and (tok[0, r, len(toks):] == -1).all()
        pad = slice(int(nh[0]), nb)
        assert (sc[0, pad] == -np.inf).all() and (gs[0, pad] == -np.inf).all() and (tl[0, pad] == 0).all()
        assert (tok[0, pad] == -1).all() and (path[0, pad] == -1).all() and (st[0, pad] == -1).all()
    assert rows > T                                          # more than one row somewhere


def test_a_lexicon_with_a_narrow_beam_has_fewer_final_rows_than_prefixes():
    """Mid-word states have no final weight: they are prefixes, not hypotheses."""
    g = GRAPHS["lexicon"]()
    T, B, K = 10, 3, 6
    x, tr, il = _case(T, B, g.N, 61, np.float32)
    il[:] = T
    s = _stream(g, tr, B, T, K, np.inf, np.float32)
    fewer = 0
    for t in range(T):
        s.advance(x[t:t + 1])
        fin, pre = stream_nbest(s, K, True), stream_nbest(s, K, False)
        assert (fin[4] <= pre[4]).all() and (pre[4] == [v.aq.size for v in s.slots]).all()
        fewer += int((fin[4] < pre[4]).sum())
    assert fewer > 0


@pytest.mark.parametrize("final", [False, True])
def test_row_0_equals_result_and_the_state_is_left_alone(final):
    g = GRAPHS["trigram_holes"]()
    T, B = 12, 3
    x, tr, il = _case(T, B, g.N, 62, np.float32)
    il[:] = T
    s = _stream(g, tr, B, T, 4, 3.0, np.float32)
    for t in range(T):
        s.advance(x[t:t + 1])
        before = copy.deepcopy(s.slots)
        res = s.result(final)
        a = stream_nbest(s, 3, final)
        b = stream_nbest(s, 3, final)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
        sc, gs, tok, tl, nh, path, st, fr, su = a
        assert sc[:, 0].tobytes() == res[0].tobytes() and tl[:, 0].tobytes() == res[3].tobytes()
        assert np.array_equal(path[:, 0], res[1]) and np.array_equal(tok[:, 0], res[2]) and np.array_equal(st[:, 0], res[4])
        assert np.array_equal(fr, res[5]) and np.array_equal(su, res[6])
        for u, v in zip(before, s.slots):
            assert (u.pos, u.overflow, u.sizes) == (v.pos, v.overflow, v.sizes)
            assert np.array_equal(u.aq, v.aq) and np.array_equal(u.av, v.av) and len(u.history) == len(v.history)


def test_masked_reset_no_frames_an_empty_set_and_overflow():
    g = GRAPHS["bigram"]()
    T, B, M = 10, 3, 8
    x, tr, _ = _case(T, B, g.N, 63, np.float64)
    s = _stream(g, tr, B, M, 3, 4.0, np.float64)
    empty = stream_nbest(s, 2, True)                         # pos == 0
    assert not empty[4].any() and (empty[0] == -np.inf).all() and (empty[2] == -1).all() and not empty[7].any()
    s.advance(x[:5])
    s.reset(np.array([0, 1, 0]))
    got = stream_nbest(s, 2, False)
    assert got[7].tolist() == [5, 0, 5] and got[4][1] == 0 and (got[0][1] == -np.inf).all() and got[4][0] > 0
    s.advance(x[5:])                                         # 5 more frames: slots 0 and 2 reach max_frames = 8 and overflow
    got = stream_nbest(s, 2, True)
    assert got[7].tolist() == [M, 5, M] and got[8].tolist() == [1, 0, 1]
    one = beam_nbest_ref(x[:M], tr, g.next, g.weight, g.final, g.start, None, 3, 2, 4.0, LW, TS)
    assert got[0][0].tobytes() == one[0][0].tobytes() and np.array_equal(got[5][0], one[6][0])
    # a beam that empties: every emission of one frame at -inf
    y = x.copy()
    y[3] = -np.inf
    s = _stream(g, tr, B, T, 3, 4.0, np.float64)
    s.advance(y)
    got = stream_nbest(s, 2, False)
    assert got[7].tolist() == [T] * B and not got[4].any() and (got[0] == -np.inf).all() and (got[5] == -1).all()


# ---- the window
def _window(nxt, w, f, start, tr, B, W, P, K, theta, dtype, ts=TS):
    return BeamWindowRef(tr, nxt, w, f, start, B, W, P, K, theta, LW, ts, dtype)


def _commits_plus_tail(acc, new, got, ref, srows, b, what):
    """acc: per slot the committed (path, states, tokens) so far.  While bit 0 is clear, commits + tail of EVERY row of the
    window (got) equal the stream's row (srows); with it set the rows equal _walk of each candidate."""
    wsc, wtok, wtl, wnh, wpath, wst, wfr, wco, wsu = got
    ssc, _, stok, stl, snh, spath, sst = srows[:7]
    v = ref.slots[b]
    assert wsc[b].tobytes() == ssc[b].tobytes() and wnh[b] == snh[b], what
    assert wfr[b] == v.pos and wco[b] == v.base, what
    for r in range(int(wnh[b])):
        n = v.pos - v.base
        if not wsu[b] & 1:
            p = acc[b][0] + wpath[b, r, :n].tolist()
            q = acc[b][1] + wst[b, r, :n].tolist()
            k = acc[b][2] + wtok[b, r, :wtl[b, r]].tolist()
            assert p == spath[b, r, :v.pos].tolist() and q == sst[b, r, :v.pos].tolist(), what
            assert k == stok[b, r, :stl[b, r]].tolist(), what
        assert (wpath[b, r, n:] == -1).all() and (wst[b, r, n:] == -1).all() and (wtok[b, r, wtl[b, r]:] == -1).all(), what


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("WP", [(8, 2), (16, 4), (5, 5)])
def test_window_rows_are_the_commits_and_the_tail_of_every_row(WP, dtype):
    W, P = WP
    T, B, K, nb = 40, 3, 4, 6
    reached = {"clear": 0, "forced": 0, "empty_tail": 0, "rows": 0}
    cases = []
    g = GRAPHS["bigram"]()
    x, tr, _ = _case(T, B, g.N, 71, dtype)
    cases.append(("bigram", g.next, g.weight, g.final, g.start, x, tr, K, TS))
    nxt, w, f, start = chain_automaton(T + 2, 5)
    x, tr, _ = _case(T, B, 5, 72, dtype)
    cases.append(("chain", nxt, w, f, start, x, tr, 1, TS))                 # K = 1: every attempt commits up to pos - 1
    nxt, w, f = two_components_automaton(6)
    tr0 = np.zeros((6, 6), dtype)
    cases.append(("two", nxt, w, f, 0, two_component_emissions(T, B, 6, dtype), tr0, K, -1.0))
    rng = np.random.default_rng(9)
    for name, nxt, w, f, start, x, tr, k, ts in cases:
        cuts = [0] + np.sort(rng.integers(0, T + 1, size=9)).tolist() + [T]
        win = _window(nxt, w, f, start, tr, B, W, P, k, np.inf, dtype, ts)
        ref = BeamStreamRef(tr, nxt, w, f, start, B, T, k, np.inf, LW, ts, dtype)
        acc = [([], [], []) for _ in range(B)]
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            new = win.advance(x[t0:t1])
            ref.advance(x[t0:t1])
            for b in range(B):
                acc[b][0].extend(new[0][b, :new[3][b]].tolist())
                acc[b][1].extend(new[1][b, :new[3][b]].tolist())
                acc[b][2].extend(new[2][b, :new[4][b]].tolist())
            for final in (False, True):
                got = window_nbest(win, nb, final)
                srows = stream_nbest(ref, nb, final)
                assert got[0].tobytes() == srows[0].tobytes() and got[3].tobytes() == srows[4].tobytes()
                for b in range(B):
                    what = "%s W=%d P=%d t1=%d b=%d final=%d" % (name, W, P, t1, b, final)
                    _commits_plus_tail(acc, new, got, win, srows, b, what)
                    v = win.slots[b]
                    if got[3][b]:
                        reached["forced" if v.status & 1 else "clear"] += 1
                        reached["rows"] += int(got[3][b] > 1)
                        reached["empty_tail"] += int(v.base == v.pos)
                    if v.status & 1:                         # the rows are still exactly the specified chains
                        cand, _ = _candidates(win.s, v.aq, v.av, final)
                        for r in range(int(got[3][b])):
                            qs = win._walk(v, int(v.aq[cand[r]]), v.pos - 1, v.base)
                            assert got[4][b, r, :len(qs)].tolist() == win.s.label[qs].tolist(), what
                            assert got[5][b, r, :len(qs)].tolist() == win.s.state[qs].tolist(), what
        if name == "chain":
            assert reached["empty_tail"] > 0, "K = 1 on a chain commits everything: base == pos"
        if name == "two" and W - P < T:
            assert reached["forced"] > 0, "two components never converge: the commit is forced"
    assert reached["clear"] > 0 and reached["rows"] > 0


def test_both_window_regimes_are_reached_somewhere():
    """(8, 2) with the two components: bit 0 set; the chain with K = 1: base == pos."""
    nxt, w, f = two_components_automaton(6)
    x = two_component_emissions(40, 2, 6, np.float32)
    win = _window(nxt, w, f, 0, np.zeros((6, 6), np.float32), 2, 8, 2, 4, np.inf, np.float32, -1.0)
    win.advance(x)
    got = window_nbest(win, 4, False)
    assert (got[8] & 1).all() and (got[3] >= 2).all()
    nxt, w, f, start = chain_automaton(30, 5)
    x, tr, _ = _case(20, 2, 5, 73, np.float32)
    win = _window(nxt, w, f, start, tr, 2, 8, 2, 1, np.inf, np.float32)
    win.advance(x)
    got = window_nbest(win, 3, False)
    assert (got[6] == got[7]).all() and (got[3] == 1).all() and (got[2] == 0).all() and (got[0][:, 0] > -np.inf).all()
    assert (got[4] == -1).all() and not got[8].any()
