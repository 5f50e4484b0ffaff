"""CPU tests of the inputs of tests/test_hip_beam_select_regimes.py (tests/beam_select_cases.py): from the numpy restatements
and the restated launch arithmetic ALONE, every case is in the regime it names -- the width `rem` of the key select and the
exit it takes, the digit of the tie select over q in which a cut falls, the full beams against the lanes per state, the side of
the LDS bound -- and every select case can tell a subtly wrong select from a right one: the restatement run with a wrong select
(tests/beam_decode_ref.py::WRONG: the narrow last digit of the keys ignored, the whole last digit ignored, the keys compared as
raw sign-magnitude bits, the second or the last digit of q cleared, the tied taken from the top) gives other outputs.  A case
whose wrong variant gave the same outputs would not be in its regime."""
import numpy as np
import pytest

import beam_select_cases as C
from beam_decode_ref import EXITS, WRONG, beam_decode_ref, digit_shifts, key_enc, q_bits, select_info
from beam_word_ref import beam_word_ref
from graph_decode_ref import fold, product

INF = float("inf")
ALL_KEY_CASES = [(n, dt) for dt in (np.float32, np.float64) for n in C.key_frame_names(dt)]
KEY_IDS = ["%s-%s" % (n, "f32" if dt == np.float32 else "f64") for n, dt in ALL_KEY_CASES]


def ref(graph, x, tr, il, K, theta, **kw):
    return beam_decode_ref(x, tr, graph.next, graph.weight, graph.final, graph.start, il, K, theta, **kw)


def _same(a, b):
    return all(u.dtype == v.dtype and u.tobytes() == v.tobytes() for u, v in zip(a, b))


def under_test(info):
    """The records of the frame under test of a key case: behind another frame, as the first frame, behind a second one."""
    return [info["frames"][0][1], info["frames"][1][0], info["frames"][2][1]]


def key_runs(name, dtype):
    """The (threshold, beam) pairs of a key case: every threshold with beams below, at and above the count that passes it,
    which the restatement itself reports."""
    x, tr, il, _ = C.key_case(name, dtype)
    out = []
    for theta in C.key_thresholds(name, dtype):
        info = {}
        ref(C.one_state(), x, tr, il, C.K_KEY, theta, info=info)
        out += [(theta, K) for K in C.key_beams(under_test(info)[0]["passing"])]
    return out


def assert_key_regime(name, dtype, theta, K, info):
    """One run of a key case is where the case says: -> the record of the frame under test."""
    _, exit_, _, how = C.KEY_FRAMES[name]
    recs = under_test(info)
    assert all(r == recs[0] for r in recs), "the frame under test selects alike wherever it stands"
    r = recs[0]
    assert r["n"] == (how[1] if how[0] == "equal" else C.N_KEY - 1)
    if theta == INF:
        assert r["rem"] == C.key_rem(name, dtype) and r["passing"] == r["n"]
    elif theta == 0:
        assert r["rem"] == 0 and r["passing"] == (10 if how[0] == "equal" else 1)
    elif how[0] != "equal":
        assert K_BAND[0] < r["passing"] < K_BAND[1], "the finite threshold cuts inside the band"
    if K >= r["passing"]:
        assert r["exit"] == ("equal-fit" if r["rem"] == 0 else "whole")
    elif theta != 0:
        assert K == C.K_KEY and r["exit"] == exit_
    else:
        assert r["exit"] == "equal-cut"
    return r


K_BAND = (C.K_KEY, 100)


# ---------------------------------------------------------------------------------------------------------------- arithmetic
def test_the_restated_keys_and_launch_arithmetic():
    for dt in (np.float32, np.float64):
        v = np.array([-np.inf, -3.5, -1.0, -1e-30, -0.0, 0.0, 1e-30, 1.0, 1.0 + C.ULP[dt], 3.5, np.inf], dt)
        k = key_enc(v)
        assert k.dtype == (np.uint32 if dt == np.float32 else np.uint64) and k[4] == k[5]          # -0 and +0 are one key
        assert (np.diff(k[:5].astype(object)) > 0).all() and (np.diff(k[5:].astype(object)) > 0).all() and k.min() > 0
        V = C.base_value(dt)
        for kk in (1, 2, 255, 256, 2 ** 17 - 1, 2 ** C.ONES[dt] - 1):                              # enc(V) ^ enc(V - k ulp) = k
            assert int(key_enc(V)) ^ int(key_enc(dt(V - dt(kk * C.ULP[dt])))) == kk
    assert digit_shifts(3) == [(0, 3)] and digit_shifts(9) == [(1, 8), (0, 1)] and digit_shifts(17) == [(9, 8), (1, 8), (0, 1)]
    assert digit_shifts(18) == [(10, 8), (2, 8), (0, 2)]
    assert digit_shifts(64)[-1] == (0, 8) and len(digit_shifts(40)) == 5 and digit_shifts(20)[-1] == (0, 4)
    assert [q_bits(Q) for Q in (1, 2, 200, 256, 257, 65536, 65537)] == [1, 1, 8, 8, 9, 16, 17]
    assert [C.beam_lanes_per_state(K) for K in C.LANE_BEAMS] == [64, 64, 64, 32, 32, 16, 16, 8, 8, 4, 4, 2, 2, 1]
    # launch_beam_graph: 4096 + K (e + 4) + 8 + N N e against 160 KiB
    assert C.graph_lds(8, 141, 8) <= C.LDS_MAX < C.graph_lds(8, 142, 8)
    assert C.LDS_STEPS == [(4, 8192, 153), (8, 8192, 87)]
    for elem, K, N in C.LDS_STEPS:
        assert C.transitions_in_lds(K, N, elem) and not C.transitions_in_lds(K, N + 1, elem)
        assert C.graph_lds(K, N, elem) - N * N * elem == 4096 + 8192 * (elem + 4) + 8 > 64 * 1024
        print("elem %d K %d: N = %d takes %d bytes of LDS, N = %d would take %d" % (elem, K, N, C.graph_lds(K, N, elem), N + 1,
                                                                                   C.graph_lds(K, N + 1, elem)))


def test_the_record_of_the_select_on_small_frames():
    q = np.arange(6)
    c = np.array([3.0, 1.0, 3.0, 2.0, 2.0, -5.0], np.float32)
    assert select_info(q[:0], c[:0], 2, np.float32(INF)) == dict(n=0, passing=0, rem=0, exit="nothing")
    assert select_info(q, c, 2, np.float32(0))["exit"] == "equal-fit" and select_info(q, c, 1, np.float32(0))["cut"] == (0, 2)
    assert select_info(q, c, 5, np.float32(2))["exit"] == "whole" and select_info(q, c, 5, np.float32(2))["passing"] == 5
    r = select_info(q, c, 3, np.float32(INF))
    assert (r["exit"], r["need"], r["tied"], r["cut"], r["rem"]) == ("tie-select", 1, 2, (3, 4), 32)
    assert select_info(q, c, 4, np.float32(INF))["exit"] == "kth-ties-taken"
    assert EXITS == ("nothing", "equal-fit", "equal-cut", "whole", "kth-ties-taken", "tie-select")


# ---------------------------------------------------------------------------------------------------------------- key widths
@pytest.mark.parametrize("name,dtype", ALL_KEY_CASES, ids=KEY_IDS)
def test_key_width_regimes_and_their_bite(name, dtype):
    x, tr, il, _ = C.key_case(name, dtype)
    graph = C.one_state()
    assert not tr[:C.WITNESS].any() and sorted(tr[C.WITNESS, :C.WITNESS]) == list(range(0, 4 * C.WITNESS, 4))
    runs = key_runs(name, dtype)
    assert (INF, C.K_KEY) in runs and len({t for t, _ in runs}) == 3 and len(runs) >= 8
    bites = {w: 0 for w in WRONG}
    seen = []
    for theta, K in runs:
        info = {}
        want = ref(graph, x, tr, il, K, theta, info=info)
        r = assert_key_regime(name, dtype, theta, K, info)
        seen.append((theta if theta in (INF, 0) else "finite", K, r["rem"], r["exit"]))
        assert info["Q"] == C.N_KEY and np.isfinite(want[0]).all() and (want[1][0, 2] == C.WITNESS)
        for w in WRONG:
            changed = not _same(want, ref(graph, x, tr, il, K, theta, wrong=w))
            bites[w] += changed
            if (theta, K, w) == (INF, C.K_KEY, C.KEY_FRAMES[name][2]):
                assert changed, "the wrong select `%s` gives the same five outputs: the case is not in its regime" % w
    print("%s %s: (threshold, K, rem, exit) %s; runs of %d whose outputs a wrong select changes: %s"
          % (name, dtype.__name__, seen, len(runs), bites))
    assert sum(bites.values()) > 0


def test_the_key_cases_reach_every_width_and_every_exit():
    for dtype in (np.float32, np.float64):
        bits = 8 * np.dtype(dtype).itemsize
        rems, exits = set(), set()
        for name in C.key_frame_names(dtype):
            x, tr, il, _ = C.key_case(name, dtype)
            for theta, K in key_runs(name, dtype):
                info = {}
                ref(C.one_state(), x, tr, il, K, theta, info=info)
                r = under_test(info)[0]
                rems.add(r["rem"]), exits.add(r["exit"])
                if r["exit"] == "whole" and r["rem"] > 8:
                    exits.add("whole, rem > 8")
        assert {0, 3, 8, 9, 16, 17, 20, bits} <= rems and any(1 <= r <= 7 for r in rems) and any(18 <= r <= 23 for r in rems)
        assert dtype == np.float32 or any(33 <= r <= 50 for r in rems)
        assert exits == set(EXITS[1:]) | {"whole, rem > 8"}      # ("nothing": tests/test_hip_beam_stream.py, the emptied beam)
        print("%s: rem %s, exits %s" % (dtype.__name__, sorted(rems), sorted(exits)))


@pytest.mark.parametrize("name,dtype", ALL_KEY_CASES, ids=KEY_IDS)
def test_the_word_copy_of_the_select_sees_the_same_frames(name, dtype):
    """With one-token words and lm_weight = word_score = 0 the frame behind a separator has the one-state automaton's
    candidates: the word restatement's own record shows the same rem, exit and counts."""
    lex, lm = C.word_case()
    x, tr, il, _ = C.word_key_case(name, dtype)
    xg, trg, ilg, _ = C.key_case(name, dtype)
    for theta, K in key_runs(name, dtype):
        info, winfo = {}, {}
        ref(C.one_state(), xg, trg, ilg, K, theta, info=info)
        want = beam_word_ref(x, tr, lex, lm, il, K, theta, 0.0, 0.0, 0.0, info=winfo)
        r = under_test(info)[0]
        for rec in (winfo["select"][0][2], winfo["select"][1][0]):
            assert {k: rec[k] for k in ("n", "passing", "rem", "exit")} == {k: r[k] for k in ("n", "passing", "rem", "exit")}
            assert "cut" not in r or (rec["need"], rec["tied"]) == (r["need"], r["tied"])
        assert np.isfinite(want["scores"]).all() and winfo["pbits"] == q_bits(winfo["Q"]) + 1


# -------------------------------------------------------------------------------------------------------------- state widths
def width_regime(info, K):
    """What one run's `info` shows of a width's regime -> counts: cuts by the digit that decides them, cuts in a frame of more
    than 1024 candidates, cuts at a beam above 1024."""
    out = {}
    for frames in info["frames"]:
        for r in frames:
            if "cut" in r:
                d = "digit %d" % C.deciding_digit(*r["cut"], info["Q"])
                out[d] = out.get(d, 0) + 1
                out["n > 1024"] = out.get("n > 1024", 0) + (r["n"] > 1024)
                out["K > 1024"] = out.get("K > 1024", 0) + (K > 1024)
    return out


def assert_width_regime(bits, total):
    digits = len(digit_shifts(bits))
    for d in range(digits):
        assert total.get("digit %d" % d, 0) > 0, "no cut decided in digit %d of %d" % (d, digits)
    if bits >= 16:
        assert total["n > 1024"] > 0 and total["K > 1024"] > 0


# the wrong selects that have to change the outputs of some run of a width
WIDTH_BITES = {8: ("ties_from_top",), 9: ("q_last_digit",), 16: ("q_second_digit",), 17: ("q_second_digit", "q_last_digit"),
               18: ("q_second_digit", "q_last_digit")}


@pytest.mark.parametrize("bits", sorted(C.WIDTHS))
def test_state_width_regimes_and_their_bite(bits):
    graph = C.width_graph(bits)
    x, tr, il = C.width_inputs(bits, np.float32)
    assert not tr.any() and not np.asarray(graph.weight).any() and set(np.unique(x)) == {-1, 0, 1}
    total, bites = {}, {w: 0 for w in WIDTH_BITES[bits]}
    for K in C.width_beams(bits):
        for theta in C.WIDTH_THETAS:
            info = {}
            want = ref(graph, x, tr, il, K, theta, info=info)
            assert q_bits(info["Q"]) == bits
            for k, v in width_regime(info, K).items():
                total[k] = total.get(k, 0) + v
            for w in bites if theta == INF else ():
                bites[w] += not _same(want, ref(graph, x, tr, il, K, theta, wrong=w))
    print("q of %d bits: Q %d, digits %s; cuts %s; runs whose outputs a wrong select changes: %s"
          % (bits, info["Q"], digit_shifts(bits), total, bites))
    assert_width_regime(bits, total)
    assert all(v > 0 for v in bites.values()), "a wrong select gives the same five outputs: the case is not in its regime"


# --------------------------------------------------------------------------------------------------------------------- lanes
def lanes_regime(K, sizes):
    """-> (G, the rows' length): a frame with a successor keeps exactly K states, each with a row of 69 arcs."""
    graph = C.lane_graph()
    present, _, _ = fold(graph.next, graph.weight, graph.final, np.float32, 1.0, 0.0)
    label, state, src, _, Q = product(np.asarray(graph.next), present)
    rows = np.bincount(src, minlength=Q)
    assert rows.min() == rows.max() == C.LANE_N - 1 and Q > max(C.LANE_BEAMS)
    assert any(K in s[:-1] for s in sizes), "no frame with a successor keeps exactly K states"
    return C.beam_lanes_per_state(K), int(rows.max())


@pytest.mark.parametrize("K", C.LANE_BEAMS)
def test_lanes_per_state_regimes(K):
    x, tr, il = C.lane_inputs()
    sizes = []
    ref(C.lane_graph(), x, tr, il, K, INF, sizes=sizes)
    G, row = lanes_regime(K, sizes)
    print("K %d: G %d, rows of %d arcs" % (K, G, row))
    assert row == 69 > 64 >= G


# ----------------------------------------------------------------------------------------------------------------------- LDS
@pytest.mark.parametrize("elem,K,N0", C.LDS_STEPS, ids=["f32", "f64"])
def test_both_sides_of_the_lds_step_at_the_largest_beam(elem, K, N0):
    dt = np.float32 if elem == 4 else np.float64
    for N in (N0, N0 + 1):
        graph = C.lds_graph(N)
        assert C.transitions_in_lds(K, N, elem) == (N == N0)
        present, _, _ = fold(graph.next, graph.weight, graph.final, dt, 1.0, 0.0)
        Q = product(np.asarray(graph.next), present)[4]
        assert Q > K == C.MAX_K, "the beam would be clamped to Q"
    sizes = []
    x, tr, il = C.lds_inputs(N0, dt)
    want = ref(C.lds_graph(N0), x, tr, il, K, INF, sizes=sizes)
    assert sizes[0][-1] == K and np.isfinite(want[0]).all()      # the last frame fills the beam
