"""CPU half of tests/test_hip_fused_regimes.py: the case list of tests/fused_regime_cases.py is checked against the
source text of the fused step and against the fp64 oracle alone -- the constants the cases rest on are still the kernel's, the list
reaches every regime it names, and the reference by itself says which utterances have a reason to be flagged."""
import os
import re

import numpy as np
import pytest

import fused_regime_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    with open(os.path.join(ROOT, "torch_asg_amd", "csrc", name)) as f:
        return f.read()


def test_constants_are_the_kernels():
    """A change to any of these sends its author back to the case list."""
    fused, chains, api = _src("asg_fused.hip"), _src("asg_chains.h"), _src("asg_api.hip")
    for name, v in (("kMinFused", fc.K_MIN_FUSED), ("kGS", fc.K_GS), ("kFR", fc.K_FR), ("kAR", fc.K_AR), ("kMaxBlk", fc.K_MAX_BLK),
                    ("kCH", fc.K_CH), ("kQB", fc.K_QB), ("kBwdSlice", fc.K_BWD_SLICE)):
        m = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, fused)
        assert m == [str(v)], (name, m, v)
    for name, v in (("kPF", fc.K_PF), ("kRenorm", fc.K_RENORM)):
        assert re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, chains) == [str(v)], name
    edges = re.findall(r"if \(N <= (\d+)\) return launch_fused_np<(\d+)>\(", fused)
    assert edges == [(str(e), str(e)) for e in fc.NP_EDGES], edges
    assert len(re.findall(r"return launch_fused_np<64>\(P, W, F, backward, stream\);", fused)) == 1
    assert len(edges) + 1 == 8
    assert re.search(r"if \(p->T > %d\) return 0;" % fc.T_MAX, api)
    assert re.search(r"static constexpr int fit = NP <= 48 \? 4 : 2;\s*static constexpr int n = 3 < fit \? 3 : fit;", fused)
    assert re.search(r"xstate_blocks\(int T\) \{ return \(T \+ 7\) / 8 \+ 2; \}", fused)
    assert re.search(r"q0 \+= 4 \* kCH \* kQB\)", fused) and fc.ROW_PASS_STRIDE == 128
    assert re.search(r"\(T \+ kPF - 1\) / kPF \+ 1", fused)
    assert "dim3(48 * ((P.B + 15) / 16))" in fused
    assert re.search(r"lo = \(127u - %du\) << 23, hi = \(127u \+ %du\) << 23" % (fc.RANGE_BITS, fc.RANGE_BITS), chains)


def test_crossing_restatement():
    """crossing(len) of the source, transcribed line by line: below 64 frames len / 2; from 64 on within base + 1 .. base + 5 and
    both second halves end on a group of at most five frames (what the search is for)."""
    fused = _src("asg_fused.hip")
    assert re.search(r"if \(len < 64\) return mid;\s*const int base = \(mid >> 3\) << 3;\s*int best = mid, cost = 99;\s*"
                     r"for \(int r = 1; r <= 5; \+\+r\) \{\s*const int m = base \+ r, ra = \(len - m\) & 7, c = max\(r, ra == 0 \? 8 : ra\);"
                     r"\s*if \(c < cost\) \{ cost = c; best = m; \}", fused)
    for n in range(1, 64):
        assert fc.crossing(n) == n // 2
    for n in range(64, fc.T_MAX + 1):
        mid = fc.crossing(n)
        a, b = fc.cross_class(n)
        assert 1 <= a <= 5 and 1 <= b <= 5 and abs(mid - n // 2) <= 7, (n, mid)


def test_case_list_reaches_every_regime():
    sweep = [n for k in range(fc.SWEEP_BATCHES) for n in fc.sweep_case(5, k).il.tolist()]
    assert sweep == list(range(1, 337))
    # all eight (mid % 8, (len - mid) % 8) classes of the searched crossing, and both sides of len 64
    classes = {fc.cross_class(n) for n in range(64, fc.T_MAX + 1)}
    assert len(classes) == 8, classes
    assert {fc.cross_class(n) for n in sweep if n >= 64} == classes
    assert 63 in sweep and 64 in sweep
    # second halves on both sides of one and of two turns of the rings (kFR = kAR = 64 frames)
    halves = {h for n in sweep for h in (fc.crossing(n), n - fc.crossing(n))}
    # (the searched crossing leaves both halves 1 .. 5 frames past a multiple of 8: the nearest lengths on either side)
    for edge in (fc.K_FR, 2 * fc.K_FR):
        assert {edge - 3, edge + 1} <= halves and not {edge - 1, edge} & {h for h in halves if h > 32}, edge
    # first and last lengths that are fused, every group remainder
    assert {1, 2, 3, 4} <= set(sweep) and {h % fc.K_GS for h in halves} == set(range(8))
    # the row pass's second outer iteration
    nq = [fc.row_quads(n) for n in fc.rowpass_case().il.tolist()]
    assert min(nq) < fc.ROW_PASS_STRIDE and fc.ROW_PASS_STRIDE in nq and fc.ROW_PASS_STRIDE + 1 in nq, nq
    assert max(fc.row_quads(n) for n in sweep) < fc.ROW_PASS_STRIDE
    # every NP, both consumer counts, at lengths with and without a ring wrap
    assert {fc.np_of(N) for N in fc.NP_ALPHABETS} == set(fc.NP_EDGES) | {64}
    assert {fc.consumers(fc.np_of(N)) for N in fc.NP_ALPHABETS} == {2, 3}
    assert [fc.consumers(fc.np_of(N)) for N in fc.SWEEP_N] == [3, 3, 2] and fc.np_of(40) == 40
    c = fc.np_case(9)
    h = [n - fc.crossing(n) for n in c.il.tolist()]
    assert min(h) < fc.K_FR < max(h) and c.B == 32
    # T padding: every T % 16 (aoff, blocks of 16), hence every T % 8 (xstate, P2); the utterances do not change
    assert {T % 16 for T in fc.PAD_T} == set(range(16)) and len(fc.PAD_T) == 17
    assert {fc.xstate_blocks(T) for T in fc.PAD_T} == {19, 20, 21} and {fc.aoff_entries(T) for T in fc.PAD_T} == {10, 11}
    assert fc.pad_case(130).il.tolist() == list(fc.PAD_LENGTHS) and fc.pad_case(146).tl.tolist() == list(fc.PAD_TARGETS)
    for T in fc.PAD_T[1:]:
        a, b = fc.pad_case(130), fc.pad_case(T)
        for i, n in enumerate(fc.PAD_LENGTHS):
            assert np.array_equal(a.x[:n, i].numpy(), b.x[:n, i].numpy()) and np.array_equal(a.tg[i].numpy(), b.tg[i].numpy())
    # batch: both sides of every grid step (48 blocks per 16 utterances), of an XCD pair, and of the fused edge
    assert fc.BATCH_SIZES == (1, 2, 15, 16, 17, 32, 33, 79, 80)
    assert [fc.grid_blocks(B) for B in (15, 16, 17, 32, 33, 80)] == [48, 48, 96, 96, 144, 240]
    assert fc.fused_edge(256) == 80 and fc.fused_preferred(80, 256) and not fc.fused_preferred(81, 256)
    # top of the range
    assert fc.top_case(4000).T == fc.T_MAX and fc.top_case(4000).fused and not fc.top_case(4001).fused
    assert (max(fc.crossing(fc.T_MAX), fc.T_MAX - fc.crossing(fc.T_MAX)) + 15) // 16 <= fc.K_MAX_BLK - 1
    # targets
    assert [fc.target_case(k).S for k in ("S1", "S2", "S63", "S64")] == [1, 2, 63, 64]
    for k in ("S2", "S63", "S64"):
        tl = fc.target_case(k).tl.tolist()
        assert min(tl) == 1 and max(tl) == fc.target_case(k).S
    c = fc.target_case("tight")
    assert c.tl.tolist() == c.il.tolist()
    c = fc.target_case("one-label")
    assert all(len(set(row.tolist())) == 1 for row in c.tg) and 64 in c.tl.tolist()
    c = fc.target_case("padded-with-a-used-label")
    assert all(int(c.tg[b, -1]) in c.tg[b, :int(c.tl[b])].tolist() for b in range(c.B))
    # mixed batch
    c = fc.mixed_case()
    assert c.flagged.tolist() == [False, True, False, True, True, False, False, False, False, False, True]
    assert c.feasible.tolist() == [b != 6 for b in range(c.B)]
    assert float(c.w[3]) == 1.0 and abs(float(c.w[4]) - 0.37) < 1e-7 and c.flagged[3] and c.flagged[4]
    assert [int(c.il[b]) for b in fc.MIXED_ORDINARY] == [fc.PAD_LENGTHS[i] for i in fc.MIXED_PAD]
    # weights of the sweep: exactly 1.0 and exactly 0.0 at rotating places
    for k in range(fc.SWEEP_BATCHES):
        w = fc.sweep_case(5, k).w
        assert float(w[k % 16]) == 1.0 and float(w[(k + 5) % 16]) == 0.0


_CASES = fc.all_cases()


@pytest.mark.parametrize("case", _CASES, ids=[c.name for c in _CASES])
def test_oracle_says_what_the_case_says(case):
    """Finite losses exactly where the case says "feasible", +inf exactly where it says "infeasible"; and every utterance the case
    expects NOT to be flagged keeps its row sums inside [2^-100, 2^100] by a wide margin: at most half of the 100 bits by the bound of
    fused_regime_cases.range_bits (2^50 to spare on either side), so the reference alone shows that it has no reason to be
    flagged; the utterance that is there to leave the window does leave it."""
    o = fc.reference(case)
    per = o["loss_per_utt"]
    assert np.array_equal(np.isfinite(per), case.feasible), (per, case.feasible)
    assert np.all(per[~case.feasible] == np.inf)
    assert np.isfinite(o["grad_inputs"]).all() and np.isfinite(o["grad_transition"]).all()
    for b in range(case.B):
        assert not o["grad_inputs"][int(case.il[b]):, b].any()
    bits = fc.range_bits(case)
    print("%s: range bound %.1f bits at most (utterance %d)" % (case.name, bits.max(), int(bits.argmax())))
    calm = ~case.flagged
    assert (bits[calm] <= 0.5 * fc.RANGE_BITS).all(), (case.name, bits)
    assert (bits[case.wide] > fc.RANGE_BITS).all(), (case.name, bits)
    short = case.il.numpy() < fc.K_MIN_FUSED
    assert np.array_equal(case.flagged, short | case.wide)
