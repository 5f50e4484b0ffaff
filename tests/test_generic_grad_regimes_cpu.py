"""CPU half of tests/test_hip_generic_grad_regimes.py: the case list of tests/generic_grad_cases.py against the
source text of csrc/asg_generic_grad.hip and against the fp64 oracle alone -- the restated launch rules are still the library's,
every case is in the regime it names, the cells the training call leaves to the old rule stay under 1 %, and three numpy
mutations of the oracle's own tensors show that the own-scale rule sees what the parity rule does not."""
import os
import re

import numpy as np
import pytest

import generic_grad_cases as gc
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    with open(os.path.join(ROOT, "torch_asg_amd", "csrc", name)) as f:
        return f.read()


def test_constants_are_the_kernels():
    """A change to any of these sends its author back to the case list."""
    s = _src("asg_generic_grad.hip")
    assert re.findall(r"#define ASG_X_GEMM_BK (\d+)", s) == [str(gc.GEMM_BK)]
    assert re.findall(r"constexpr int kG3TM = (\d+), kG3TN = (\d+);", s) == [(str(gc.G3_TM), str(gc.G3_TN))]
    assert re.findall(r"constexpr int kG3TailSlices = (\d+), kG3WholeSlices = (\d+);", s) == [(str(gc.G3_TAIL_SLICES), str(gc.G3_WHOLE_SLICES))]
    assert re.findall(r"constexpr size_t kG3TailBytes = \(size_t\) (\d+) << 20;", s) == [str(gc.G3_TAIL_BYTES >> 20)]
    assert re.findall(r"#define ASG_X_G3_MIN_N (\d+)", s) == [str(gc.G3_MIN_N)]
    assert "constexpr int kG3MinN = ASG_X_G3_MIN_N;" in s and "N > kG3MinN)) return 0;" in s
    # gemm_slices, line by line
    assert re.search(r"const int tiles = \(\(N \+ 127\) / 128\) \* \(\(N \+ 127\) / 128\);\s*if \(tiles >= %d\) return 1;" % gc.SLICE_TILES, s)
    assert "int n = (%d + tiles - 1) / tiles;" % gc.SLICE_TILES in s
    assert "if (n > K / %d) n = K / %d;" % (gc.SLICE_MIN_ROWS, gc.SLICE_MIN_ROWS) in s
    # both roundings of a slice's length, and the fp64 contraction's own BK
    assert "const int kslice = ((K + nsl - 1) / nsl + ASG_X_GEMM_BK - 1) / ASG_X_GEMM_BK * ASG_X_GEMM_BK;" in s
    assert "const int kslice = ((K + nsl - 1) / nsl + %d) / %d * %d;" % (gc.F64_BK - 1, gc.F64_BK, gc.F64_BK) in s
    assert re.search(r"bwd_gemm_kernel\(.*?\{\s*constexpr int BK = %d;" % gc.F64_BK, s, re.S)
    # the bf16x3 launch plan
    assert "return (N + kG3TM - 1) / kG3TM * kG3TM; }" in s
    assert "const int Mt = npadT / kG3TM, Nt = (P.N + kG3TN - 1) / kG3TN;" in s
    assert "const int blocks = ((Mt + 3) / 4) * ((Nt + 7) / 8);" in s
    assert "int tail = blocks % 8, tks = 1;" in s and "if (blocks <= 8) {" in s
    assert "double best = (double) ((real + 255) / 256);" in s and "for (int t = 2; t <= kG3WholeSlices; ++t) {" in s
    assert "const double c = (double) ((real * t + 255) / 256) / t;" in s
    assert "if (c < best - 0.05 && (size_t) tail * 32 * t * kG3TM * kG3TN * sizeof(float) <= kG3TailBytes) { best = c; tks = t; }" in s
    assert "} else if (tail * 32 * 2 <= 256 && tail > 0) {" in s
    assert "tks = 256 / (tail * 32) > kG3TailSlices ? kG3TailSlices : 256 / (tail * 32);" in s
    assert "if (tks < 2 || (size_t) tail * 32 * tks * kG3TM * kG3TN * sizeof(float) > kG3TailBytes) { tail = 0; tks = 1; }" in s
    assert "const int mainb = blocks - tail;" in s
    assert "dim3(8 * 32 * ((mainb + 7) / 8))" in s
    # which precision compacts its rows, and the count of the valid ones
    assert "int v = len > 1 ? len - 1 : 0;" in s and "if (lane == 0) rowoff[B] = base;" in s
    assert "template <> struct StepUsesMfma<float> { static constexpr bool v = true; };" in _src("asg_generic_common.h")
    assert "if (nsl > 1 && !pbytes3) {" in s
    # the packed planes: blocks of 32 rows, stages of 16
    assert "if (8 * kg >= (K + 31) / 32 * 32) return;" in s and "const int nall = (K + 31) / 32 * 2;" in s


def test_restated_plan_at_the_alphabets_of_the_cases():
    plan = {N: gc.g3_plan(N) for N in (1025, 1281, 2048, 2049, 2816, 2817, 3584, 4096, 4097, 4100, 5121, 6145, 10000)}
    assert [(plan[N]["Nt"], plan[N]["blocks"]) for N in (2048, 2049)] == [(8, 2), (9, 6)]
    assert [plan[N]["tks"] for N in (2816, 2817)] == [2, 3] and plan[2817]["Mt"] * plan[2817]["Nt"] == 144
    for N in (1025, 1281, 2048, 2049, 2816, 2817):
        p = plan[N]
        assert p["blocks"] <= 8 and 2 <= p["tks"] <= 8 and p["mainb"] == 0 and p["tail"] == p["blocks"], (N, p)
        assert p["tail"] * 32 * p["tks"] * 256 * 256 * 4 <= gc.G3_TAIL_BYTES
    for N in (3584, 4096):
        assert plan[N]["blocks"] == 8 and plan[N]["tks"] == 1 and plan[N]["tail"] == 0 and plan[N]["mainb"] == 8, plan[N]
    # 15 blocks: two rounds of 8 in ONE launch, the 16th block's workgroups find g >= mblocks * nblocks and return
    for N in (4097, 4100):
        assert plan[N] == dict(Mt=17, Nt=17, blocks=15, tail=0, tks=1, mainb=15), plan[N]
    assert plan[5121] == dict(Mt=21, Nt=21, blocks=18, tail=2, tks=4, mainb=16)
    assert plan[6145] == dict(Mt=25, Nt=25, blocks=28, tail=4, tks=2, mainb=24)
    assert plan[10000]["blocks"] == 50 and plan[10000]["tail"] == 2 and plan[10000]["tks"] == 4          # cfg 5: 6 rounds + 2 blocks
    # gemm_slices and the roundings
    assert [gc.gemm_slices(65, K) for K in (511, 512, 767, 768)] == [1, 2, 2, 3]
    assert gc.kslice(520, 2) == 288 and gc.kslice(520, 2, True) == 272 and gc.kslice(512, 2) == 256 and gc.kslice(768, 3) == 256
    assert gc.gemm_slices(1024, 512) == 2 and gc.gemm_slices(1024, 20) == 1
    assert gc.gemm_slices(2816, 512) == 2 and gc.gemm_slices(2817, 512) == 1 and gc.gemm_slices(2817, 1 << 20) == 1
    assert gc.valid_rows([0, 1, 2, 9, 12], 9) == 0 + 0 + 1 + 8 + 8


_CASES = gc.all_cases()
_BY_NAME = {c.name: c for c in _CASES}


def test_case_names_are_unique():
    assert len(_BY_NAME) == len(_CASES)


def test_every_case_is_in_its_regime():
    for c in _CASES:
        name, d = c.route()
        if c.regime not in (None, "frames"):
            assert name == c.regime, (c.name, name, d)
        # from 2049 labels on the cases stay small unless they are about the batch
        if c.N >= 2049 and c.B <= 3:
            assert c.T <= 5 and c.T * c.B <= 12, c.name
        assert c.T <= gc.DEEP_T and (c.regime is not None or c.T <= 8)
    route = lambda n: _BY_NAME[n].route()
    assert route("mfma-whole-BT511-N65")[1]["nsl"] == 1 and _BY_NAME["mfma-whole-BT511-N65"].B * 7 == 511
    assert route("mfma-sliced-BT512-N65")[1] == dict(nsl=2, kslice=256)
    assert route("mfma-2-slices-BT767-N129")[1]["nsl"] == 2 and route("mfma-3-slices-BT768-N129")[1] == dict(nsl=3, kslice=256)
    # B T = 520: slices of 288 rows, and the valid rows reach into the second one without filling it
    c = _BY_NAME["mfma-sliced-BT520-N257"]
    assert c.route()[1] == dict(nsl=2, kslice=288) and 288 < c.Kp < 2 * 288
    c = _BY_NAME["mfma-sliced-rows-in-first-slice-N130"]
    assert c.route()[1] == dict(nsl=2, kslice=256) and 0 < c.Kp <= 256
    c = _BY_NAME["mfma-sliced-one-row-in-second-slice-N131"]
    assert c.route()[1] == dict(nsl=2, kslice=256) and c.Kp == 257
    c = _BY_NAME["mfma-sliced-N1024"]
    assert c.route()[1] == dict(nsl=2, kslice=256) and 0 < c.Kp < 32
    # fp64: rows in place (row b T + t) -- live rows on both sides of the slice boundary, padding rows between them
    for n, ks in (("f64-sliced-BT512-N128", 256), ("f64-sliced-BT520-N128", 272), ("f64-sliced-BT512-N1100", 256),
                  ("f64-sliced-BT520-N1100", 272)):
        c = _BY_NAME[n]
        assert c.route()[1] == dict(nsl=2, kslice=ks), (n, c.route())
        rows = [b * c.T + t for b in range(c.B) for t in range(1, int(c.il[b]))]
        assert min(rows) < ks <= max(rows) and len(rows) == c.Kp
        assert any(int(c.il[b]) < c.T for b in range(c.B))
    assert _BY_NAME["f64-whole-BT511-N128"].route()[1]["nsl"] == 1 and _BY_NAME["step-f64-N2100"].route()[0] == "f64-whole"
    # the same inputs on either side of 1024 | 1025 labels would need the same N: the same seed, shape and lengths instead
    a, b = _BY_NAME["mfma-whole-N1024"], _BY_NAME["bf3-N1025"]
    assert (a.T, a.B, a.L) == (b.T, b.B, b.L) and a.il.tolist() == b.il.tolist()
    # one alphabet with N % 4 == 1 (npad), and so no multiple of 128 or 256 either, on every route
    for regime in ("mfma-whole", "mfma-sliced", "bf3-whole-sliced", "bf3-rounds", "bf3-main+tail"):
        assert any(c.N % 4 == 1 for c in _CASES if c.regime == regime), regime
    assert any(c.N % 4 == 0 and c.N % 256 for c in _CASES if c.regime == "f64-sliced")
    # the frame axis of the bf16x3 route
    for N in gc.FRAME_AXIS_N:
        kp = sorted(c.Kp for c in gc.frame_axis_cases() if c.N == N and "mixed" not in c.name and "deep" not in c.name)
        assert kp == list(gc.FRAME_AXIS_KP[N]) and {0, 1} <= set(kp)
        m = _BY_NAME["frames-mixed-N%d" % N]
        il = m.il.tolist()
        assert any(il[b] == 1 and il[b - 1] >= 2 and max(il[b + 1:]) >= 2 for b in range(1, m.B - 1))
        assert len(m.infeasible) == 1 and all(int(m.tl[b]) > il[b] for b in m.infeasible)
    assert {15, 16, 17, 31, 32, 33} <= set(gc.FRAME_AXIS_KP[1100])
    tks = gc.g3_plan(1100)["tks"]
    assert tks >= 3 and {1, 2} <= {k for k in gc.FRAME_AXIS_KP[1100] if 0 < k < tks}          # fewer rows than slices
    # a slice is whole 16-row stages: with K' = 81 valid rows each of the six slices has one stage and the LAST one holds a valid
    # row (rows 80 .. 95); with fewer it multiplies the zero padding of the packed planes, and a slice sum that stops one slice
    # early goes unseen
    assert tks == 6 and max(gc.FRAME_AXIS_KP[1100]) == 16 * (tks - 1) + 1 and (81 + 31) // 32 * 2 == tks
    assert "const int per = (nall + ks - 1) / ks, first = min(slice * per, nall);" in _src("asg_generic_grad.hip")
    assert "const int nst = min(first + per, nall) - first;" in _src("asg_generic_grad.hip")
    assert "const bool issue = loader && st + 2 < nst;" in _src("asg_generic_grad.hip")
    assert gc.g3_stages(81, 6) == [1] * 6 and gc.g3_stages(33, 6) == [1, 1, 1, 1, 0, 0] and gc.g3_stages(33, 1) == [4]
    # the steady state of the loop: a workgroup with more than two stages issues transfers inside the loop and waits with
    # vmcnt(ND); with more than three it reuses a stage of the ring.  frames-deep-N1100: every slice has four, all rows valid
    c = _BY_NAME["frames-deep-N1100"]
    assert c.Kp == 354 and c.route()[1]["tks"] == 6 and gc.g3_stages(c.Kp, 6) == [4] * 6 and c.Kp > 16 * 4 * 5
    # ... and it is the only one: everything else stays at one or two stages a workgroup (the cost of the oracle, N^2 a row)
    for o_ in _CASES:
        if not o_.f64 and o_.N > gc.G3_MIN_N and o_ is not c:
            p_ = o_.route()[1]
            assert max(gc.g3_stages(o_.Kp, p_["tks"]) + gc.g3_stages(o_.Kp, 1) * (p_["mainb"] > 0)) <= 2, o_.name
    # a valid row in the second slice (rows 16 ..) of a few-slice launch: at N = 2048, since from 2049 labels on T B <= 12 leaves
    # at most 9 valid rows (the tks = 2 | 3 pair at N = 2816 | 2817 checks the plan and that slices of padding add zero)
    c = _BY_NAME["bf3-Nt8-N2048"]
    assert c.route()[1]["tks"] == 4 and gc.g3_stages(c.Kp, 4) == [1, 1, 0, 0] and c.Kp > 16
    for n in ("bf3-N1025", "bf3-3-slices-N2817", "bf3-tail-N5121"):
        c = _BY_NAME[n]
        assert 0 < (c.Kp + 31) // 32 * 2 < c.route()[1]["tks"], n
    # weights
    for c in _CASES:
        w = c.w.tolist()
        assert 1.0 in w and min(w) == -0.5 and (c.B < 3 or 0.0 in w) and (c.B < 4 or max(w) == 1.5)


def _old_rule(x, ref):
    return util.tol_ok(x, ref, gc.OLD_RTOL)


@pytest.mark.parametrize("case", _CASES, ids=[c.name for c in _CASES])
def test_the_case_bites(case):
    """From the oracle alone: the cells left to the old rule stay under 1 %, and three mutations of the oracle's own tensors each
    fail the own-scale rule -- the full part times 1.01, one 16 x 16 block of grad_transition's full part zeroed at the last tile
    corner, the last valid frame row's edge posterior taken out.  What the OLD rule makes of them is printed; from 2049 labels on it
    lets all three through in grad_transition (asserted at the small shapes, T B <= 12; in a wide batch the one row taken out can
    carry a weight of 1.5 and reach 1.3e-4), which is why this file exists."""
    o = gc.reference(case)
    g = gc.gate(case.dtype)
    N = case.N
    gtr, gin = o["grad_transition_full"], o["grad_inputs_full"]
    assert np.isfinite(gtr).all() and np.isfinite(gin).all() and np.isfinite(o["grad_transition"]).all()
    share_t, share_i = gc.excluded_share(case, o)
    assert share_t <= gc.EXCLUDED_CAP, (case.name, share_t)
    if case.gin_in_training:
        assert share_i <= gc.EXCLUDED_CAP, (case.name, share_i)
    else:
        assert N < 100          # (one target label of a row is more than 1 % of it: grad_inputs is left to the full-lattice call)
    for b in range(case.B):
        assert not gin[int(case.il[b]):, b].any()
        if float(case.w[b]) == 0.0:
            assert not gin[:, b].any()
    assert gc.row_errs(gin, gin, case.il.tolist())[0] == 0.0
    # the reference of the training call (fp32 sum of the parts) is the full part on the cells compared: far inside the gate
    mt, mi = gc.training_cells(o)
    assert gc.own_scale_err(o["grad_transition"], gtr, mt) < 1e-12 and gc.own_scale_err(o["grad_inputs"], gin, mi) < 1e-12
    rec = ["excluded %.2e of grad_transition, %.2e of a row" % (share_t, share_i)]
    # 1. the full part times 1.01
    e = gc.row_errs(1.01 * gin, gin, case.il.tolist())[0]
    assert e > g and gc.own_scale_err(1.01 * gin, gin) > g
    rec.append("gin x 1.01: old rule %s" % ("passes" if _old_rule(o["grad_inputs"] + 0.01 * gin, o["grad_inputs"])[0] else "fails"))
    live = [b for b in range(case.B) if int(case.il[b]) >= 2 and float(case.w[b]) != 0.0]
    if not live:
        assert case.Kp == 0 and not gtr.any(), case.name          # (no transition: the full part of grad_transition is exactly zero)
        print("%s: %s" % (case.name, "; ".join(rec)))
        return
    old = []
    peak = np.abs(gtr).max()
    old_scale = max(1.0, float(np.abs(o["grad_transition"]).max()))
    # (the comparison in the training call is on a subset of the cells: the mutations must show there too)
    for what, mut in (("x 1.01", 1.01 * gtr), ("corner block zeroed", None), ("last row dropped", None)):
        if what == "corner block zeroed":
            mut = gtr.copy()
            mut[N - 16:, N - 16:] = 0.0
        elif what == "last row dropped":
            post, b, t = gc.last_row_posterior(case)
            assert float(case.w[b]) != 0.0 and b == max(bb for bb in range(case.B) if int(case.il[bb]) >= 2)
            mut = gtr - post
            assert np.abs(post).max() > 1e-3 * peak
        assert gc.own_scale_err(mut, gtr) > g, (case.name, what)
        assert gc.own_scale_err(mut, gtr, mt) > g, (case.name, what, "cells of the training call")
        ok, err = _old_rule(o["grad_transition"] + (mut - gtr), o["grad_transition"])
        old.append(ok)
        rec.append("gtr %s: old rule %s (%.1e)" % (what, "passes" if ok else "fails", err))
    print("%s: %s" % (case.name, "; ".join(rec)))
    if N >= 2049 and case.T * case.B <= 12:
        assert all(old), (case.name, rec)
