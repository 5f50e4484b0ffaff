"""CPU tests behind tests/test_hip_viterbi_regimes.py: from the numpy restatements alone they assert that
every case of the GPU module is in the regime it is named for and that it bites -- a wrong tie rule gives other outputs, the
paths cross the blocks and strips they are meant to cross -- and they pin the aligner's restatement (tests/viterbi_ref.py)
against the oracle and exhaustive enumeration, and the C entry points `asg_viterbi` / `asg_viterbi_work_bytes` without a
device.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import viterbi_regime_cases as C
from decode_ref import decode_ref
from oracle import asg_oracle as orc
from viterbi_ref import labels_of, viterbi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    return open(os.path.join(ROOT, "torch_asg_amd", "csrc", name)).read()


# ---- the restated launch arithmetic against the source ------------------------------------------------------------------------
def test_restated_constants_match_the_source():
    v = _src("asg_viterbi.hip")
    assert int(re.search(r"constexpr int kVPF = (\d+);", v).group(1)) == C.K_VPF
    one, other = re.search(r"constexpr int PF = KP == 1 \? (\d+) : (\d+);", v).groups()
    assert (int(one), int(other)) == (C.WIDE_PF[1], C.WIDE_PF[4]) and C.WIDE_PF[8] == C.WIDE_PF[4]
    # launch_viterbi_small: the edges of the four kernels, in order
    assert [int(e) for e in re.findall(r"if \(P\.S <= (\d+)\)", v)] == [64, 1024, 4096, C.ALIGN_MAX_S]
    assert "dim3((P.S + 63) / 64 * 64)" in v and "const bool take = come > stay;" in v
    assert v.count("c0 -= 64") == 2 and v.count("min(63, len - 1 - c0)") == 2
    d = _src("asg_decode.hip")
    assert int(re.search(r"constexpr int kEPFMax = (\d+);", d).group(1)) == C.K_EPF
    assert int(re.search(r"constexpr int kBTF = (\d+);", d).group(1)) == C.BT
    assert "constexpr bool KEEP = KS == 1 && sizeof(R) * NP <= 256;" in d
    assert "return N <= (elem == 8 ? 128 : 256);" in d
    edges = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"if \(N <= (\d+)\) ASG_DECODE_RES\((\d+), (\d+)\);", d)]
    assert edges == [(n, n, 1) for n in range(8, 65, 8)] + [(128, 64, 2)]
    assert "else if constexpr (sizeof(R) == 4) ASG_DECODE_RES(64, 4);" in d
    assert "sizeof(R) == 8 ? 8 : (P.B <= 4 ? 4 : (P.B <= 8 ? 8 : 16))" in d and "(nrt + 7) / 8 * 8 * ngr" in d


def test_align_kernel_table():
    A = C.align_kernel
    assert A(1) == A(63) == A(64) == ("small", 1, 64, 1, 16)
    assert A(65) == ("wide", 1, 128, 2, 8) and A(128) == ("wide", 1, 128, 2, 8) and A(129) == ("wide", 1, 192, 3, 8)
    assert A(1023) == A(1024) == ("wide", 1, 1024, 16, 8)
    assert A(1025) == ("wide", 4, 1024, 17, 2) and A(1088) == ("wide", 4, 1024, 17, 2)
    assert A(4095) == A(4096) == ("wide", 4, 1024, 64, 2)
    assert A(4097) == ("wide", 8, 1024, 65, 2) and A(8191) == A(8192) == ("wide", 8, 1024, 128, 2)


def test_decode_route_table():
    R = C.decode_route
    for e in (4, 8):
        for n in range(1, 65):
            r = R(e, n, 4)
            assert r.KS == 1 and r.threads == 64 and r.NP == (n + 7) // 8 * 8 and r.NP - 8 < n <= r.NP
            assert r.KEEP == (e * r.NP <= 256)
        assert R(e, 65, 4) == R(e, 128, 4) == (64, 2, False, 256)
    assert R(4, 64, 4).KEEP and R(8, 32, 4).KEEP and not R(8, 33, 4).KEEP
    assert R(4, 129, 4) == R(4, 256, 4) == (64, 4, False, 1024)
    assert R(8, 129, 4) == (192, 3, 8, 1, 8) and R(8, 129, 9) == (192, 3, 8, 2, 16)
    assert R(4, 257, 4) == (320, 5, 4, 1, 8) and R(4, 257, 5) == (320, 5, 8, 1, 8) and R(4, 257, 9) == (320, 5, 16, 1, 8)
    assert R(4, 257, 17) == (320, 5, 16, 2, 16) and R(4, 520, 16) == (576, 9, 16, 1, 16) and R(4, 520, 17) == (576, 9, 16, 2, 32)


# ---- the aligner's restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("seed", range(4))
def test_viterbi_ref_equals_the_oracle_bit_for_bit(seed, dtype):
    rng = np.random.default_rng(300 + seed)
    for k in range(12):
        T, B, N = int(rng.integers(1, 90)), int(rng.integers(1, 7)), int(rng.integers(1, 9))
        S = int(rng.integers(1, T + 1))
        x = rng.normal(size=(T, B, N)).astype(dtype)
        tr = rng.normal(size=(N, N)).astype(dtype)
        tg = rng.integers(0, N, size=(B, S))
        il = rng.integers(0, T + 2, size=B)                          # 0: nothing to align; T + 1: clamped
        tl = rng.integers(0, S + 2, size=B)                          # tl > il happens: infeasible
        il[0], tl[0] = T, S
        if k % 3 == 1:
            x[rng.random(size=x.shape) < 0.2] = -np.inf              # masked emissions
        if k % 3 == 2:
            x[T // 2, B - 1, :] = -np.inf                            # a frame nothing can emit
        if k % 4 == 3:
            x = np.ascontiguousarray(x.transpose(1, 0, 2)).transpose(1, 0, 2)      # batch-major storage
        sc, pos = viterbi_ref(x, tg, tr, il, tl)
        so, po = orc.viterbi(x, tg, tr, il, tl)
        assert sc.dtype == np.dtype(dtype) and np.array_equal(sc, so) and np.array_equal(pos, po)
        sc2, pos2 = viterbi_ref(x, tg, tr, None, None)
        so2, po2 = orc.viterbi(x, tg, tr, None, None)
        assert np.array_equal(sc2, so2) and np.array_equal(pos2, po2)


def test_viterbi_ref_equals_exhaustive_enumeration():
    # emissions and transitions on a grid of 1 / 1024: every sum is exact, so the two orders of addition agree to the bit
    rng = np.random.default_rng(77)
    for _ in range(150):
        T, N, L = int(rng.integers(1, 8)), int(rng.integers(1, 4)), int(rng.integers(1, 6))
        x = np.round(rng.normal(size=(T, 1, N)) * 1024) / 1024
        tr = np.round(rng.normal(size=(N, N)) * 1024) / 1024
        tg = rng.integers(0, N, size=(1, L))
        il, tl = np.array([rng.integers(1, T + 1)]), np.array([rng.integers(1, L + 1)])
        sc, pos = viterbi_ref(x, tg, tr, il, tl)
        best, bp = orc.brute_force_viterbi(x[:, 0], tg[0], tr, il[0], tl[0])
        if bp is None:
            assert sc[0] == -np.inf and (pos == -1).all()
        else:
            assert sc[0] == best and list(pos[0, :il[0]]) == bp and (pos[0, il[0]:] == -1).all()


def test_viterbi_ref_tie_rule_by_hand():
    # everything ties: "stay" wins every comparison, so the walk from the end advances as EARLY as possible; `>=` as late
    x = np.zeros((6, 1, 3), np.float32)
    tg, tr = np.array([[0, 1, 2]]), np.zeros((3, 3), np.float32)
    sc, pos = viterbi_ref(x, tg, tr)
    assert sc[0] == 0 and list(pos[0]) == [0, 1, 2, 2, 2, 2]
    sc, pos = viterbi_ref(x, tg, tr, take=np.greater_equal)
    assert sc[0] == 0 and list(pos[0]) == [0, 0, 0, 0, 1, 2]
    assert list(labels_of(tg, np.array([[0, 1, 1, 2, -1, -1]]))[0]) == [0, 1, 1, 2, -1, -1]


# ---- aligner cases: regimes -------------------------------------------------------------------------------------------------------
def _valid_alignment(case):
    sc, pos = case.ref()
    for b in range(case.B):
        n, o = int(min(case.il[b], case.T)), int(min(case.tl[b], case.S, case.T))
        if not sc[b] > -np.inf:
            assert (pos[b] == -1).all()
            continue
        p = pos[b, :n]
        assert p[0] == 0 and p[-1] == o - 1 and ((np.diff(p) == 0) | (np.diff(p) == 1)).all() and (pos[b, n:] == -1).all()


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_kernel_cases_sit_on_both_sides_of_every_switch(dtype):
    kinds = {}
    for S in C.KERNEL_S:
        c = C.kernel_case(S, dtype)
        assert (c.T, c.B, c.S) == (S + 3, 3, S) and list(c.tl[:2]) == [S, 1]
        edge = int(c.tl[2])
        assert (S < 64 and edge == max(1, S // 2)) or edge % 64 == (1 if dtype == "float32" else 0) or edge == S
        kinds[S] = (c.kernel.kind, c.kernel.KP)
    assert [kinds[s] for s in (1, 63, 64)] == [("small", 1)] * 3
    assert [kinds[s] for s in (65, 128, 129, 1023, 1024)] == [("wide", 1)] * 5
    assert [kinds[s] for s in (1025, 1088, 4095, 4096)] == [("wide", 4)] * 4
    assert [kinds[s] for s in (4097, 8191, 8192)] == [("wide", 8)] * 3
    # one position per thread: every workgroup size on a side of a strip (64 | 65, 128 | 129), the full one from below and at it
    assert [C.kernel_case(s, dtype).kernel.threads for s in (65, 128, 129, 1023, 1024)] == [128, 128, 192, 1024, 1024]
    for S in C.SINGLE_S:
        c = C.kernel_case(S, dtype, True)
        assert c.T == S and c.tl[0] == S
        assert list(c.ref()[1][0]) == list(range(S))                 # the single alignment: position = frame


@pytest.mark.parametrize("S", [1, 63, 64, 65, 129, 1024, 1025])
def test_small_kernel_cases_have_valid_alignments(S):
    # (the wide ones are checked where their references are needed anyway: the GPU module; these are cheap)
    for dtype in C.DTYPES:
        c = C.kernel_case(S, dtype)
        assert np.isfinite(c.ref()[0]).all()
        _valid_alignment(c)


def _other_cases(dtype):
    yield from (C.kernel_case(S, dtype) for S in C.KERNEL_S)
    yield from (C.kernel_case(S, dtype, True) for S in C.SINGLE_S)
    yield from (C.chunk_case(T, S, dtype) for T, S in C.CHUNK_TS)
    yield from (C.ring_case(20, dtype, 0), C.ring_case(20, dtype, 1), C.ring_case(300, dtype), C.ring_case(1025, dtype))
    yield from (C.inf_case(S, dtype) for S in C.INF_S)
    yield from (C.host_case(S, dtype, seed) for S in C.HOST_S for seed in (0, 1, 2))


def _same_under_the_other_rule(c):
    wsc, wpos = viterbi_ref(c.x, c.tg[:, :c.T], c.tr, c.il, np.minimum(c.tl, c.T), take=np.greater_equal)
    assert np.array_equal(wsc, c.ref()[0]) and np.array_equal(wpos, c.ref()[1]), c


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_only_the_tie_cases_depend_on_the_tie_rule(dtype):
    # neighbouring equal targets tie exactly whatever the emissions are (the same label and transition on both branches): every
    # case but the tie cases has none, and gives the same alignment under `>=` (here: up to 1500 positions)
    for c in _other_cases(dtype):
        assert (c.tg[:, 1:] != c.tg[:, :-1]).all(), c
        if c.S <= 1500:
            _same_under_the_other_rule(c)


BIG_F32 = [(S, False) for S in C.KERNEL_S if S > 1500] + [(S, True) for S in C.SINGLE_S if S > 1500]


@pytest.mark.parametrize("S,single", BIG_F32, ids=["S%d%s" % (s, "_single" if g else "") for s, g in BIG_F32])
def test_wide_float32_cases_have_no_rounding_ties(S, single):
    # float32 sums of several thousand round to equal values now and then (KERNEL_SALT); float64 sums do not
    _same_under_the_other_rule(C.kernel_case(S, "float32", single))


# ---- aligner cases: the tie rule bites --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("T,S", C.TIE_TS, ids=["S%d" % s for _, s in C.TIE_TS])
def test_aligner_tie_cases_tell_the_two_rules_apart(T, S, dtype):
    c = C.align_tie_case(T, S, dtype)
    assert (c.T, c.S) == (T, S)
    assert c.kernel == C.align_kernel(S)
    sc, pos = c.ref()
    _valid_alignment(c)
    wsc, wpos = viterbi_ref(c.x, c.tg, c.tr, c.il, c.tl, take=np.greater_equal)
    assert np.array_equal(sc, wsc) and np.isfinite(sc).all()          # the score cannot tell the rules apart ...
    diff = pos != wpos
    assert diff[0].any() and diff[1].any()                            # ... the positions do, in every utterance
    print("%s: positions differ at %d + %d frames" % (c, diff[0].sum(), diff[1].sum()))
    if c.kernel.KP > 1:
        # ... and not in one thread's first positions only: in at least two blocks of 1024 positions (k of tid + 1024 k)
        blocks = set((pos[diff] // 1024).tolist())
        assert len(blocks) >= 2, blocks
        strips = set((pos[diff] // 64).tolist())
        print("%s: 1024-blocks %s, strips %d .. %d" % (c, sorted(blocks), min(strips), max(strips)))


# ---- aligner cases: backtrace blocks, strip words, prefetch rings, -inf -------------------------------------------------------------
def _crossings(p):
    """Per 64-frame block of one utterance's positions p[0..len): (a strip is crossed inside the block, the block's first
    position is a strip's first, the block's last position is a strip's first)."""
    out = []
    for c0 in range(0, len(p), 64):
        q = p[c0:c0 + 64]
        inside = bool(((q[1:] % 64 == 0) & (q[1:] == q[:-1] + 1)).any())
        out.append((inside, q[0] % 64 == 0 and q[0] > 0, q[-1] % 64 == 0 and q[-1] > 0))
    return out


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("T,S", C.CHUNK_TS, ids=["S%d" % s for _, s in C.CHUNK_TS])
def test_chunk_cases_have_the_lengths_and_cross_the_strips(T, S, dtype):
    c = C.chunk_case(T, S, dtype)
    assert list(c.il) == [1, 2, 63, 64, 65, 127, 128, 129, T] and (c.tl <= np.minimum(c.il, S)).all() and (c.tl >= 1).all()
    assert c.kernel.kind == ("small" if S <= 64 else "wide") and c.kernel.KP == (1 if S < 1025 else 4)
    sc, pos = c.ref()
    assert np.isfinite(sc).all()
    _valid_alignment(c)
    if c.kernel.kind == "small":
        return
    assert c.kernel.nw == (min(S, T) + 63) // 64 >= 3
    seen = [x for b in range(c.B) for x in _crossings(pos[b, :c.il[b]])]
    assert any(i for i, _, _ in seen), "no block whose path crosses a strip (the w_lo word is never read)"
    assert any(f for _, f, _ in seen), "no block that begins on a strip's first position"
    assert any(e for _, _, e in seen), "no block whose walk starts on a strip's first position"
    # the walk of a block goes DOWN from its last frame: a block with a crossing inside reads both words
    blocks_with_two_words = sum(1 for i, _, _ in seen if i)
    print("%s: %d blocks read both mask words" % (c, blocks_with_two_words))


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_ring_cases_have_lengths_around_every_prefetch_depth(dtype):
    a, b = C.ring_case(20, dtype, 0), C.ring_case(20, dtype, 1)
    assert list(a.il) + list(b.il) == list(range(1, 19)) and a.kernel.PF == 16 == C.K_VPF and a.kernel.kind == "small"
    assert {15, 16, 17, 18} <= set(b.il.tolist())                      # below, at and above the ring's depth (frames 1 .. len - 1)
    for S, KP, PF in ((300, 1, 8), (1025, 4, 2)):
        c = C.ring_case(S, dtype)
        assert list(c.il) == [1, 2, 3, 9, 10] and (c.kernel.kind, c.kernel.KP, c.kernel.PF) == ("wide", KP, PF)
        assert c.S == S and c.T >= S
    for c in (a, b, C.ring_case(300, dtype), C.ring_case(1025, dtype)):
        assert (c.tl <= c.il).all() and np.isfinite(c.ref()[0]).all()
        _valid_alignment(c)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("S", C.INF_S)
def test_inf_cases_keep_finite_alignments_among_masked_cells(S, dtype):
    c = C.inf_case(S, dtype)
    assert c.kernel.kind == "wide" and c.kernel.KP == (1 if S == 300 else 4)
    frac = np.isneginf(c.x).mean()
    assert 0.40 < frac < 0.5                                           # one half drawn, one alignment per utterance restored
    sc, pos = c.ref()
    assert np.isfinite(sc[:3]).all() and sc[3] == -np.inf and (pos[3] == -1).all()
    assert np.isneginf(c.x[c.T // 2, 3]).all()
    _valid_alignment(c)
    so, po = orc.viterbi(c.x, c.tg, c.tr, c.il, c.tl)
    assert np.array_equal(sc, so) and np.array_equal(pos, po)
    # the best alignment is found among masked cells: without the mask it would be another one
    x0 = np.where(np.isneginf(c.x), c.x.dtype.type(0), c.x)
    assert (viterbi_ref(x0, c.tg, c.tr, c.il, c.tl)[1][:3] != pos[:3]).any()


# ---- decoder cases ---------------------------------------------------------------------------------------------------------------
def test_instance_cases_run_every_instantiation():
    seen = {d: set() for d in C.DTYPES}
    for dtype in C.DTYPES:
        for N in C.INSTANCE_N:
            for integer in (False, True):
                c = C.instance_case(N, dtype, integer)
                assert (c.T, c.B, c.N) == (70, 4, N) and list(c.il) == [70, 0, 1, 64]
                r = c.route
                seen[dtype].add(("res", r.NP, r.KS, r.KEEP) if isinstance(r, C.Resident) else ("str", r.PAD))
    one = {("res", np_, 1, True) for np_ in range(8, 65, 8)}
    assert seen["float32"] == one | {("res", 64, 2, False), ("res", 64, 4, False), ("str", 320)}
    one64 = {("res", np_, 1, np_ <= 32) for np_ in range(8, 65, 8)}
    assert seen["float64"] == one64 | {("res", 64, 2, False), ("str", 192), ("str", 256), ("str", 320)}
    # float64: KEEP switches between N = 32 and 33
    assert C.instance_case(32, "float64", False).route.KEEP and not C.instance_case(33, "float64", False).route.KEEP


def _tied_slices(case, b):
    """Frames of utterance b at which the maxima of the reference path's back-pointer lie in more than one 64-column slice."""
    sc, path, _, _ = case.ref()
    x, tr, L = case.x, case.tr, int(case.il[b])
    v = x[0, b].copy()
    frames = []
    for t in range(1, L):
        cand = v + tr[path[b, t]]
        where = np.nonzero(cand == cand.max())[0]
        if len(set((where // 64).tolist())) >= 2:
            frames.append(t)
        v = (v[None, :] + tr).max(axis=1) + x[t, b]
    return frames


def _decoder_tie_bite(c):
    ref = c.ref()
    wrong = decode_ref(c.x, c.tr, c.il, argmax=C.last_index_argmax)
    assert np.array_equal(ref[0], wrong[0])                            # the score cannot tell the rules apart ...
    assert not np.array_equal(ref[1], wrong[1])                        # ... the path does
    if isinstance(c.route, C.Resident) and c.route.KS > 1:
        frames = _tied_slices(c, 0)
        assert frames, "no frame whose tied maxima lie in two slices"
        return len(frames)
    return 0


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_decoder_tie_cases_tell_first_index_from_last(dtype):
    for N in C.SLICE_TIE_N[dtype]:
        c = C.slice_tie_case(N, dtype)
        assert isinstance(c.route, C.Resident) and c.route.KS == (2 if N <= 128 else 4)
        n = _decoder_tie_bite(c)
        print("%s: %d frames of utterance 0 tie across slices" % (c, n))
    # the integer half of the instantiation table: every one of its cases ties, the sliced ones across slices
    ks = set()
    for N in C.INSTANCE_N:
        c = C.instance_case(N, dtype, True)
        _decoder_tie_bite(c)
        if isinstance(c.route, C.Resident):
            ks.add(c.route.KS)
    assert ks == ({1, 2, 4} if dtype == "float32" else {1, 2})


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("N", C.BLOCK_N)
def test_block_cases_decode_their_schedules(N, dtype):
    c = C.block_case(N, dtype)
    assert list(c.il) == [1, 2, 7, 8, 9, 10, 63, 64, 65, 127, 128, 129, 130] and c.T == 130
    sc, path, tok, tl = c.ref()
    run63, change64, run127, change128 = False, False, False, False
    for b in range(c.B):
        L = int(c.il[b])
        assert np.array_equal(path[b, :L], c.schedule[b, :L])          # +20 per frame: the decoded path is the schedule
        p = path[b, :L]
        assert tl[b] == 1 + int((p[1:] != p[:-1]).sum())
        if L > 64:
            run63 |= bool(p[63] == p[64])
            change64 |= bool(p[63] != p[64])
        if L > 128:
            run127 |= bool(p[127] == p[128])
            change128 |= bool(p[127] != p[128])
    assert run63 and change64 and run127 and change128
    kinds = {40: (40, 1), 100: (64, 2), 200: (64, 4)}
    if N in kinds and not (N == 200 and dtype == "float64"):
        assert (c.route.NP, c.route.KS) == kinds[N]
    else:
        assert isinstance(c.route, C.Streaming)
    # lengths on both sides of the prefetch depth (frames 1 .. len - 1 in groups of 8) and of the 64-frame blocks
    assert {8, 9, 10} <= set(c.il.tolist()) and C.K_EPF == 8


def test_uint8_case_has_back_pointers_above_127_and_at_255():
    c = C.uint8_case()
    assert c.route == (64, 4, False, 1024) and c.x.dtype == np.float32
    sc, path, _, _ = c.ref()
    bp = np.concatenate([path[b, :int(c.il[b]) - 1] for b in range(c.B)])          # the back-pointer of frame t is path[t - 1]
    assert (bp == 255).sum() >= 4 and ((bp >= 128) & (bp < 255)).sum() >= 4 and (bp < 128).any()
    print("uint8 case: %d back-pointers, %d at 255, %d in 128 .. 254" % (len(bp), (bp == 255).sum(), ((bp >= 128) & (bp < 255)).sum()))


def test_stream_cases_cover_the_grid():
    seen = set()
    for dtype in C.DTYPES:
        for N in C.STREAM_N:
            for B in C.STREAM_B[dtype]:
                c = C.stream_case(N, B, dtype)
                r = c.route
                assert isinstance(r, C.Streaming) and r.nrt == (5 if N == 257 else 9) and c.T == 6
                assert r.nblk == (8 if N == 257 else 16) * r.ngr and r.nblk > r.nrt * r.ngr          # idle blocks: rt >= nrt returns
                assert c.il[0] == 6 and c.il[-1] == 6
                seen.add((dtype, r.UB, r.ngr, B % r.UB != 0))
    # UB = 4 / 8 / 16 full and clamped (the last group of a batch that is no multiple of UB reads utterance B - 1 again)
    assert seen == {("float32", 4, 1, False), ("float32", 8, 1, True), ("float32", 8, 1, False), ("float32", 16, 1, True),
                    ("float32", 16, 1, False), ("float32", 16, 2, True), ("float64", 8, 1, False), ("float64", 8, 2, True)}


# ---- the C entry points: no kernel is launched -------------------------------------------------------------------------------------
def _problem(T, B, N, S, dtype):
    from torch_asg_amd import _lib
    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.S = T, B, N, S
    p.dtype = dtype
    p.inputs, p.transition, p.targets = 16, 16, 16          # never dereferenced: only sizes / checks
    return p


def test_library_exports_the_aligner():
    from torch_asg_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "asg_viterbi") and hasattr(L, "asg_viterbi_work_bytes")
    assert {"asg_viterbi", "asg_viterbi_work_bytes"} <= set(_lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    assert "size_t asg_viterbi_work_bytes(const asg_problem *p);" in hdr and "int asg_viterbi(asg_ctx *ctx" in hdr


@pytest.mark.parametrize("T,B,S", [(7, 3, 1), (70, 3, 64), (70, 3, 65), (400, 64, 128), (400, 5, 129), (1100, 3, 1024),
                                   (1100, 3, 1025), (4200, 2, 4097), (8300, 1, 8192)])
def test_viterbi_work_bytes_follow_the_documented_formula(T, B, S):
    from torch_asg_amd import _lib
    L = _lib.lib()
    for dt in (_lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64):
        p = _problem(T, B, 8, S, dt)
        assert L.asg_viterbi_work_bytes(ctypes.byref(p)) == B * T * ((S + 63) // 64) * 8 == C.align_work_bytes(T, B, S)


def test_viterbi_argument_validation():
    from torch_asg_amd import _lib
    L = _lib.lib()
    INVALID, UNSUPPORTED, WORKSPACE = 1, 2, 3                        # include/asg_hip.h: ASG_ERR_*
    hdr = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    for name, val in (("INVALID", INVALID), ("UNSUPPORTED", UNSUPPORTED), ("WORKSPACE", WORKSPACE)):
        assert re.search(r"#define ASG_ERR_%s %d\b" % (name, val), hdr)
    p = _problem(10, 2, 8, 5, _lib.ASG_DTYPE_F32)
    assert L.asg_viterbi_work_bytes(None) == 0
    assert L.asg_viterbi(None, None, None, 0, None, None, 0, None) == INVALID
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.addressof(buf)
    # null work / scores / path
    assert L.asg_viterbi(None, ctypes.byref(p), None, 1 << 12, a, a, 0, None) == INVALID
    assert L.asg_viterbi(None, ctypes.byref(p), a, 1 << 12, None, a, 0, None) == INVALID
    assert L.asg_viterbi(None, ctypes.byref(p), a, 1 << 12, a, None, 0, None) == INVALID
    # a workspace one byte short
    need = L.asg_viterbi_work_bytes(ctypes.byref(p))
    assert need == 2 * 10 * 1 * 8
    assert L.asg_viterbi(None, ctypes.byref(p), a, need - 1, a, a, 0, None) == WORKSPACE
    # no targets, no emissions, empty shapes, a bad dtype
    for field in ("targets", "inputs", "transition"):
        q = _problem(10, 2, 8, 5, _lib.ASG_DTYPE_F32)
        setattr(q, field, None)
        assert L.asg_viterbi_work_bytes(ctypes.byref(q)) == 0
        assert L.asg_viterbi(None, ctypes.byref(q), a, 1 << 12, a, a, 0, None) == INVALID
    for T, B, N, S in ((0, 2, 8, 5), (10, 0, 8, 5), (10, 2, 0, 5), (10, 2, 8, 0)):
        q = _problem(T, B, N, S, _lib.ASG_DTYPE_F32)
        assert L.asg_viterbi(None, ctypes.byref(q), a, 1 << 12, a, a, 0, None) == INVALID
    q = _problem(10, 2, 8, 5, 7)
    assert L.asg_viterbi_work_bytes(ctypes.byref(q)) == 0
    assert L.asg_viterbi(None, ctypes.byref(q), a, 1 << 12, a, a, 0, None) == INVALID
    # more than 8192 target positions: refused, in both entry points
    q = _problem(8300, 1, 8, 8193, _lib.ASG_DTYPE_F32)
    assert L.asg_viterbi_work_bytes(ctypes.byref(q)) == 0
    assert L.asg_viterbi(None, ctypes.byref(q), a, 1 << 12, a, a, 0, None) == UNSUPPORTED
    q = _problem(8300, 1, 8, 8192, _lib.ASG_DTYPE_F32)
    assert L.asg_viterbi_work_bytes(ctypes.byref(q)) == 8300 * 128 * 8
    # bfloat16 emissions are the fused pair's alone (viterbi_align widens them before it gets here)
    q = _problem(10, 2, 8, 5, _lib.ASG_DTYPE_F32)
    q.inputs_dtype = _lib.ASG_DTYPE_BF16
    assert L.asg_viterbi_work_bytes(ctypes.byref(q)) == 0
    assert L.asg_viterbi(None, ctypes.byref(q), a, 1 << 12, a, a, 0, None) == UNSUPPORTED
    q.dtype = _lib.ASG_DTYPE_F64
    assert L.asg_viterbi(None, ctypes.byref(q), a, 1 << 12, a, a, 0, None) == INVALID
