"""Test-only helpers shared by tests/test_hip_generic_grad_regimes.py (GPU) and tests/test_generic_grad_regimes_cpu.py (DESIGN.md
5c.1): the rule that measures the full-lattice gradient of the generic loss (N > 64) at the scale of its own values, the launch
rules of csrc/asg_generic_grad.hip restated so that a case can assert the regime it names, and the memoised cases with their fp64
references.  Nothing here needs a GPU.

Why a rule of its own: grad_inputs and grad_transition are the sum of an aligned part (O(1) entries on a handful of cells) and a
full-lattice part that spreads one unit of posterior over N labels / N^2 cells.  The parity rule of tests/util.py,
max|x - ref| <= 1e-4 * max(1, max|ref|), is scaled by the floor of 1 and by the aligned peak: from about 1000 labels up the whole
full-lattice part of grad_transition can be dropped or doubled inside it.

Draws are util.synth's (transitions `rand`, emissions `randn`, targets `randint`); lengths are the case's own.
"""
import functools

import numpy as np
import torch

import util
from oracle import asg_oracle as orc

# ---- the rule -------------------------------------------------------------------------------------------------------------------
GATE_F32, GATE_F64 = 1e-4, 1e-9          # the project's own numbers without the floor of 1
OLD_RTOL = 1e-4                          # util.tol_ok, the rule every other generic-path test uses
EXCLUDED_CAP = 0.01                      # share of cells the training-call comparison may leave to the old rule


def gate(dtype):
    return GATE_F64 if dtype == torch.float64 else GATE_F32


def own_scale_err(x, ref, cells=None):
    """max over `cells` (boolean mask, default all) of |x - ref|  /  max over ALL finite cells of |ref|.  Infinities must match in
    place and a NaN fails (both -> inf).  A reference that is zero everywhere admits exact zeros only."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    fin = np.isfinite(ref)
    scale = max(float(ref.max(where=fin, initial=0.0)), -float(ref.min(where=fin, initial=0.0)))
    with np.errstate(invalid="ignore"):
        d = x - ref                                        # (nan at inf - inf and at a NaN of either side)
    np.abs(d, out=d)
    if not fin.all():
        nf = ~fin
        d[nf] = np.where(x[nf] == ref[nf], 0.0, np.inf)      # infinities in place and of the same sign; a NaN equals nothing
    d = float(d.max(initial=0.0) if cells is None else d.max(where=np.asarray(cells, bool), initial=0.0))
    if d != d:
        return float("inf")
    if scale == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / scale


def tiles_of(label):
    """The tiles a label falls into: 16 (matrix-instruction block), 80 (row tile of the streaming step), 256 (bf16 contraction)."""
    return "tile/16 %d, /80 %d, /256 %d" % (label // 16, label // 80, label // 256)


def row_errs(gin, ref, il, w=None, cells=None, bitwise=False):
    """The rule per (t, b) row of grad_inputs, each at the scale of its own peak (a row is a distribution times the upstream
    weight: its peak is at least |g_b| / N).  -> (worst error, message naming b, t, the length, the label and its tiles).
    Rows of frames t >= len_b must be zero -- `bitwise`: +0.0, what a kernel that clears them writes -- (error inf otherwise)."""
    T, B, N = ref.shape
    worst, msg = 0.0, "no row"
    for b in range(B):
        n = int(min(max(int(il[b]), 0), T))
        tail = np.ascontiguousarray(gin[n:, b])
        if (tail.view(np.uint8) if bitwise else tail).any():
            return float("inf"), "b %d (length %d): frames behind the length are not%s zero" % (b, n, " bitwise" if bitwise else "")
        for t in range(n):
            e = own_scale_err(gin[t, b], ref[t, b], None if cells is None else cells[t, b])
            if e > worst:
                d = np.abs(np.asarray(gin[t, b], np.float64) - ref[t, b])
                if cells is not None:
                    d = np.where(cells[t, b], d, 0.0)
                lab = int(np.argmax(np.where(np.isfinite(d), d, np.inf)))
                worst = e
                msg = "b %d t %d (length %d%s): label %d (%s) is %.9g, reference %.9g, row peak %.3g" % (
                    b, t, n, "" if w is None else ", weight %g" % float(w[b]), lab, tiles_of(lab), float(gin[t, b, lab]),
                    float(ref[t, b, lab]), float(np.abs(ref[t, b]).max()))
    return worst, msg


# ---- csrc/asg_generic_grad.hip, restated (tests/test_generic_grad_regimes_cpu.py matches the numbers to the source) --------------
GEMM_BK = 32                              # ASG_X_GEMM_BK: k per stage of bwd_gemm_mfma, the rounding of its slices
F64_BK = 16                               # BK of bwd_gemm_kernel, the rounding of the fp64 slices
G3_TM, G3_TN = 256, 256                   # kG3TM, kG3TN
G3_TAIL_SLICES, G3_WHOLE_SLICES = 4, 8    # kG3TailSlices, kG3WholeSlices
G3_TAIL_BYTES = 208 << 20                 # kG3TailBytes
G3_MIN_N = 1024                           # ASG_X_G3_MIN_N = kG3MinN: the bf16x3 planes take over BEYOND it
SLICE_TILES, SLICE_MIN_ROWS = 512, 256    # gemm_slices: `tiles >= 512` and `K / 256`


def gemm_slices(N, K):
    tiles = ((N + 127) // 128) ** 2
    if tiles >= SLICE_TILES:
        return 1
    n = (SLICE_TILES + tiles - 1) // tiles
    if n > K // SLICE_MIN_ROWS:
        n = K // SLICE_MIN_ROWS
    return max(n, 1)


def kslice(K, nsl, f64=False):
    bk = F64_BK if f64 else GEMM_BK
    return ((K + nsl - 1) // nsl + bk - 1) // bk * bk


def g3_npadT(N):
    return (N + G3_TM - 1) // G3_TM * G3_TM


def g3_plan(N):
    """launch_bwd_full_generic's bf16x3 branch -> dict(Mt, Nt, blocks, tail, tks, mainb)."""
    npadT = g3_npadT(N)
    Mt, Nt = npadT // G3_TM, (N + G3_TN - 1) // G3_TN
    blocks = ((Mt + 3) // 4) * ((Nt + 7) // 8)
    tail, tks = blocks % 8, 1
    tile_bytes = G3_TM * G3_TN * 4
    if blocks <= 8:
        tail = blocks
        real = Mt * Nt
        best = float((real + 255) // 256)
        for t in range(2, G3_WHOLE_SLICES + 1):
            c = float((real * t + 255) // 256) / t
            if c < best - 0.05 and tail * 32 * t * tile_bytes <= G3_TAIL_BYTES:
                best, tks = c, t
    elif tail * 32 * 2 <= 256 and tail > 0:
        tks = min(256 // (tail * 32), G3_TAIL_SLICES)
    if tks < 2 or tail * 32 * tks * tile_bytes > G3_TAIL_BYTES:
        tail, tks = 0, 1
    return dict(Mt=Mt, Nt=Nt, blocks=blocks, tail=tail, tks=tks, mainb=blocks - tail)


def g3_stages(Kp, tks):
    """bwd_gemm_bf3_kernel: the 16-row stages (nst) of each of the tks slices of a frame axis of Kp valid rows."""
    nall = (Kp + 31) // 32 * 2
    per = (nall + tks - 1) // tks
    return [min(min(s * per, nall) + per, nall) - min(s * per, nall) for s in range(tks)]


def valid_rows(il, T):
    """K' = rowoff[B] of rowoff_kernel: frames 1 .. len - 1 of every utterance."""
    return int(sum(max(min(max(int(n), 0), T) - 1, 0) for n in il))


def contraction(N, T, B, f64):
    """The route grad_transition's contraction takes -> (name, details)."""
    K = B * T
    if f64:
        nsl = gemm_slices(N, K)
        return ("f64-sliced" if nsl > 1 else "f64-whole"), dict(nsl=nsl, kslice=kslice(K, nsl, True) if nsl > 1 else 0)
    if N > G3_MIN_N:
        p = g3_plan(N)
        if p["blocks"] <= 8:
            return ("bf3-whole-sliced" if p["tks"] > 1 else "bf3-round-unsliced"), p
        return ("bf3-main+tail" if p["tail"] else "bf3-rounds"), p
    nsl = gemm_slices(N, K)
    return ("mfma-sliced" if nsl > 1 else "mfma-whole"), dict(nsl=nsl, kslice=kslice(K, nsl) if nsl > 1 else 0)


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def weights(B):
    """Upstream weights from -0.5 to 1.5 with an exact 1.0 at utterance B // 2 and an exact 0.0 in front of it -- all of that from
    four utterances on; three have 0.0, 1.0 and -0.5 (no 1.5), two have -0.5 and 1.0 (no room for a 0.0 beside a negative and a
    unit weight), one has 1.0."""
    w = torch.linspace(-0.5, 1.5, B, dtype=torch.float64)
    if B >= 4:
        w[B // 2], w[B // 2 - 1] = 1.0, 0.0
    elif B == 3:
        w[0], w[1], w[2] = 0.0, 1.0, -0.5
    elif B == 2:
        w[1] = 1.0
    else:
        w[0] = 1.0
    return w


class Case:
    def __init__(self, name, regime, T, B, N, L, il=None, f64=False, seed=None, tl=None, shared_target=False, serial=False,
                 env=None, fwd=None, gin_in_training=True, infeasible=()):
        self.name, self.regime, self.f64, self.serial, self.fwd = name, regime, f64, serial, fwd
        self.T, self.B, self.N, self.L = T, B, N, L
        self.dtype = torch.float64 if f64 else torch.float32
        self.env = dict(env or {})
        self.gin_in_training = gin_in_training
        tr, x, tg, il0, tl0 = util.synth(T, B, N, L, N + 31 * T + B if seed is None else seed, True)
        # (fp64 cases run on the float32 draws widened: the same values in both precisions)
        self.tr, self.x = tr, x
        if shared_target:
            tg = tg[:1].repeat(B, 1)
        self.tg = tg
        self.il = il0 if il is None else torch.as_tensor(il, dtype=torch.int64)
        assert self.il.shape == (B,) and int(self.il.max()) <= T and int(self.il.min()) >= 0
        tl = tl0 if tl is None else torch.as_tensor(tl, dtype=torch.int64)
        self.tl = torch.clamp(torch.minimum(tl, self.il), min=1)
        for b in infeasible:
            self.tl[b] = min(L, int(self.il[b]) + 1)
            assert int(self.tl[b]) > int(self.il[b])
        self.infeasible = tuple(infeasible)
        self.w = weights(B)
        self.Kp = valid_rows(self.il.tolist(), T)

    def __repr__(self):
        return self.name

    def route(self):
        return contraction(self.N, self.T, self.B, self.f64)


def spread(Kp, B, T, skip=None):
    """Lengths of B utterances of at most T frames whose valid rows sum to Kp: full utterances from the last one down (never the
    one at `skip`), then one partial, the rest one frame long (a score and a posterior row, but no transition)."""
    il = [1] * B
    for b in range(B - 1, -1, -1):
        if b == skip or Kp <= 0:
            continue
        n = min(Kp, T - 1)
        il[b] = n + 1
        Kp -= n
    assert Kp == 0
    return il


def _sparse(B, T, live):
    """All utterances one frame long but the ones at the places `live` (place -> length)."""
    il = [1] * B
    for b, n in live.items():
        il[b] = n
    return il


@functools.lru_cache(maxsize=None)
def contraction_cases():
    c = []
    # fp32 bwd_gemm_mfma<1> whole: N <= 1024 and B T < 512
    c += [Case("mfma-whole-N65", "mfma-whole", 5, 4, 65, 2, fwd="fwd_mid_kernel", gin_in_training=False, serial=True),
          Case("mfma-whole-N128", "mfma-whole", 5, 4, 128, 1, fwd="fwd_mid_kernel"),
          Case("mfma-whole-N129", "mfma-whole", 6, 3, 129, 1, fwd="fwd_mid_kernel"),
          Case("mfma-whole-N1024", "mfma-whole", 4, 5, 1024, 3, il=[4, 3, 2, 4, 3], seed=1024, fwd="fwd_cluster_kernel"),
          Case("mfma-whole-BT511-N65", "mfma-whole", 7, 73, 65, 1, shared_target=True, gin_in_training=False)]
    # fp32 sliced + gemm_combine_kernel: N <= 1024 and B T >= 512
    c += [Case("mfma-sliced-BT512-N65", "mfma-sliced", 8, 64, 65, 1, shared_target=True, gin_in_training=False, serial=True),
          Case("mfma-2-slices-BT767-N129", "mfma-sliced", 13, 59, 129, 1, shared_target=True),
          Case("mfma-3-slices-BT768-N129", "mfma-sliced", 12, 64, 129, 1, shared_target=True),
          Case("mfma-sliced-BT520-N257", "mfma-sliced", 8, 65, 257, 2, shared_target=True),
          Case("mfma-sliced-rows-in-first-slice-N130", "mfma-sliced", 8, 64, 130, 1, il=[1 + b % 4 for b in range(64)],
               shared_target=True),
          Case("mfma-sliced-one-row-in-second-slice-N131", "mfma-sliced", 8, 64, 131, 1, il=spread(257, 64, 8, skip=31),
               shared_target=True),
          Case("mfma-sliced-N1024", "mfma-sliced", 8, 64, 1024, 3, il=_sparse(64, 8, {0: 8, 31: 5, 32: 2, 63: 8}))]
    # fp64 bwd_gemm_kernel<R, 1>: rows in place (no compaction), padding rows must contribute zero
    c += [Case("f64-sliced-BT512-N128", "f64-sliced", 8, 64, 128, 1, f64=True, shared_target=True, serial=True),
          Case("f64-sliced-BT520-N128", "f64-sliced", 8, 65, 128, 1, f64=True, shared_target=True),
          Case("f64-sliced-BT512-N1100", "f64-sliced", 8, 64, 1100, 3, f64=True, il=_sparse(64, 8, {0: 8, 31: 3, 32: 6, 63: 8})),
          Case("f64-sliced-BT520-N1100", "f64-sliced", 8, 65, 1100, 3, f64=True, il=_sparse(65, 8, {1: 7, 33: 2, 34: 8, 64: 8})),
          # (gemm_slices' `tiles >= 512` edge, N = 2816 | 2817 in fp64, needs B T >= 512 there: 8 s of oracle a case -- not here)
          Case("f64-whole-BT511-N128", "f64-whole", 7, 73, 128, 1, f64=True, shared_target=True)]
    # N = 1024 | 1025 on the same kind of inputs: the fp32 matrix instruction | the bf16x3 planes
    c += [Case("bf3-N1025", "bf3-whole-sliced", 4, 5, 1025, 3, il=[4, 3, 2, 4, 3], seed=1024, fwd="fwd_cluster_kernel", serial=True),
          Case("bf3-N1281", "bf3-whole-sliced", 4, 5, 1281, 3),
          # (K' = 18: a valid row in the second of its four slices -- the last alphabet whose shape may grow, see the CPU file)
          Case("bf3-Nt8-N2048", "bf3-whole-sliced", 10, 3, 2048, 3, il=[2, 10, 9], seed=2048),
          Case("bf3-Nt9-N2049", "bf3-whole-sliced", 4, 3, 2049, 3, seed=2048),
          Case("bf3-2-slices-N2816", "bf3-whole-sliced", 3, 3, 2816, 2, il=[2, 3, 3], seed=2816),
          Case("bf3-3-slices-N2817", "bf3-whole-sliced", 3, 3, 2817, 2, il=[2, 3, 3], seed=2816)]
    c += [Case("bf3-round-N3584", "bf3-round-unsliced", 3, 3, 3584, 2, il=[2, 3, 2], serial=True),
          Case("bf3-round-N4096", "bf3-round-unsliced", 3, 3, 4096, 2, il=[2, 2, 3])]
    c += [Case("bf3-15-blocks-N4097", "bf3-rounds", 3, 3, 4097, 2, il=[2, 3, 2], serial=True)]
    c += [Case("bf3-tail-N5121", "bf3-main+tail", 2, 3, 5121, 2, il=[2, 2, 2], serial=True)]
    return tuple(c)


DEEP_T, DEEP_B = 60, 6          # frames-deep-N1100: K' = 354, six slices of four 16-row stages each
FRAME_AXIS_N = (1100, 4100)
FRAME_AXIS_KP = {1100: (0, 1, 2, 15, 16, 17, 31, 32, 33, 81), 4100: (0, 1)}


@functools.lru_cache(maxsize=None)
def frame_axis_cases():
    """The frame axis of the bf16x3 route: gemm3_pack_kernel packs blocks of 32 rows, bwd_gemm_bf3_kernel walks stages of 16, and
    the number of valid rows K' is known on the device only."""
    c = []
    for N in FRAME_AXIS_N:
        big = N > 2048
        T, B, L = (3, 3, 2) if big else (14, 5, 3)
        for Kp in FRAME_AXIS_KP[N]:
            if Kp > (B - 1) * (T - 1):
                T = Kp // (B - 1) + 2
            c.append(Case("frames-K%d-N%d" % (Kp, N), "frames", T, B, N, L, il=spread(Kp, B, T, skip=B // 2 - 1),
                          seed=N + Kp, serial=(Kp == 0)))
        if not big:
            # the steady state of bwd_gemm_bf3_kernel: more than two stages a workgroup (transfers issued inside the loop, the
            # vmcnt(ND) wait) and more than three (the ring of three stages reused)
            c.append(Case("frames-deep-N%d" % N, "frames", DEEP_T, DEEP_B, N, L, il=[DEEP_T] * DEEP_B, seed=N + 200))
        # utterances of one frame (a posterior row, no transition) between ordinary ones, and an infeasible utterance (tl > il)
        if big:
            c.append(Case("frames-mixed-N%d" % N, "frames", 3, 4, N, 3, il=[3, 1, 1, 2], infeasible=(3,), seed=N + 100))
        else:
            c.append(Case("frames-mixed-N%d" % N, "frames", 9, 6, N, 3, il=[7, 1, 9, 1, 2, 5], infeasible=(4,), seed=N + 100))
    return tuple(c)


@functools.lru_cache(maxsize=None)
def forward_cases():
    """One or two cases per producer of the stored states that bwd_post_kernel turns into grad_inputs (the shapes
    tests/test_hip_parity.py chose for these routes, T cut to at most 8)."""
    c = [Case("mid-N256", None, 8, 4, 256, 2, fwd="fwd_mid_kernel"),
         Case("mid-f64-N128", None, 8, 3, 128, 1, f64=True, fwd="fwd_mid_kernel<double>"),
         Case("cluster-N257-B3", None, 8, 3, 257, 2, fwd="fwd_cluster_kernel"),
         Case("cluster-N300-B3", None, 8, 3, 300, 3, fwd="fwd_cluster_kernel"),
         Case("cluster-N700-B20", None, 6, 20, 700, 4, fwd="fwd_cluster_kernel"),
         Case("cluster-N1024-B70", None, 3, 70, 1024, 3, il=[2 + (b % 7 == 0) for b in range(70)], fwd="fwd_cluster_kernel"),
         Case("cluster-N2048-B2", None, 5, 2, 2048, 3, fwd="fwd_cluster_kernel"),
         Case("cluster-f64-N512", None, 8, 3, 512, 3, f64=True, fwd="fwd_cluster_kernel<double>"),
         Case("tile-f64-N1030-B5", None, 6, 5, 1030, 4, f64=True, fwd="fwd_step_tile_kernel<double, 1>"),
         Case("tile-f64-N2048-B18", None, 3, 18, 2048, 3, f64=True, il=_sparse(18, 3, {0: 3, 7: 2, 15: 3, 16: 3, 17: 2}),
              fwd="fwd_step_tile_kernel<double, 2>"),
         Case("step-N2049-B3", None, 4, 3, 2049, 3, seed=2048, fwd="fwd_step_mfma (half tile)"),
         Case("step-N2049-B17", None, 4, 17, 2049, 3, il=_sparse(17, 4, {0: 4, 8: 3, 15: 2, 16: 4}), fwd="fwd_step_mfma"),
         Case("step-N2049-B40", None, 4, 40, 2049, 3, il=_sparse(40, 4, {0: 3, 31: 4, 32: 4, 39: 2}), fwd="fwd_step_mfma"),
         Case("step-N2049-B64", None, 3, 64, 2049, 3, il=_sparse(64, 3, {0: 3, 31: 2, 32: 3, 63: 3}), fwd="fwd_step_mfma"),
         Case("step-bf3-N2049-B70", None, 3, 70, 2049, 3, il=_sparse(70, 3, {0: 3, 31: 2, 32: 3, 63: 2, 64: 3, 69: 3}),
              fwd="fwd_step_bf3"),
         Case("step-bf3-N1300-B70", None, 5, 70, 1300, 3, il=_sparse(70, 5, {0: 5, 31: 4, 32: 5, 63: 3, 64: 5, 69: 4}),
              fwd="fwd_step_bf3"),
         Case("step-tail-chunk-N4111", None, 3, 3, 4111, 2, il=[2, 3, 3], fwd="fwd_step_mfma"),
         Case("step-f64-N2100", None, 4, 3, 2100, 3, f64=True, seed=2100, fwd="fwd_step_kernel<double>")]
    for mb in (2, 3, 4, 5):
        c.append(Case("step-N2100-%d-row-blocks" % mb, None, 4, 3, 2100, 3, seed=2100, env={"ASG_STEP_ROW_BLOCKS": mb},
                      fwd="fwd_step_mfma"))
    return tuple(c)


def all_cases():
    return contraction_cases() + frame_axis_cases() + forward_cases()


# ---- the fp64 reference ---------------------------------------------------------------------------------------------------------
_REF = {}


def reference(case):
    """oracle/asg_oracle.py under the case's weights, once per process and per set of inputs (the cases that differ in a
    library switch only share theirs).  The arrays are read-only."""
    key = (case.T, case.B, case.N, case.L, tuple(case.il.tolist()), tuple(case.tl.tolist()), case.tg.numpy().tobytes(),
           float(case.x[0, 0, 0]), float(case.tr[0, 0]))
    if key not in _REF:
        o = orc.asg_loss(case.x.double().numpy(), case.tg.numpy(), case.tr.double().numpy(), case.il.numpy(), case.tl.numpy(),
                         "none", grad_out=case.w.numpy())
        o = {k: o[k] for k in ("loss", "full_scores", "grad_inputs", "grad_transition", "grad_inputs_full", "grad_inputs_aligned",
                               "grad_transition_full", "grad_transition_aligned")}
        for v in o.values():
            v.setflags(write=False)
        _REF[key] = o
    return _REF[key]


def training_cells(o):
    """Where the training call's combined tensors ARE the full-lattice part: every cell whose aligned part is exactly zero.
    -> (mask of grad_transition, mask of grad_inputs)."""
    return o["grad_transition_aligned"] == 0, o["grad_inputs_aligned"] == 0


def excluded_share(case, o):
    """-> (share of grad_transition's cells, largest share of the labels of a grad_inputs row) left to the old rule."""
    mt, mi = training_cells(o)
    worst = 0.0
    for b in range(case.B):
        n = int(case.il[b])
        if n:
            worst = max(worst, float((~mi[:n, b]).sum(axis=1).max()) / case.N)
    return float((~mt).sum()) / mt.size, worst


def last_row_posterior(case):
    """What the LAST valid frame row (the last frame of the last utterance that has two) adds to the full part of grad_transition:
    w_b exp(alpha[t-1][j] + transition[i][j] + x[t][i] + beta[t][i] - score_b), from the oracle's alpha and beta."""
    x, tr = case.x.double().numpy(), case.tr.double().numpy()
    sc, al, be = orc.full_forward(x, tr, case.il.numpy())
    b = max(b for b in range(case.B) if int(case.il[b]) >= 2)
    t = int(case.il[b]) - 1
    return float(case.w[b]) * np.exp(al[t - 1, b][None, :] + tr + (x[t, b] + be[t, b])[:, None] - sc[b]), b, t
