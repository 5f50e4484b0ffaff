"""Test-only helpers shared by tests/test_hip_viterbi_regimes.py (GPU) and tests/test_viterbi_regimes_cpu.py: the launch
arithmetic of the two tropical-semiring kernels restated in Python -- `launch_viterbi_small` (csrc/asg_viterbi.hip, DESIGN.md
5d.1) and `launch_decode` (csrc/asg_decode.hip, 5f.1) -- so that a case can assert the regime it names, and the inputs of the
cases with their numpy results (tests/viterbi_ref.py, tests/decode_ref.py), computed once per process.  Nothing here needs a GPU.

Every array is numpy; draws are seeded per case.  "Integer" inputs (emissions in {-2..2}, transitions in {-1, 0, 1}) tie all the
time; "peaked" emissions add +20 to one chosen label per frame, so the decoded path is that schedule.
"""
import collections
import functools

import numpy as np

from decode_ref import decode_ref
from viterbi_ref import viterbi_ref

DTYPES = ("float32", "float64")

# ---- csrc/asg_viterbi.hip, restated (tests/test_viterbi_regimes_cpu.py matches the constants to the source) ----------------
K_VPF = 16                       # emission prefetch depth of the one-wavefront aligner
WIDE_PF = {1: 8, 4: 2, 8: 2}     # ... and of viterbi_wide_kernel<R, KP>
BT = 64                          # both kernels backtrace in blocks of 64 frames; a mask word is 64 positions
ALIGN_MAX_S = 8192

Align = collections.namedtuple("Align", "kind KP threads nw PF")


def align_kernel(S):
    """What launch_viterbi_small launches for S target positions (after viterbi_align has cut S to T)."""
    assert 1 <= S <= ALIGN_MAX_S
    nw = (S + 63) // 64
    if S <= 64:
        return Align("small", 1, 64, nw, K_VPF)
    if S <= 1024:
        return Align("wide", 1, nw * 64, nw, WIDE_PF[1])
    KP = 4 if S <= 4096 else 8
    return Align("wide", KP, 1024, nw, WIDE_PF[KP])


def align_work_bytes(T, B, S):
    return B * T * ((S + 63) // 64) * 8


# ---- csrc/asg_decode.hip, restated -------------------------------------------------------------------------------------------
K_EPF = 8                        # emission prefetch depth of the resident decoder
Resident = collections.namedtuple("Resident", "NP KS KEEP threads")
Streaming = collections.namedtuple("Streaming", "PAD nrt UB ngr nblk")


def decode_route(elem, N, B):
    """What launch_decode runs for an alphabet of N labels, B utterances and elements of `elem` bytes."""
    if N <= (128 if elem == 8 else 256):
        if N <= 64:
            NP, KS = (N + 7) // 8 * 8, 1
        else:
            NP, KS = 64, (2 if N <= 128 else 4)
        return Resident(NP, KS, KS == 1 and elem * NP <= 256, 64 * KS * KS)
    PAD = (N + 63) // 64 * 64
    nrt = PAD // 64
    UB = 8 if elem == 8 else (4 if B <= 4 else (8 if B <= 8 else 16))
    ngr = (B + UB - 1) // UB
    return Streaming(PAD, nrt, UB, ngr, (nrt + 7) // 8 * 8 * ngr)


def elem_of(dtype):
    return np.dtype(dtype).itemsize


# ---- draws -------------------------------------------------------------------------------------------------------------------
def _random(rng, T, B, N, dtype):
    return rng.normal(size=(T, B, N)).astype(dtype), rng.normal(size=(N, N)).astype(dtype)


def _integer(rng, T, B, N, dtype):
    return rng.integers(-2, 3, size=(T, B, N)).astype(dtype), rng.integers(-1, 2, size=(N, N)).astype(dtype)


def _targets(rng, B, S, N):
    """Targets whose neighbours differ.  Two equal neighbours emit the same label with the same transition whether the path
    stays or moves on, so they tie EXACTLY even under continuous emissions; only the tie cases are meant to depend on the rule."""
    steps = rng.integers(1, N, size=(B, S))
    steps[:, 0] = rng.integers(0, N, size=B)
    return np.cumsum(steps, axis=1) % N


class AlignCase:
    """One call of viterbi_align: x [T,B,N], tr [N,N], tg [B,S] int64, il, tl [B] int64.  S > T is cut to T by viterbi_align (as
    by ASGLoss.forward): `kernel` and `ref()` are those of the cut targets."""

    def __init__(self, name, x, tr, tg, il, tl):
        self.name, self.x, self.tr, self.tg = name, x, tr, np.asarray(tg, np.int64)
        self.T, self.B, self.N = x.shape
        self.S = self.tg.shape[1]
        self.il = np.full(self.B, self.T, np.int64) if il is None else np.asarray(il, np.int64)
        self.tl = np.full(self.B, self.S, np.int64) if tl is None else np.asarray(tl, np.int64)
        assert self.B <= 16 and self.N <= 8
        self.kernel = align_kernel(min(self.S, self.T))
        self._ref = None

    def ref(self):
        """(scores [B], positions [B,T]) of the restatement; computed once, never written to."""
        if self._ref is None:
            self._ref = viterbi_ref(self.x, self.tg[:, :self.T], self.tr, self.il, np.minimum(self.tl, self.T))
            for a in self._ref:
                a.setflags(write=False)
        return self._ref

    def __repr__(self):
        return self.name


class DecodeCase:
    """One call of viterbi_decode: x [T,B,N], tr [N,N], il [B] int64; schedule [B,T] for peaked emissions (else None)."""

    def __init__(self, name, x, tr, il, schedule=None):
        self.name, self.x, self.tr, self.schedule = name, x, tr, schedule
        self.T, self.B, self.N = x.shape
        self.il = np.asarray(il, np.int64)
        self.route = decode_route(elem_of(x.dtype), self.N, self.B)
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = decode_ref(self.x, self.tr, self.il)
            for a in self._ref:
                a.setflags(write=False)
        return self._ref

    def __repr__(self):
        return self.name


def _seed(*parts):
    """A seed from the case's own numbers (no hash(): stable across processes)."""
    s = 12345
    for p in parts:
        s = (s * 1000003 + (sum(map(ord, p)) if isinstance(p, str) else int(p))) % (1 << 31)
    return s


# ---- aligner cases -----------------------------------------------------------------------------------------------------------
ALIGN_N = 5
# S: the one-wavefront kernel | one position per thread (64 .. 1024 threads) | four | eight
KERNEL_S = (1, 63, 64, 65, 128, 129, 1023, 1024, 1025, 1088, 4095, 4096, 4097, 8191, 8192)
SINGLE_S = (64, 65, 1025, 4097)          # T = S: every utterance of full target length has ONE alignment
TIE_TS = ((70, 64), (130, 65), (1100, 1024), (1100, 1025), (4200, 4097), (8300, 8192))
# float32 sums of several thousand round to equal values now and then: draws in which no comparison on or next to the best path
# ties, so that only the tie cases depend on the tie rule (asserted by the CPU module)
KERNEL_SALT = {(8192, "float32", False): 1, (4097, "float32", True): 1}
TIE_SALT = {(64, "float32"): 1, (64, "float64"): 1}          # draws in which both utterances tell the tie rules apart (CPU module)
CHUNK_TS = ((130, 30), (130, 200), (1600, 1500))
RING_SHORT = (1, 2, 3, 9, 10)
INF_S = (300, 1500)
HOST_S = (30, 300)                        # strides, capture, 16-bit emissions: the one-wavefront kernel and the wide one


def strip_edge(S, dtype):
    """A target length on a strip edge: 64 k in float64, 64 k + 1 in float32 (k near the middle of the target: 2048 | 2049 at
    4097, where it is also the edge between two positions of one thread); S < 64 has no strip edge: half of S."""
    if S < 64:
        return max(1, S // 2)
    k = max(1, S // 128)
    return min(S, 64 * k + (1 if np.dtype(dtype).itemsize == 4 else 0))


@functools.lru_cache(maxsize=None)
def kernel_case(S, dtype, single=False, salt=None):
    T, B, N = (S if single else S + 3), 3, ALIGN_N
    rng = np.random.default_rng(_seed("kernel", S, dtype, single, KERNEL_SALT.get((S, dtype, single), 0) if salt is None else salt))
    x, tr = _random(rng, T, B, N, dtype)
    tg = _targets(rng, B, S, N)
    return AlignCase("S%d%s_%s" % (S, "_single" if single else "", dtype), x, tr, tg, None, [S, 1, strip_edge(S, dtype)])


@functools.lru_cache(maxsize=None)
def align_tie_case(T, S, dtype, salt=None):
    B, N = 2, 8
    rng = np.random.default_rng(_seed("tie", T, S, dtype, TIE_SALT.get((S, dtype), 0) if salt is None else salt))
    x, tr = _integer(rng, T, B, N, dtype)
    tg = rng.integers(0, N, size=(B, S))                     # (equal neighbours included: they tie as well)
    return AlignCase("ties_T%d_S%d_%s" % (T, S, dtype), x, tr, tg, None, [S, S - 1])


def chunk_lengths(T):
    return [1, 2, 63, 64, 65, 127, 128, 129, T]


@functools.lru_cache(maxsize=None)
def chunk_case(T, S, dtype):
    """Lengths at the 64-frame backtrace blocks.  Target lengths: equal to the length (one alignment: the position IS the frame,
    so a block starts on a strip's first position), or three quarters of it (the path crosses the strips inside the blocks)."""
    il = chunk_lengths(T)
    tl = [min(S, n if k % 2 == 0 else max(1, 3 * n // 4)) for k, n in enumerate(il)]
    tl[-1] = S if S <= T else 3 * T // 4
    B, N = len(il), ALIGN_N
    rng = np.random.default_rng(_seed("chunk", T, S, dtype))
    x, tr = _random(rng, T, B, N, dtype)
    tg = _targets(rng, B, S, N)
    return AlignCase("chunks_T%d_S%d_%s" % (T, S, dtype), x, tr, tg, il, tl)


@functools.lru_cache(maxsize=None)
def ring_case(S, dtype, half=0):
    """Utterances shorter than, equal to and just above the prefetch depth: S = 20 (depth 16), lengths 1 .. 18 in two batches of
    nine; S = 300 (depth 8) and 1025 (depth 2), lengths {1, 2, 3, 9, 10}."""
    il = list(range(1 + 9 * half, 10 + 9 * half)) if S == 20 else list(RING_SHORT)
    T, B, N = S + 3, len(il), ALIGN_N
    rng = np.random.default_rng(_seed("ring", S, dtype, half))
    x, tr = _random(rng, T, B, N, dtype)
    tg = _targets(rng, B, S, N)
    tl = [int(rng.integers(1, n + 1)) for n in il]
    tl[-1] = min(il[-1], S)
    return AlignCase("ring_S%d_%d_%s" % (S, half, dtype), x, tr, tg, il, tl)


@functools.lru_cache(maxsize=None)
def inf_case(S, dtype):
    """Half the emissions -inf (drawn with probability one half), then ONE random alignment per utterance made finite again, so
    that finite alignments exist and the best one has to be found among masked cells.  Utterance 3 has a fully masked frame."""
    T, B, N = 2 * S, 4, 8
    rng = np.random.default_rng(_seed("inf", S, dtype))
    x, tr = _random(rng, T, B, N, dtype)
    tg = _targets(rng, B, S, N)
    il = np.array([T, T - 7, S + 1, T])
    tl = np.array([S, S // 2, S, S // 3])
    masked = rng.random(size=x.shape) < 0.5
    for b in range(B):
        adv = np.zeros(il[b], bool)
        adv[rng.choice(np.arange(1, il[b]), size=tl[b] - 1, replace=False)] = True
        safe = np.cumsum(adv)                                                     # a monotone alignment 0 .. tl - 1
        masked[np.arange(il[b]), b, tg[b, safe]] = False
    x[masked] = -np.inf
    x[T // 2, 3, :] = -np.inf
    return AlignCase("inf_S%d_%s" % (S, dtype), x, tr, tg, il, tl)


@functools.lru_cache(maxsize=None)
def host_case(S, dtype, seed=0):
    """A small batch for the host-side cases (strides, capture, 16-bit emissions)."""
    T, B, N = S + 40, 4, 8
    rng = np.random.default_rng(_seed("host", S, dtype, seed))
    x, tr = _random(rng, T, B, N, dtype)
    tg = _targets(rng, B, S, N)
    il = np.array([T, T - 1, 1, int(rng.integers(S, T))])
    tl = np.array([S, int(rng.integers(1, S + 1)), 1, S])
    return AlignCase("host_S%d_%d_%s" % (S, seed, dtype), x, tr, tg, il, tl)


# ---- decoder cases -----------------------------------------------------------------------------------------------------------
# both sides of every one-wavefront instantiation, of KEEP in float64 (32 | 33), of the slice counts and of the route switches
INSTANCE_N = (8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 64, 65, 128, 129, 256, 257)
SLICE_TIE_N = {"float32": (100, 129, 256), "float64": (100, 128)}
BLOCK_N = (40, 100, 200, 300)
BLOCK_LENGTHS = (1, 2, 7, 8, 9, 10, 63, 64, 65, 127, 128, 129, 130)
STREAM_N = (257, 520)
STREAM_B = {"float32": (4, 5, 8, 9, 16, 17), "float64": (8, 9)}
PEAK = 20.0


@functools.lru_cache(maxsize=None)
def instance_case(N, dtype, integer):
    T, B = 70, 4
    rng = np.random.default_rng(_seed("instance", N, dtype, integer))
    x, tr = (_integer if integer else _random)(rng, T, B, N, dtype)
    return DecodeCase("N%d_%s_%s" % (N, "int" if integer else "rand", dtype), x, tr, [T, 0, 1, 64])


@functools.lru_cache(maxsize=None)
def slice_tie_case(N, dtype):
    T, B = 60, 4
    rng = np.random.default_rng(_seed("slices", N, dtype))
    x, tr = _integer(rng, T, B, N, dtype)
    return DecodeCase("slice_ties_N%d_%s" % (N, dtype), x, tr, [T, T - 1, 33, 2])


def _schedule(rng, T, N, change_at):
    """Labels of T frames in runs of 1 .. 6 frames, neighbouring runs of different labels.  change_at: the runs are cut so that a
    new run starts exactly at frames 64 and 128; otherwise one run covers frames 61 .. 66 and another 125 .. 129."""
    starts = {0}
    t = 0
    while t < T:
        t += int(rng.integers(1, 7))
        starts.add(t)
    if change_at:
        starts |= {64, 128}
    else:
        starts = {s for s in starts if not (61 < s <= 66 or 125 < s <= 129)} | {61, 125}
    sched = np.empty(T, np.int64)
    lab = -1
    for t in range(T):
        if t in starts:
            lab = int((lab + rng.integers(1, N)) % N) if lab >= 0 else int(rng.integers(0, N))
        sched[t] = lab
    return sched


@functools.lru_cache(maxsize=None)
def block_case(N, dtype):
    """Lengths at the 64-frame backtrace and collapse blocks and around the prefetch depth.  Utterances alternate between a
    schedule that changes label exactly at frames 64 and 128 and one whose runs straddle 63 | 64 and 127 | 128."""
    T, B = 130, len(BLOCK_LENGTHS)
    rng = np.random.default_rng(_seed("blocks", N, dtype))
    x, tr = _random(rng, T, B, N, dtype)
    sched = np.stack([_schedule(rng, T, N, b % 2 == 0) for b in range(B)])
    x[np.arange(T)[:, None], np.arange(B)[None, :], sched.T] += np.dtype(dtype).type(PEAK)
    return DecodeCase("blocks_N%d_%s" % (N, dtype), x, tr, BLOCK_LENGTHS, schedule=sched)


@functools.lru_cache(maxsize=None)
def uint8_case():
    """N = 256, float32: every label has one favoured predecessor at or above 128 (+6 on that transition), label 255 for every
    fourth label: the back-pointers on the best path are mostly >= 128, and 255 again and again."""
    T, B, N = 70, 4, 256
    rng = np.random.default_rng(_seed("uint8"))
    x, tr = _random(rng, T, B, N, "float32")
    pred = rng.integers(128, 256, size=N)
    pred[::4] = 255
    tr[np.arange(N), pred] += np.float32(6)
    return DecodeCase("uint8_N256_float32", x, tr, [T, T - 1, 64, 65])


@functools.lru_cache(maxsize=None)
def stream_case(N, B, dtype):
    T = 6
    rng = np.random.default_rng(_seed("stream", N, B, dtype))
    x, tr = _random(rng, T, B, N, dtype)
    il = rng.integers(0, T + 1, size=B)
    il[0], il[B - 1] = T, T
    return DecodeCase("stream_N%d_B%d_%s" % (N, B, dtype), x, tr, il)


def last_index_argmax(a):
    """The wrong tie rule of the decoder's bite checks: the LAST index of the max."""
    return len(a) - 1 - int(np.argmax(a[::-1]))
