"""Test-only helpers shared by tests/test_hip_fused_regimes.py (GPU) and tests/test_fused_regimes_cpu.py: the inputs and the cached
fp64 references of the cases that put the fused training step (csrc/asg_fused.hip) at the lengths, alphabets,
paddings and batch sizes where its kernels change shape, plus the kernel's own shape rules restated so that a case can assert
the regime it names.  Nothing here needs a GPU; the two readers of device memory at the end take what a GPU test hands them.

Draws are seeded and util.synth-style: transitions `rand`, emissions `randn`, targets `randint`, and target_lengths <=
input_lengths unless a case says "infeasible".  Cases whose utterances must keep their bits when the batch around them changes
(padding, neighbours, mixed) draw every utterance from its own seed and fill the frames behind its length with other draws.
"""
import functools

import numpy as np
import torch

from oracle import asg_oracle as orc

# ---- csrc/asg_fused.hip, csrc/asg_chains.h and csrc/asg_api.hip, restated (tests/test_fused_regimes_cpu.py matches them to the source)
K_MIN_FUSED, K_GS, K_FR, K_AR, K_MAX_BLK, K_CH, K_QB, K_BWD_SLICE = 4, 8, 64, 64, 128, 8, 4, 64
K_PF, K_RENORM = 16, 4
T_MAX = 4000
NP_EDGES = (8, 16, 24, 32, 40, 48, 56)        # launch_fused: N <= edge -> fused kernels of NP = edge; above the last one NP = 64
ROW_PASS_STRIDE = 4 * K_CH * K_QB             # quads one outer iteration of the row pass takes per utterance
RANGE_BITS = 100                              # row sums and normalisers outside [2^-100, 2^100] flag the utterance


def crossing(n):
    """Where the alpha and the beta chain of an utterance of n frames cross (asg_fused.hip: crossing)."""
    mid = n // 2
    if n < 64:
        return mid
    base = (mid >> 3) << 3
    best, cost = mid, 99
    for r in range(1, 6):
        m = base + r
        ra = (n - m) & 7
        c = max(r, 8 if ra == 0 else ra)
        if c < cost:
            cost, best = c, m
    return best


def cross_class(n):
    mid = crossing(n)
    return mid % 8, (n - mid) % 8


def row_quads(n):
    """P2 quads of the backward launch's row pass: the alpha side's second half, then the beta side's."""
    mid = crossing(n)
    return ((n - mid + 3) >> 2) + ((mid + 3) >> 2)


def xstate_blocks(T):
    return (T + 7) // 8 + 2


def aoff_entries(T):
    return (T + K_PF - 1) // K_PF + 1


def np_of(N):
    for e in NP_EDGES:
        if N <= e:
            return e
    return 64


def consumers(NP):
    return min(3, 4 if NP <= 48 else 2)


def fused_preferred(B, cus):
    """HipBackend.fused_preferred: utterances 2x, 2x + 1 sit on XCD x mod 8 and the fullest XCD must hold its workgroups."""
    pairs = (B + 1) // 2
    return ((pairs + 7) // 8) * 2 * 3 <= cus // 8


def fused_edge(cus):
    """The largest batch the fused launch takes on a device of `cus` compute units (80 on 256)."""
    B = 1
    while fused_preferred(B + 1, cus):
        B += 1
    return B


def grid_blocks(B):
    return 48 * ((B + 15) // 16)


# ---- cases ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One call of the fused step.  x [T,B,N] float32 (bf16: already rounded to bfloat16 values), tr [N,N], tg [B,S], il, tl [B];
    w = upstream gradient ([B] for reduction 'none', None = 1); flagged / feasible [B] bool: what the kernel must report and what
    the oracle must find; fused = the route on a device whose fused edge is >= B."""

    def __init__(self, name, x, tr, tg, il, tl, reduction="none", w=None, flagged=None, feasible=None, bf16=False,
                 batch_major=False, fused=True, wide=None):
        self.name, self.x, self.tr, self.tg = name, x, tr, tg
        self.il, self.tl = torch.as_tensor(il, dtype=torch.int64), torch.as_tensor(tl, dtype=torch.int64)
        self.reduction, self.w, self.bf16, self.batch_major, self.fused = reduction, w, bf16, batch_major, fused
        self.T, self.B, self.N = x.shape
        self.S = tg.shape[1]
        B = self.B
        self.feasible = np.ones(B, bool) if feasible is None else np.asarray(feasible, bool)
        self.wide = np.zeros(B, bool) if wide is None else np.asarray(wide, bool)     # emissions far outside the fp32 window
        short = self.il.numpy() < K_MIN_FUSED
        # what flags an utterance (asg_fused.hip, header): fewer than kMinFused frames, or row sums / normalisers outside the window.
        # An infeasible target (tl > il) does not: fused_afin finds no mass (`feasible`), writes zero posteriors, the score is log-zero.
        self.flagged = (short | self.wide) if flagged is None else np.asarray(flagged, bool)
        if bf16:
            self.x = self.x.to(torch.bfloat16).to(torch.float32)
        assert self.S <= self.T and self.S <= 64 and self.N < 64
        assert bool((self.tl[torch.as_tensor(self.feasible)] <= self.il[torch.as_tensor(self.feasible)]).all())

    def __repr__(self):
        return self.name


def _draw(seed, T, B, N, S):
    g = torch.Generator().manual_seed(seed)
    tr = torch.rand(N, N, generator=g)
    x = torch.randn(T, B, N, generator=g)
    tg = torch.randint(0, N, (B, S), generator=g)
    return g, tr, x, tg


SWEEP_N = (5, 40, 50)            # three consumers; the benchmark's tile; two consumers
SWEEP_BATCHES = 21               # lengths 1 .. 336 in batches of 16 consecutive lengths


@functools.lru_cache(maxsize=None)
def sweep_case(N, k, bf16=False, batch_major=False):
    """Batch k of the length sweep: lengths 16 k + 1 .. 16 k + 16 (T = the largest), L = 7, reduction 'none' under the weights
    linspace(-0.5, 1.5, 16) with exactly 1.0 at utterance k % 16 and exactly 0.0 at utterance (k + 5) % 16."""
    B, L = 16, 7
    il = torch.arange(16 * k + 1, 16 * k + 17)
    T = int(il[-1])
    g, tr, x, tg = _draw(7000 + 100 * N + k, T, B, N, L)
    tl = torch.minimum(torch.randint(1, L + 1, (B,), generator=g), il)
    w = torch.linspace(-0.5, 1.5, B)
    w[k % 16], w[(k + 5) % 16] = 1.0, 0.0
    return Case("sweep-N%d-len%d..%d%s%s" % (N, int(il[0]), T, "-bf16" if bf16 else "", "-bmajor" if batch_major else ""),
                x, tr, tg, il, tl, "none", w, bf16=bf16, batch_major=batch_major)


@functools.lru_cache(maxsize=None)
def rowpass_case():
    """nq on both sides of 128: the row pass's outer loop takes a second iteration from nq = 129."""
    B, N, L = 32, 5, 3
    il = torch.arange(496, 528)
    g, tr, x, tg = _draw(7101, 527, B, N, L)
    return Case("rowpass-len496..527", x, tr, tg, il, torch.randint(1, L + 1, (B,), generator=g), "sum")


NP_ALPHABETS = (1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 63)


@functools.lru_cache(maxsize=None)
def np_case(N):
    """Every alphabet tile past the rings: second halves of 30..38 frames (no wrap) and of 65..73 (one wrap of kFR / kAR)."""
    B = 32
    S = 5 if N == 1 else min(N, 9)
    il = torch.cat([torch.arange(60, 76), torch.arange(130, 146)])
    g, tr, x, tg = _draw(7200 + N, 145, B, N, S)
    tl = torch.randint(1, S + 1, (B,), generator=g)
    return Case("np-N%d" % N, x, tr, tg, il, tl, ("mean", "sum", "none")[N % 3],
                torch.linspace(0.25, 1.75, B) if N % 3 == 2 else None)


# -- utterances that keep their own draws wherever they stand
def _utterance(seed, n, N, S, tl, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(n, N, generator=g), torch.randint(0, N, (S,), generator=g), n, tl


def _batch(name, utts, T, N, S, seed, **kw):
    """Utterances side by side at time extent T; frames behind each length hold draws of the batch's own seed (nobody may read them)."""
    g = torch.Generator().manual_seed(seed)
    B = len(utts)
    x = torch.randn(T, B, N, generator=g)
    tg = torch.empty(B, S, dtype=torch.int64)
    for b, (xu, tu, n, _) in enumerate(utts):
        x[:n, b] = xu
        tg[b] = tu
    return Case(name, x, _transition(N), tg, [u[2] for u in utts], [u[3] for u in utts], **kw)


@functools.lru_cache(maxsize=None)
def _transition(N):
    return torch.rand(N, N, generator=torch.Generator().manual_seed(7300 + N))


PAD_LENGTHS = (4, 9, 31, 64, 65, 100, 129, 130)
PAD_TARGETS = (1, 2, 31, 64, 33, 64, 1, 50)
PAD_T = tuple(range(130, 147))       # T % 16 in all sixteen classes (and T % 8 in all eight, twice)
PAD_N, PAD_S = 11, 64


@functools.lru_cache(maxsize=None)
def pad_utterances():
    return tuple(_utterance(7400 + i, n, PAD_N, PAD_S, tl) for i, (n, tl) in enumerate(zip(PAD_LENGTHS, PAD_TARGETS)))


@functools.lru_cache(maxsize=None)
def other_utterances():
    return tuple(_utterance(7450 + i, n, PAD_N, PAD_S, tl)
                 for i, (n, tl) in enumerate(zip((130, 5, 77, 128, 63, 97, 16, 111), (64, 3, 20, 1, 63, 40, 16, 7))))


@functools.lru_cache(maxsize=None)
def pad_case(T, bf16=False, reduction="none"):
    return _batch("pad-T%d%s-%s" % (T, "-bf16" if bf16 else "", reduction), pad_utterances(), T, PAD_N, PAD_S, 7500 + T,
                  reduction=reduction, bf16=bf16)


NEIGHBOUR_ORDER = (5, 2, 7, 0, 3, 6, 1, 4)


@functools.lru_cache(maxsize=None)
def neighbour_case(kind, reduction="none"):
    """-> (case, where): where[i] = the place of pad utterance i in the batch."""
    u, o = pad_utterances(), other_utterances()
    if kind == "reordered":
        utts, where = [u[i] for i in NEIGHBOUR_ORDER], [NEIGHBOUR_ORDER.index(i) for i in range(8)]
    elif kind == "interleaved":
        utts, where = [v for pair in zip(o, u) for v in pair], [2 * i + 1 for i in range(8)]
    else:                                   # "alone-<i>"
        i = int(kind.split("-")[1])
        utts, where = [u[i]], {i: 0}
    return _batch("neighbours-%s-%s" % (kind, reduction), utts, 130, PAD_N, PAD_S, 7600, reduction=reduction), where


BATCH_SIZES = (1, 2, 15, 16, 17, 32, 33, 79, 80)


@functools.lru_cache(maxsize=None)
def batch_case(B, fused=True):
    T, N, L = 72, 40, 9
    g, tr, x, tg = _draw(7700 + B, T, B, N, L)
    il = torch.randint(36, T + 1, (B,), generator=g)
    tl = torch.randint(1, L + 1, (B,), generator=g)
    red = ("mean", "sum", "none")[B % 3]
    return Case("batch-B%d" % B, x, tr, tg, il, tl, red, torch.linspace(0.5, 1.5, B) if red == "none" else None, fused=fused)


@functools.lru_cache(maxsize=None)
def top_case(T):
    """The longest utterance the fused launch takes (kMaxBlk blocks of 16 indices per half) and the first it does not."""
    B, N, S = 2, 7, 64
    g, tr, x, tg = _draw(7800 + T, T, B, N, S)
    return Case("top-T%d" % T, x, tr, tg, [T, T - 1], [64, 17], "sum", fused=T <= T_MAX)


TARGET_KINDS = ("S1", "S2", "S63", "S64", "tight", "one-label", "padded-with-a-used-label")


@functools.lru_cache(maxsize=None)
def target_case(kind):
    N = 13
    if kind in ("S1", "S2", "S63", "S64"):
        S, B, T = int(kind[1:]), 8, 90
        g, tr, x, tg = _draw(7900 + S, T, B, N, S)
        tl = torch.tensor(sorted({1, S} | {max(1, (S * i) // 7) for i in range(1, 7)}) + [S] * 8)[:B]
        il = torch.maximum(torch.randint(40, T + 1, (B,), generator=g), tl)
        return Case("targets-" + kind, x, tr, tg, il, tl, "none", torch.linspace(0.5, 1.5, B))
    if kind == "tight":                    # tl == il: one alignment, every aligned posterior 1
        il = torch.tensor([64, 37, 5, 4, 63, 8])
        g, tr, x, tg = _draw(7910, 64, 6, N, 64)
        return Case("targets-tight", x, tr, tg, il, il.clone(), "sum")
    S, B, T = 64, 6, 100
    g, tr, x, tg = _draw(7920 + len(kind), T, B, N, S)
    il = torch.tensor([100, 64, 65, 99, 70, 81])
    if kind == "one-label":                # the scatter adds 64 positions into one LDS word
        tg = torch.full((B, S), 3, dtype=torch.int64)
        tg[1] = 0
        tg[2] = N - 1
        return Case("targets-one-label", x, tr, tg, il, [64, 64, 64, 63, 33, 2], "mean")
    tl = torch.tensor([1, 2, 31, 32, 33, 63])
    for b in range(B):                     # behind tl: a label the utterance's target also uses -- P2 must be exact zeros there
        tg[b, int(tl[b]):] = tg[b, 0]
    return Case("targets-padded-with-a-used-label", x, tr, tg, il, tl, "none", torch.linspace(1.5, 0.5, B))


MIXED_ORDINARY = (0, 2, 5, 7, 9)       # places of the ordinary utterances in the mixed batch (pad utterances 3, 5, 2, 7, 1)
MIXED_PAD = (3, 5, 2, 7, 1)


@functools.lru_cache(maxsize=None)
def mixed_case(bf16=False):
    """Ordinary utterances beside lengths 1, 2, 3, an infeasible one (tl > il), one with a -inf label and one with emissions
    40 * randn.  Weight exactly 1.0 on the flagged utterance of length 2 and 0.37 on the one of length 3."""
    u = pad_utterances()
    N, S = PAD_N, PAD_S
    neg = _utterance(7951, 90, N, S, 12)
    neg[0][:, N - 1] = float("-inf")                      # a masked label ...
    neg = (neg[0], neg[1].clamp(max=N - 2), 90, 12)       # ... that the target does not use
    utts = [u[3], _utterance(7952, 1, N, S, 1), u[5], _utterance(7953, 2, N, S, 2), _utterance(7954, 3, N, S, 1), u[2],
            _utterance(7955, 20, N, S, 21), u[7], neg, u[1], _utterance(7956, 70, N, S, 9, scale=40.0)]
    B = len(utts)
    feasible = np.ones(B, bool)
    feasible[6] = False
    wide = np.zeros(B, bool)
    wide[10] = True
    w = torch.linspace(0.6, 1.4, B)
    w[3], w[4], w[1] = 1.0, 0.37, 0.0
    return _batch("mixed%s" % ("-bf16" if bf16 else ""), utts, 130, N, S, 7950, reduction="none", w=w, feasible=feasible, wide=wide,
                  bf16=bf16)


@functools.lru_cache(maxsize=None)
def mixed_plain_case(bf16=False):
    """The ordinary utterances of the mixed batch by themselves, under the weights they have there."""
    u, m = pad_utterances(), mixed_case(bf16)
    return _batch("mixed-plain%s" % ("-bf16" if bf16 else ""), [u[i] for i in MIXED_PAD], 130, PAD_N, PAD_S, 7960, reduction="none",
                  w=m.w[list(MIXED_ORDINARY)].clone(), bf16=bf16)


def all_cases():
    """Every case of tests/test_hip_fused_regimes.py on a device whose fused edge is 80 (B = 81 is built there from that edge)."""
    out = [sweep_case(N, k) for N in SWEEP_N for k in range(SWEEP_BATCHES)]
    out += [rowpass_case()] + [np_case(N) for N in NP_ALPHABETS] + [pad_case(T) for T in PAD_T]
    out += [neighbour_case(k)[0] for k in ("reordered", "interleaved")] + [neighbour_case("alone-%d" % i)[0] for i in range(8)]
    out += [neighbour_case("interleaved", "mean")[0]]
    out += [batch_case(B) for B in BATCH_SIZES] + [batch_case(81, fused=False)]
    out += [top_case(T_MAX), top_case(T_MAX + 1)] + [target_case(k) for k in TARGET_KINDS] + [mixed_case(), mixed_plain_case()]
    out += [sweep_case(40, 9, batch_major=True)]
    out += [sweep_case(40, k, bf16=True) for k in range(SWEEP_BATCHES)] + [pad_case(T, bf16=True) for T in PAD_T]
    out += [mixed_case(bf16=True), mixed_plain_case(bf16=True)]
    return out


# ---- the fp64 reference ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(case):
    """oracle/asg_oracle.py on the case's values (bf16 cases: the bf16-representable ones), computed once per process."""
    w = None if case.w is None else case.w.double().numpy()
    o = orc.asg_loss(case.x.double().numpy(), case.tg.numpy(), case.tr.double().numpy(), case.il.numpy(), case.tl.numpy(),
                     case.reduction, grad_out=w)
    return {k: o[k] for k in ("loss", "loss_per_utt", "grad_inputs", "grad_transition")}


def _lse(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m, axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def range_bits(case):
    """How far, in bits and per utterance, the row sums of the exp-domain recursion can stray from 1, from the fp64 oracle's alpha
    and beta alone.  The kernel keeps v_t = 2^(alpha_t - C_t) with E = exp(transition - row max) and emission factors relative to
    the largest of their 16-frame block, and moves C by a power of two every kRenorm steps with a lag of as many; so a row sum
    differs from 1 by at most
        |log row sum with the incoming vector at L1 norm 1|                                              (the mat-vec itself)
      + 2 kRenorm * max_t |log L1 growth of a frame once its largest emission factor is taken out|       (the lagged scale)
      + the spread of the frames' largest emission factors inside a 16-frame block                       (the block scale)
    (a bound, not the kernel's trajectory: anything near the 100 bits of Rng<float> has a reason to be flagged, anything a wide
    margin below it has none)."""
    x, tr = case.x.double().numpy(), case.tr.double().numpy()
    il = case.il.numpy()
    _, alpha, beta = orc.full_forward(x, tr, il)
    out = np.zeros(case.B)
    for b in range(case.B):
        n = int(il[b])
        if n < 2:
            continue
        worst = 0.0
        for side in (0, 1):
            if side == 0:     # alpha: state t-1 -> row sums of frame t
                M, st, e = tr, alpha[:n, b], x[:n, b]
            else:             # beta, in the kernel's own order (index m = frame n-1-m): state = beta + emission of its frame
                M, st, e = tr.T, (beta[:n, b] + x[:n, b])[::-1], x[:n, b][::-1]
            rmax = M.max(axis=1)
            norm = _lse(st, 1)                                                       # log L1 norm of the state of each index
            rows = _lse(M[None] - rmax[None, :, None] + st[:-1, None, :], 2) - norm[:-1, None]     # [n-1, N]: into index m+1
            emax = (e + rmax[None]).max(axis=1)                                      # largest emission factor of each index
            growth = norm[1:] - norm[:-1] - emax[1:]
            spread = 0.0
            for m0 in range(0, n, K_PF):
                blk = emax[m0:m0 + K_PF]
                spread = max(spread, float(blk.max() - blk.min()))
            worst = max(worst, float(np.abs(rows).max()) + 2 * K_RENORM * float(np.abs(growth).max()) + spread)
        out[b] = worst / np.log(2.0)
    return out


# ---- what the workspace of HipBackend.loss_forward says -------------------------------------------------------------------------
def align256(v):
    return (v + 255) // 256 * 256


def flags_of(saved, B, N):
    """The per-utterance flag words of a fused forward (1 = redone exactly by the backward launch), as tools/fused_flags.py reads
    them: behind the scores, the state and the [B][2][N][N] float tiles of the workspace."""
    ws = saved.tensors[0]
    sc_bytes, state_bytes, _ = saved.sizes
    off = sc_bytes + state_bytes + align256(B * 2 * N * N * 4)
    return ws[off: off + 4 * B].view(torch.int32).cpu().numpy()


def sync_bytes(B):
    return align256(256 + B * 64)               # asg_loss_fused_sync_bytes: the ticket block, then 64 bytes per utterance


def sync_region(be, dev, B):
    """The backend's zero-on-entry, zero-on-exit region of the calling stream (HipBackend._sync), as the fused forward got it."""
    return be._sync(torch.device(dev), sync_bytes(B))
