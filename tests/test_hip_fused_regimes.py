"""The fused training step (csrc/asg_fused.hip: fused_fwd_kernel + fused_bwd_kernel) at the lengths, alphabets, paddings, batch
sizes and targets where its kernels change shape (cases and restated shape rules: tests/fused_regime_cases.py; their
CPU half: tests/test_fused_regimes_cpu.py).

Every call goes through HipBackend.loss_forward(..., FLAG_SINGLE_LAUNCH) + loss_backward, which shows the route that ran and its
workspace, and is checked for ALL of
  (a) the route: "fused" (or "split" where the case says so),
  (b) the flag words: 1 exactly at the utterances of fewer than kMinFused frames or with emissions outside the fp32 window, 0
      elsewhere -- a flagged utterance is redone by the exact stand-alone code and passes every comparison, so a regression that
      flags a whole length class shows only here.  (An utterance whose target is longer than its input is NOT flagged: the
      finishers of the aligned workgroup find no mass on its first frame, write zero posteriors, and the score comes out as
      log-zero -- loss +inf, gradient rows the full-lattice posterior, all on the fused path.  A -inf label is not flagged
      either: its emission factor is 0, its row sum is as large as its neighbours'.)
  (c) the sync region of the stream: all zero once the device is idle,
  (d) loss, grad_inputs and grad_transition against the fp64 oracle under the project's rule (1e-4 of max(1, max|ref|); bfloat16
      emissions: grad_inputs 2^-8) -- grad_inputs and the per-utterance loss PER UTTERANCE, so that one bad row of a short
      utterance is not measured against the largest number of the batch,
  (e) grad_inputs[len:, b] bitwise zero,
  (f) a second run: the same bits.
"""
import collections

import numpy as np
import pytest
import torch

import fused_regime_cases as fc
import util

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST = collections.defaultdict(lambda: [0.0, 0.0, 0.0])     # group -> worst scaled error of loss, grad_inputs, grad_transition


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for grp, (el, eg, et) in sorted(WORST.items()):
        print("\nfused regimes, worst scaled error vs fp64 oracle [%s]: loss %.2e  grad_inputs %.2e  grad_transition %.2e"
              % (grp, el, eg, et))


def _be():
    import torch_asg_amd
    return torch_asg_amd.asg.native()


def _edge():
    return fc.fused_edge(int(torch.cuda.get_device_properties(0).multi_processor_count))


class Result:
    pass


def _device_args(case):
    x = case.x.to(torch.bfloat16) if case.bf16 else case.x
    if case.batch_major:
        x = x.permute(1, 0, 2).contiguous().to(DEV).permute(1, 0, 2)          # a [T,B,N] view of batch-major storage
    else:
        x = x.to(DEV)
    g = case.w.to(DEV) if case.reduction == "none" and case.w is not None else None
    if g is None:
        g = torch.ones((case.B,) if case.reduction == "none" else (), device=DEV)
    return x, case.tg.to(DEV), case.tr.to(DEV), case.il.to(DEV), case.tl.to(DEV), g


def run(case):
    """One forward + backward through the backend.  Everything read back is read after the device went idle."""
    from torch_asg_amd import _lib
    be = _be()
    x, tg, tr, il, tl, g = _device_args(case)
    loss, saved = be.loss_forward(x, tg, tr, il, tl, case.reduction, _lib.FLAG_SINGLE_LAUNCH)
    gtr, gin = be.loss_backward(saved, saved.tensors, g, x, tg, tr, il, tl, case.reduction)
    torch.cuda.synchronize()
    r = Result()
    r.mode = saved.mode
    r.flags = fc.flags_of(saved, case.B, case.N) if saved.mode == "fused" else None
    r.sync_nonzero = int(torch.count_nonzero(fc.sync_region(be, DEV, case.B)))
    r.loss, r.gin, r.gtr = loss.cpu(), gin.cpu(), gtr.cpu()
    return r


def run_module(case):
    """The same call as a user makes it: ASGLoss, autograd."""
    import torch_asg_amd
    x, tg, tr, il, tl, g = _device_args(case)
    m = torch_asg_amd.ASGLoss(case.N, reduction=case.reduction).to(DEV)
    with torch.no_grad():
        m.transition.copy_(tr)
    xd = x.detach().requires_grad_(True)
    loss = m(xd, tg, il, tl)
    if case.reduction == "none":
        loss.backward(g)
    else:
        loss.backward()
    torch.cuda.synchronize()
    r = Result()
    r.loss, r.gin, r.gtr = loss.detach().cpu(), xd.grad.cpu(), m.transition.grad.cpu()
    return r


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def problems(case, r, again=None):
    """-> the list of everything (a) .. (f) that does not hold for result r (and its repetition `again`)."""
    bad = []
    o = fc.reference(case)
    il = case.il.numpy()
    T, B = case.T, case.B
    want = "fused" if case.fused and B <= _edge() else "split"
    if r.mode != want:                                                                                    # (a)
        bad.append("%s: route %s, expected %s" % (case.name, r.mode, want))
    if r.mode == "fused" and not np.array_equal(r.flags != 0, case.flagged):                              # (b)
        bad.append("%s: flags %s, expected %s (lengths %s)" % (case.name, (r.flags != 0).astype(int).tolist(),
                                                               case.flagged.astype(int).tolist(), il.tolist()))
    if r.sync_nonzero:                                                                                    # (c)
        bad.append("%s: %d non-zero bytes left in the sync region" % (case.name, r.sync_nonzero))
    grp = case.name.split("-")[0] + ("-bf16" if case.bf16 else "")
    gin = r.gin.float().numpy().astype(np.float64)
    if r.gin.dtype != (torch.bfloat16 if case.bf16 else torch.float32):
        bad.append("%s: grad_inputs came back as %s" % (case.name, r.gin.dtype))
    rtol_g = 2.0 ** -8 if case.bf16 else 1e-4
    ref = o["grad_inputs"]
    for b in range(B):                                                                                    # (d) per utterance
        n = int(il[b])
        scale = max(1.0, float(np.abs(ref[:, b]).max()))
        err = np.abs(gin[:, b] - ref[:, b])
        err = np.where(np.isfinite(err), err, np.inf)
        t = int(err.max(axis=1).argmax())
        e = float(err.max()) / scale
        WORST[grp][1] = max(WORST[grp][1], e)
        if not e <= rtol_g:
            bad.append("%s: grad_inputs of utterance b=%d: scaled error %.3e > %.1e, worst at frame t=%d (len %d, crossing %d, T %d)"
                       % (case.name, b, e, rtol_g, t, n, fc.crossing(n), T))
        tail = _bits(r.gin[n:, b])
        if np.any(tail != 0):                                                                             # (e)
            bad.append("%s: grad_inputs[%d:, b=%d] is not bitwise zero (len %d, crossing %d, T %d): holds the bit patterns %s"
                       % (case.name, n, b, n, fc.crossing(n), T, [hex(int(v) & 0xffffffff) for v in np.unique(tail[tail != 0])[:4]]))
    loss = r.loss.numpy().astype(np.float64)
    if case.reduction == "none":
        for b in range(B):
            ok, e = util.tol_ok(loss[b:b + 1], o["loss"][b:b + 1], 1e-4)
            WORST[grp][0] = max(WORST[grp][0], e if np.isfinite(o["loss"][b]) else 0.0)
            if not ok:
                n = int(il[b])
                bad.append("%s: loss of utterance b=%d: %r vs %r, scaled error %.3e (len %d, crossing %d, T %d)"
                           % (case.name, b, loss[b], o["loss"][b], e, n, fc.crossing(n), T))
    else:
        ok, e = util.tol_ok(loss, np.asarray(o["loss"]), 1e-4)
        WORST[grp][0] = max(WORST[grp][0], e)
        if not ok:
            bad.append("%s: loss %r vs %r, scaled error %.3e" % (case.name, loss, o["loss"], e))
    ok, e = util.tol_ok(r.gtr.numpy(), o["grad_transition"], 1e-4)
    WORST[grp][2] = max(WORST[grp][2], e)
    if not ok:
        bad.append("%s: grad_transition: scaled error %.3e > 1e-4" % (case.name, e))
    if again is not None:                                                                                 # (f)
        for what in ("loss", "gin", "gtr"):
            if not same_bits(getattr(r, what), getattr(again, what)):
                bad.append("%s: %s differs between two runs" % (case.name, what))
        if r.mode == "fused" and again.mode == "fused" and not np.array_equal(r.flags, again.flags):
            bad.append("%s: flags differ between two runs" % case.name)
        if again.sync_nonzero:
            bad.append("%s: %d non-zero bytes left in the sync region by the second run" % (case.name, again.sync_nonzero))
    return bad


def checked(case, module=False):
    """Run twice, assert (a) .. (f); module=True: the ASGLoss module must give the same bits.  -> the first result."""
    r, again = run(case), run(case)
    bad = problems(case, r, again)
    if module:
        m = run_module(case)
        for what in ("loss", "gin", "gtr"):
            if not same_bits(getattr(r, what), getattr(m, what)):
                bad.append("%s: %s of the ASGLoss module differs from the backend call" % (case.name, what))
    assert not bad, "\n".join(bad)
    return r


# ---------------------------------------------------------------------------------------------------------------- length sweep
def _sweep(N, third, bf16):
    """Seven batches back to back on one stream: a sync word that one length class leaves non-zero breaks the next batch, and (c)
    names the batch that left it.  Everything that fails is reported, not the first batch only."""
    bad = []
    for k in range(7 * third, 7 * third + 7):
        case = fc.sweep_case(N, k, bf16)
        r, again = run(case), run(case)
        bad += problems(case, r, again)
        if k in (0, 4, 9, 20):          # (lengths 1..16, 65..80, 145..160, 321..336)
            m = run_module(case)
            bad += ["%s: %s of the ASGLoss module differs from the backend call" % (case.name, w) for w in ("loss", "gin", "gtr")
                    if not same_bits(getattr(r, w), getattr(m, w))]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("third", range(3))
@pytest.mark.parametrize("N", fc.SWEEP_N)
def test_every_length_1_to_336(N, third):
    """kMinFused, crossing = len / 2 and the searched crossing in its eight classes, every remainder of the 8-frame groups over
    two and three consumers, one and two turns of the rings; weights -0.5 .. 1.5 with an exact 1.0 and an exact 0.0."""
    _sweep(N, third, False)


@pytest.mark.parametrize("third", range(3))
def test_every_length_1_to_336_bf16(third):
    """The same sweep on bfloat16 emissions at the benchmark's tile (the short, flagged utterances read the widened copy)."""
    _sweep(40, third, True)


def test_batch_major_strides():
    """One sweep batch as a permuted [B,T,N] view: the same bits as the time-major call."""
    r = checked(fc.sweep_case(40, 9, batch_major=True))
    base = run(fc.sweep_case(40, 9))
    assert same_bits(r.loss, base.loss) and same_bits(r.gin, base.gin) and same_bits(r.gtr, base.gtr)


def test_row_pass_second_outer_iteration():
    """Lengths 496..527: nq = 125..133 quads -- one and two iterations of the row pass's outer loop (128 quads each)."""
    checked(fc.rowpass_case(), module=True)


# ---------------------------------------------------------------------------------------------------------------- alphabet
@pytest.mark.parametrize("N", fc.NP_ALPHABETS)
def test_every_alphabet_tile_past_the_rings(N):
    """Both sides of every NP edge (two and three consumers), second halves below and above one turn of the rings; N = 1 is the
    one-label cancellation of grad_transition."""
    checked(fc.np_case(N), module=N in (1, 40, 63))


# ---------------------------------------------------------------------------------------------------------------- T padding
def _rows(case, r, places=None):
    """Per-utterance loss and the live rows of grad_inputs of a reduction-'none' result, by utterance."""
    places = range(case.B) if places is None else places
    return [(r.loss[b:b + 1].clone(), r.gin[:int(case.il[b]), b].clone()) for b in places]


def _pad_sweep(bf16):
    bad, base = [], None
    for T in fc.PAD_T:
        case = fc.pad_case(T, bf16)
        r, again = run(case), run(case)
        bad += problems(case, r, again)
        rows = _rows(case, r)
        if base is None:
            base, base_gtr = rows, r.gtr
            continue
        for b, ((l0, g0), (l1, g1)) in enumerate(zip(base, rows)):
            n = fc.PAD_LENGTHS[b]
            if not same_bits(l0, l1):
                bad.append("T=%d: loss of utterance %d (len %d, crossing %d) differs from T=%d" % (T, b, n, fc.crossing(n), fc.PAD_T[0]))
            if not same_bits(g0, g1):
                d = (g0.float() - g1.float()).abs().amax(dim=1)
                bad.append("T=%d: grad_inputs of utterance %d (len %d, crossing %d) differs from T=%d, first at frame %d"
                           % (T, b, n, fc.crossing(n), fc.PAD_T[0], int((d > 0).nonzero()[0])))
        if not same_bits(base_gtr, r.gtr):
            bad.append("T=%d: grad_transition differs from T=%d" % (T, fc.PAD_T[0]))
    assert not bad, "\n".join(bad)


def test_time_extent_does_not_change_an_utterance():
    """The same eight utterances at T = 130 .. 146 (p2 [T + 8], xstate (T + 7) / 8 + 2 blocks, aoff (T + 15) / 16 + 1 entries per
    utterance and side; S = 64): an utterance's arithmetic depends on its length, not on T -- all seventeen results are the same bits."""
    _pad_sweep(False)


def test_time_extent_does_not_change_an_utterance_bf16():
    _pad_sweep(True)


def test_time_extent_module_route():
    checked(fc.pad_case(137), module=True)


# ---------------------------------------------------------------------------------------------------------------- neighbours
def test_neighbours_do_not_change_an_utterance():
    """The same eight utterances in another order, between eight others, and alone: per-utterance loss and grad_inputs rows keep
    their bits wherever the utterance stands (reductions 'none' and 'sum': gscale = 1); 'mean' holds against the oracle."""
    base_case = fc.pad_case(130)
    base = _rows(base_case, checked(base_case))
    bad = []
    kinds = ["reordered", "interleaved"] + ["alone-%d" % i for i in range(8)]
    for red in ("none", "sum"):
        for kind in kinds:
            case, where = fc.neighbour_case(kind, red)
            r = checked(case, module=kind == "interleaved")
            for i in (range(8) if isinstance(where, list) else where):
                b = where[i]
                if red == "none" and not same_bits(base[i][0], r.loss[b:b + 1]):
                    bad.append("%s: loss of utterance %d (now at %d) changed" % (case.name, i, b))
                if not same_bits(base[i][1], r.gin[:fc.PAD_LENGTHS[i], b].clone()):
                    bad.append("%s: grad_inputs rows of utterance %d (now at %d) changed" % (case.name, i, b))
    checked(fc.neighbour_case("interleaved", "mean")[0])
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------- batch
@pytest.mark.parametrize("B", fc.BATCH_SIZES)
def test_batch_edges(B):
    """Both sides of every step of the grid (48 workgroups per 16 utterances), an odd utterance without its XCD partner, and the
    last batch the fused launch takes on 256 compute units."""
    checked(fc.batch_case(B), module=B in (17, 80))


def test_first_batch_past_the_fused_edge_is_split():
    """fused_preferred's edge on THIS device (80 on 256 compute units), restated; one utterance more takes the stand-alone kernels."""
    edge, cus = _edge(), int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert fc.fused_preferred(edge, cus) and not fc.fused_preferred(edge + 1, cus)
    r = checked(fc.batch_case(edge + 1, fused=False))
    assert r.mode == "split"
    if edge not in fc.BATCH_SIZES:
        assert checked(fc.batch_case(edge)).mode == "fused"


# ---------------------------------------------------------------------------------------------------------------- top of the range
def test_longest_fused_utterance_and_the_first_split_one():
    """T = 4000: kMaxBlk - 1 blocks of 16 indices per half at most; T = 4001 takes the stand-alone route."""
    assert checked(fc.top_case(fc.T_MAX), module=True).mode == "fused"
    assert checked(fc.top_case(fc.T_MAX + 1)).mode == "split"


# ---------------------------------------------------------------------------------------------------------------- targets
@pytest.mark.parametrize("kind", fc.TARGET_KINDS)
def test_targets(kind):
    """S = 1, 2, 63, 64 lanes with target lengths 1 .. S in one batch; tl == il (one alignment); one label 64 times (the scatter adds
    64 positions into one LDS word); targets padded with a label the utterance uses (P2 must be exact zeros behind tl)."""
    case = fc.target_case(kind)
    r = checked(case, module=kind in ("S64", "tight"))
    if kind == "tight":
        # a single alignment: the aligned posterior is 1 at the target's label of every frame, so the rows of grad_inputs sum to 0
        # like every row, and the label's entry is (full posterior - 1)
        for b in range(case.B):
            n = int(case.il[b])
            g = r.gin[:n, b].double()
            at = g[torch.arange(n), case.tg[b, :n]]
            assert float(g.sum(dim=1).abs().max()) < 1e-4 and bool((at <= 1e-4).all()) and bool((at >= -1 - 1e-4).all()), b


# ---------------------------------------------------------------------------------------------------------------- mixed batch
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_mixed_batch(bf16):
    """Ordinary utterances beside lengths 1, 2, 3, an infeasible target, a -inf label and emissions 40 * randn: the flags are exactly
    the predicted ones (the short ones and the wide one), the redo scales by 1.0, 0.37 and 0.0 (its g != 1 branch), the infeasible
    utterance's loss is +inf, and the ordinary utterances carry the bits they carry in a batch without the others."""
    case, plain = fc.mixed_case(bf16), fc.mixed_plain_case(bf16)
    r = checked(case, module=True)
    p = _rows(plain, checked(plain))
    for (l0, g0), b in zip(p, fc.MIXED_ORDINARY):
        n = int(case.il[b])
        assert same_bits(l0, r.loss[b:b + 1]), "loss of the ordinary utterance at %d changed beside the flagged ones" % b
        assert same_bits(g0, r.gin[:n, b].clone()), "grad_inputs of the ordinary utterance at %d changed beside the flagged ones" % b
    assert np.isposinf(r.loss[6].item())
