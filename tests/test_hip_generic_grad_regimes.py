"""The full-lattice gradient of the generic loss (N > 64) seen at the scale of its own values, at the shapes where
the kernels of csrc/asg_generic_grad.hip change shape: bwd_gemm_mfma<1> whole and sliced with gemm_combine_kernel, the fp64
bwd_gemm_kernel<R, 1>, gemm3_pack_kernel + bwd_gemm_bf3_kernel in its whole-sliced / single-round / several-rounds / main + tail
launches with gemm3_tail_kernel, the row compaction of rowoff_kernel, and bwd_post_kernel behind every producer of the stored states.

Two ways to the full part on the device (cases, rule and references: tests/generic_grad_cases.py; what each case is and that it bites:
tests/test_generic_grad_regimes_cpu.py):
  (a) FCC alone under non-uniform upstream weights: both gradients ARE the full part, compared cell by cell;
  (b) the training call (ASGLoss, default mode and the serial route): the combined tensors against the oracle's full part on every
      cell whose aligned part is exactly zero (at least 99 % of them), the whole tensors by the parity rule as everywhere else.
Gates: 1e-4 (float32) and 1e-9 (float64) of the reference's own peak -- grad_inputs also per (t, b) row at that row's peak.
Every test prints what it measured; DESIGN.md 5c.1 holds the worst figure per regime."""
import numpy as np
import pytest
import torch

import generic_grad_cases as gc
import util

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CASES = gc.all_cases()
_TRAINING = [(c, False) for c in _CASES] + [(c, True) for c in _CASES if c.serial]
_WORST = {}


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _record(case, how, **errs):
    key = (case.regime or case.fwd, "f64" if case.f64 else "f32")
    w = _WORST.setdefault(key, {})
    for k, v in errs.items():
        w[k] = max(w.get(k, 0.0), v)
    print("[own scale] %-44s %-22s %s" % (case.name, how, "  ".join("%s %.2e" % kv for kv in errs.items())))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (regime, prec), w in sorted(_WORST.items()):
        print("[own scale, worst] %-34s %s  %s" % (regime, prec, "  ".join("%s %.2e" % kv for kv in sorted(w.items()))))


def _switches(case, monkeypatch):
    for k, v in case.env.items():
        util.setenv(monkeypatch, k, v)


def _full_alone(case):
    A = _asg()
    x = case.x.to(case.dtype).to(DEV).requires_grad_(True)
    tr = case.tr.to(case.dtype).to(DEV).requires_grad_(True)
    full = A.FCC.apply(tr, x, case.tg.to(DEV), case.il, case.tl)
    (full * case.w.to(case.dtype).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return full.detach().cpu().numpy(), x.grad.cpu().numpy(), tr.grad.cpu().numpy()


def _training(case, serial):
    A = _asg()
    m = A.ASGLoss(case.N, reduction="none", gpu_no_stream_impl=serial).to(DEV).to(case.dtype)
    with torch.no_grad():
        m.transition.copy_(case.tr.to(case.dtype))
    x = case.x.to(case.dtype).to(DEV).requires_grad_(True)
    loss = m(x, case.tg.to(DEV), case.il.to(DEV), case.tl.to(DEV))
    (loss * case.w.to(case.dtype).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return loss.detach().cpu().numpy(), x.grad.cpu().numpy(), m.transition.grad.cpu().numpy()


def _where(err_map, N):
    i, j = np.unravel_index(int(np.argmax(err_map)), err_map.shape)
    return "worst cell [%d][%d] (row %s; column %s)" % (i, j, gc.tiles_of(int(i)), gc.tiles_of(int(j)))


@pytest.mark.parametrize("case", _CASES, ids=[c.name for c in _CASES])
def test_full_lattice_alone(case, monkeypatch):
    """(a): FCC.apply under the weights -0.5 .. 1.5 with an exact 1.0 and an exact 0.0.  transition.grad is the oracle's
    grad_transition_full and x.grad its grad_inputs_full at their own scale (no valid row at all: exact zeros, not what the scratch
    buffers held); frames behind a length are +0.0, the rows of the utterance of weight zero are zero; a second call gives the same
    bits."""
    _switches(case, monkeypatch)
    o = gc.reference(case)
    g = gc.gate(case.dtype)
    full, gin, gtr = _full_alone(case)
    util.assert_close(full, o["full_scores"], 1e-9 if case.f64 else 1e-4, case.name + ": full scores")
    ref_t, ref_i = o["grad_transition_full"], o["grad_inputs_full"]
    e_t = gc.own_scale_err(gtr, ref_t)
    e_i = gc.own_scale_err(gin, ref_i)
    e_r, row = gc.row_errs(gin, ref_i, case.il.tolist(), case.w.tolist(), bitwise=True)
    _record(case, "full lattice alone", gtr=e_t, gin=e_i, gin_row=e_r)
    assert e_t <= g, "%s %s: grad_transition, full part: %.3e of its own peak %.3e > %.0e; K' = %d valid rows; %s" % (
        case.name, case.route(), e_t, np.abs(ref_t).max(), g, case.Kp, _where(np.abs(gtr - ref_t), case.N))
    assert e_i <= g, "%s: grad_inputs, full part: %.3e of its own peak > %.0e" % (case.name, e_i, g)
    assert e_r <= g, "%s (%s): grad_inputs row at its own peak: %.3e > %.0e: %s" % (case.name, case.fwd, e_r, g, row)
    for b in range(case.B):
        if float(case.w[b]) == 0.0:
            assert not gin[:, b].any(), "%s: utterance %d has weight zero" % (case.name, b)
    full2, gin2, gtr2 = _full_alone(case)
    assert np.array_equal(full, full2) and np.array_equal(gin, gin2) and np.array_equal(gtr, gtr2), case.name + ": run to run"


@pytest.mark.parametrize("case,serial", _TRAINING, ids=[c.name + ("-serial" if s else "") for c, s in _TRAINING])
def test_training_call(case, serial, monkeypatch):
    """(b): ASGLoss (default mode; gpu_no_stream_impl=True on one case per regime).  The whole tensors by the parity rule; on the
    cells whose aligned part is exactly zero the combined gradient against the oracle's full part at that part's own scale (the
    fp32 rounding of the sum costs 3e-8 there); no NaN beside an infeasible utterance; a second call gives the same bits."""
    _switches(case, monkeypatch)
    o = gc.reference(case)
    g = gc.gate(case.dtype)
    loss, gin, gtr = _training(case, serial)
    rtol = 1e-9 if case.f64 else gc.OLD_RTOL
    feasible = np.isfinite(o["loss"])
    assert not feasible[list(case.infeasible)].any() and feasible.sum() == case.B - len(case.infeasible)
    util.assert_close(loss, o["loss"], rtol, case.name + ": loss")
    util.assert_close(gin, o["grad_inputs"], rtol, case.name + ": grad_inputs, parity rule")
    util.assert_close(gtr, o["grad_transition"], rtol, case.name + ": grad_transition, parity rule")
    mt, mi = gc.training_cells(o)
    ref_t, ref_i = o["grad_transition_full"], o["grad_inputs_full"]
    e_t = gc.own_scale_err(gtr, ref_t, mt)
    errs = dict(gtr=e_t)
    assert e_t <= g, "%s %s: grad_transition off the target's cells: %.3e of the full part's peak %.3e > %.0e; K' = %d; %s" % (
        case.name, case.route(), e_t, np.abs(ref_t).max(), g, case.Kp, _where(np.where(mt, np.abs(gtr - ref_t), 0.0), case.N))
    if case.gin_in_training:
        e_i = gc.own_scale_err(gin, ref_i, mi)
        e_r, row = gc.row_errs(gin, ref_i, case.il.tolist(), case.w.tolist(), cells=mi)
        errs.update(gin=e_i, gin_row=e_r)
        assert e_i <= g, "%s: grad_inputs off the target's labels: %.3e of the full part's peak > %.0e" % (case.name, e_i, g)
        assert e_r <= g, "%s (%s): grad_inputs row off the target's labels: %.3e > %.0e: %s" % (case.name, case.fwd, e_r, g, row)
    _record(case, "training call, serial" if serial else "training call", **errs)
    loss2, gin2, gtr2 = _training(case, serial)
    assert np.array_equal(loss, loss2) and np.array_equal(gin, gin2) and np.array_equal(gtr, gtr2), case.name + ": run to run"
