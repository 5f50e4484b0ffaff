#!/usr/bin/env python3
"""Scaled error (the parity rule's figure, tests/util.py::tol_ok) of the beam-pruned graph loss against the numpy restatement
tests/beam_loss_ref.py by utterance length -- the table "float32 at long T" of DESIGN.md section 5j.  The case is
tests/test_hip_beam_loss_regimes.py::long_case(T, dtype): bigram over 10 tokens, K = 4, B = 10, S = 40 targets forced, equal
full lengths.  One line per (dtype, T).

    python tools/beam_loss_f32_error.py [T ...]            (default 60 125 250 500 1000 2000 3000)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_hip_beam_loss_regimes as R  # noqa: E402
from beam_loss_cases import _full  # noqa: E402
from util import tol_ok  # noqa: E402

for dt in (torch.float32, torch.float64):
    for T in [int(a) for a in sys.argv[1:]] or (60, 125, 250, 500, 1000, 2000, 3000):
        graph, x, tr, il, tg, tl, gs = R.long_case(T, dt)
        want, _, _ = R._reference(x, tr, graph, il, 4, R.INF, gs, tg, tl)
        got = _full(x, tr, graph, il, 4, gs=gs, tg=tg, tl=tl)
        errs = [tol_ok(g.numpy(), w)[1] for g, w in zip(got, want)]
        print("%s T=%d max|Z| %.1f scaled err: Z %.3e grad_inputs %.3e grad_transition %.3e"
              % (dt, T, abs(want[0]).max(), errs[0], errs[1], errs[2]), flush=True)
