"""CPU tests of the Viterbi (hard) score over target graphs: the exported names, the C entry points' size formulas and
refusals (include/asg_hip.h::asg_target_graph_viterbi_forward) -- no kernel is launched here."""
import ctypes

import numpy as np
import pytest

import torch_asg_amd as A
from test_target_graph_viterbi_cpu import CYCLE, DIAMOND
from torch_asg_amd import TargetGraphs, _lib


def test_exported_names_and_version():
    for name in ("TargetGraphViterbiScore", "target_graph_viterbi_score", "target_graph_viterbi_loss"):
        assert name in A.__all__ and hasattr(A, name)
    assert hasattr(A.ASGLoss, "target_graph_viterbi_loss")
    for name in ("asg_target_graph_viterbi_train_work_bytes", "asg_target_graph_viterbi_train_scratch_bytes",
                 "asg_target_graph_viterbi_forward", "asg_target_graph_viterbi_backward"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert _lib.lib().asg_hip_version() == _lib.ABI_VERSION == 230


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_c_entry_points_without_a_device(dt):
    L = _lib.lib()
    graphs = TargetGraphs(*[[s[n] for s in (DIAMOND, CYCLE)] for n in range(4)], 3)
    h = graphs.compile_host(dt)
    g = _lib.AsgTargetGraphs()
    g.B, g.Kmax, g.Emax, g.npairs, g.N = 2, graphs.Kmax, graphs.Emax, h["pkey"].size, 3
    g.dtype = _lib.ASG_DTYPE_F32 if dt == np.float32 else _lib.ASG_DTYPE_F64
    for n in _lib.TARGET_GRAPH_ARRAYS:
        setattr(g, n, h[n].ctypes.data)
    p, dummy = _lib.AsgProblem(), np.zeros(8, dt)
    p.inputs, p.transition = dummy.ctypes.data, dummy.ctypes.data
    p.T, p.B, p.N, p.S, p.dtype = 7, 2, 3, 1, g.dtype
    P, G, one = ctypes.byref(p), ctypes.byref(g), ctypes.c_void_p(1)
    need = L.asg_target_graph_viterbi_train_work_bytes(P, G, 1)
    # r16(B T Kmax 2) + r16(B T 4) + r16(B (Kmax + Emax) 4) + r16(B T 2) at B = 2, T = 7, Kmax = Emax = 4
    assert (graphs.Kmax, graphs.Emax) == (4, 4) and need == 112 + 64 + 64 + 32
    assert L.asg_target_graph_viterbi_train_work_bytes(P, G, 0) == 0 == L.asg_target_graph_viterbi_train_scratch_bytes(P, G)

    def fwd(nbytes=need, null=-1, tg=G, flags=_lib.FLAG_GRAPH_LOSS_KEEP_ALPHA):
        a = [None if i == null else one for i in range(2)]                  # work, scores
        return L.asg_target_graph_viterbi_forward(None, P, tg, a[0], nbytes, a[1], flags, None)

    def bwd(nbytes=need, null=-1, tg=G):
        a = [None if i == null else one for i in range(5)]                  # work, scores, grad_scores, grad_inputs, grad_transition
        return L.asg_target_graph_viterbi_backward(None, P, tg, a[0], nbytes, *a[1:], None, 0, 0, None)
    assert [fwd(null=i) for i in range(2)] == [1] * 2 and fwd(tg=None) == 1               # ASG_ERR_INVALID: a null pointer
    assert [bwd(null=i) for i in range(5)] == [1] * 5 and bwd(tg=None) == 1               # (a null scratch is none: it is unused)
    assert fwd(nbytes=need - 1) == 3 and bwd(nbytes=need - 1) == 3          # ASG_ERR_WORKSPACE: one byte short
    assert fwd(nbytes=0, null=1, flags=0) == 1                              # without the flag only scores is needed, and is null
    p.B = 3
    assert fwd() == 1 and bwd() == 1                                        # p->B != tg->B
    p.B = 2
    g.Kmax = 1025
    assert fwd() == 2 and bwd() == 2 and L.asg_target_graph_viterbi_train_work_bytes(P, G, 1) == 0      # ASG_ERR_UNSUPPORTED
    g.Kmax = graphs.Kmax
    g.Emax = L.asg_target_graph_max_edges(g.dtype, g.Kmax) + 1
    assert fwd() == 2 and bwd() == 2 and L.asg_target_graph_viterbi_train_work_bytes(P, G, 1) == 0
