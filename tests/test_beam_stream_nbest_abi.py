"""CPU tests of the C ABI and the Python surface of the n-best lists of the two token-graph beam streams (asg_beam_stream_nbest,
asg_beam_window_nbest, `BeamStream.result_nbest`, `BeamWindowStream.result_nbest`): the entry points exist and are declared, the
scratch follows the formulas of the header, arguments are validated before anything touches a device -- no kernel is launched
here."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("asg_beam_stream_nbest_work_bytes", "asg_beam_stream_nbest", "asg_beam_window_nbest_work_bytes", "asg_beam_window_nbest")


def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    assert int(L.asg_hip_version()) == 230                           # additions only


def _graph(_lib, Q=65640, E=2559960, N=40, dtype=None):
    g = _lib.AsgTokenGraph()
    g.Q, g.E, g.N, g.dtype = Q, E, N, _lib.ASG_DTYPE_F32 if dtype is None else dtype
    for n in ("label", "state", "row", "src", "src_label", "start_w", "final_w", "edge_w"):
        setattr(g, n, 256)                                           # never dereferenced here
    gb = _lib.AsgTokenGraphBeam()
    gb.graph = ctypes.pointer(g)
    gb.num_start, gb.max_out = 40, 39
    for n in ("orow", "oarc", "ow", "start_q"):
        setattr(gb, n, 256)
    return g, gb


def _a256(v):
    return (v + 255) // 256 * 256


def test_stream_sizes_and_argument_validation_without_gpu():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32, F64 = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64
    g, gb = _graph(_lib)
    wb = lambda K, nbest, B=64, M=400, dt=F32: int(L.asg_beam_stream_nbest_work_bytes(ctypes.byref(gb), B, dt, K, M, nbest))
    for K, nbest, B, M in ((256, 100, 64, 400), (256, 1, 1, 400), (64, 100, 3, 130), (8192, 8192, 2, 7), (1, 5, 2, 1)):
        assert wb(K, nbest, B, M) == B * _a256(M * min(nbest, K) * 4)
    assert wb(256, 0) == 0 and wb(256, -3) == 0 and wb(256, 8193) == 0
    assert wb(0, 1) == 0 and wb(8193, 1) == 0 and wb(8, 1, B=0) == 0 and wb(8, 1, M=0) == 0 and wb(8, 1, dt=F64) == 0
    assert int(L.asg_beam_stream_nbest_work_bytes(None, 1, F32, 8, 10, 1)) == 0
    g.Q = 100
    assert wb(1 << 30, 500) == wb(100, 500) == 64 * _a256(400 * 100 * 4)      # a beam above Q is Q
    g.Q = 65640

    big = 1 << 40
    outs = (256,) * 9                # scores, graph_scores, path, tokens, token_lengths, states, num_hyps, frames, status
    sb = int(L.asg_beam_stream_state_bytes(ctypes.byref(gb), 2, F32, 8, 10))
    call = lambda K=8, B=2, M=10, state=256, n=big, nbest=3, work=256, wn=big, o=outs: L.asg_beam_stream_nbest(
        None, ctypes.byref(gb), B, K, M, state, n, 1, nbest, work, wn, *o, 0, None)
    assert call(K=0) == 1 and call(M=0) == 1 and call(B=0) == 1 and call(state=None) == 1 and call(work=None) == 1
    assert call(K=8193) == 2
    assert call(nbest=0) == 1 and call(nbest=-1) == 1 and call(nbest=8193) == 2
    assert call(n=sb - 1) == 3 and call(n=16) == 3
    need = 2 * _a256(10 * 3 * 4)
    assert wb(8, 3, 2, 10) == need and call(wn=need - 1) == 3 and call(wn=0) == 3         # a `work` one byte short
    for i in range(9):
        if i not in (2, 5):                                          # path and states may be NULL
            assert call(o=outs[:i] + (None,) + outs[i + 1:]) == 1
    assert L.asg_beam_stream_nbest(None, None, 2, 8, 10, 256, big, 1, 3, 256, big, *outs, 0, None) == 1
    g64, gb64 = _graph(_lib, dtype=F64)
    assert int(L.asg_beam_stream_nbest_work_bytes(ctypes.byref(gb64), 4, F64, 64, 50, 10)) == 4 * _a256(50 * 10 * 4)


def test_window_sizes_and_argument_validation_without_gpu():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32, F64 = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64
    g, gb = _graph(_lib)
    wb = lambda K, nbest, B=64, W=128, P=32, dt=F32: int(L.asg_beam_window_nbest_work_bytes(ctypes.byref(gb), B, dt, K, W, P, nbest))
    for K, nbest, B, W in ((256, 100, 64, 128), (256, 1, 1, 128), (64, 100, 3, 65), (8192, 8192, 2, 7), (1, 5, 2, 1)):
        assert wb(K, nbest, B, W, 1) == B * _a256(W * min(nbest, K) * 4)
    assert wb(256, 10, P=1) == wb(256, 10, P=128)                    # the commit period takes no memory
    assert wb(256, 0) == 0 and wb(256, -3) == 0 and wb(256, 8193) == 0
    assert wb(0, 1) == 0 and wb(8193, 1) == 0 and wb(8, 1, B=0) == 0 and wb(8, 1, W=0) == 0 and wb(8, 1, dt=F64) == 0
    assert wb(8, 1, P=0) == 0 and wb(8, 1, W=16, P=17) == 0
    assert int(L.asg_beam_window_nbest_work_bytes(None, 1, F32, 8, 10, 2, 1)) == 0

    big = 1 << 40
    outs = (256,) * 9                # scores, path, tokens, token_lengths, states, num_hyps, frames, committed, status
    sb = int(L.asg_beam_window_state_bytes(ctypes.byref(gb), 2, F32, 8, 10, 2))
    call = lambda K=8, B=2, W=10, P=2, state=256, n=big, nbest=3, work=256, wn=big, o=outs: L.asg_beam_window_nbest(
        None, ctypes.byref(gb), B, K, W, P, state, n, 0, nbest, work, wn, *o, 0, None)
    assert call(K=0) == 1 and call(W=0) == 1 and call(P=0) == 1 and call(P=11) == 1 and call(B=0) == 1
    assert call(state=None) == 1 and call(work=None) == 1
    assert call(K=8193) == 2
    assert call(nbest=0) == 1 and call(nbest=-1) == 1 and call(nbest=8193) == 2
    assert call(n=sb - 1) == 3
    need = 2 * _a256(10 * 3 * 4)
    assert wb(8, 3, 2, 10, 2) == need and call(wn=need - 1) == 3     # a `work` one byte short
    for i in range(9):
        if i not in (1, 4):                                          # path and states may be NULL
            assert call(o=outs[:i] + (None,) + outs[i + 1:]) == 1
    assert L.asg_beam_window_nbest(None, None, 2, 8, 10, 2, 256, big, 0, 3, 256, big, *outs, 0, None) == 1


def test_public_argument_errors_come_before_any_device_work():
    import torch
    import torch_asg_amd as A
    g = A.TokenGraph.from_ngram(np.log(np.full((6, 6), 1.0 / 6)))
    for cls in (A.BeamStream, A.BeamWindowStream):
        s = cls.__new__(cls)                                         # a stream whose constructor never ran: nbest is checked first
        for bad in (0, -1):
            with pytest.raises(ValueError, match="nbest"):
                cls.result_nbest(s, bad)
            with pytest.raises(ValueError, match="nbest"):
                cls.result_nbest(s, bad, final=True, return_alignments=True)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.BeamStream(torch.zeros(5, 5), g, 2, 10)
