"""CPU tests of the C ABI and the Python surface of streaming beam decoding (asg_beam_stream_*, `torch_asg_amd.BeamStream`):
the entry points exist and are declared, the size of a state follows the formula of the header, arguments are validated before
anything touches a device -- no kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM = ("asg_beam_stream_state_bytes", "asg_beam_stream_reset", "asg_beam_stream_advance", "asg_beam_stream_result")


def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in STREAM:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    import torch_asg_amd as A
    assert A.BeamStream is not None and "BeamStream" in A.__all__ and hasattr(A.ASGLoss, "beam_stream")
    assert A.BeamStreamResult._fields == ("scores", "path", "tokens", "token_lengths", "states", "frames", "status")


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


def test_sizes_and_argument_validation_without_gpu():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32, F64 = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64
    g, gb = _graph(_lib)
    sb = lambda K, B=64, M=400, dt=F32: int(L.asg_beam_stream_state_bytes(ctypes.byref(gb), B, dt, K, M))
    a = lambda v: (v + 255) // 256 * 256

    def want(K, B=64, M=400, e=4):
        cap = max(min(g.Q, K * 40), 40)
        return B * (2 * a(M * K * 4) + a(g.Q * 8) + a(g.Q * e) + a(cap * e) + a(cap * 4) + 256 + a(K * (e + 4)))
    for K in (1, 64, 256, 1024, 8192):
        assert sb(K) == want(K)
    assert sb(64, 1, 1) == want(64, 1, 1) and sb(64, 3, 130) == want(64, 3, 130)
    # the one-shot decoder's workspace for T = max_frames, plus the header and the stored set
    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.dtype = 400, 64, 40, F32
    p.inputs = p.transition = 256
    one = int(L.asg_beam_decode_graph_work_bytes(ctypes.byref(p), ctypes.byref(gb), 256))
    assert sb(256) == one + 64 * (256 + a(256 * 8))
    assert sb(0) == 0 and sb(-1) == 0 and sb(8193) == 0              # no beam; above K <= 8192
    assert sb(8, M=0) == 0 and sb(8, M=-5) == 0 and sb(8, B=0) == 0
    assert sb(8, dt=F64) == 0 and sb(8, dt=7) == 0                   # not the graph's dtype
    assert int(L.asg_beam_stream_state_bytes(None, 1, F32, 8, 10)) == 0
    g.Q = 100
    assert sb(1 << 30) == sb(100) > 0                                # a beam above Q is Q
    g.Q = 65640

    big = 1 << 40
    reset = lambda K=8, B=2, M=10, state=256, n=big: L.asg_beam_stream_reset(None, ctypes.byref(gb), B, K, M, state, n, None, 0, None)
    assert reset(K=0) == 1 and reset(M=0) == 1 and reset(B=0) == 1 and reset(state=None) == 1
    assert reset(K=8193) == 2                                        # ASG_ERR_UNSUPPORTED
    assert reset(n=16) == 3 and reset(n=sb(8, 2, 10) - 1) == 3       # ASG_ERR_WORKSPACE
    assert L.asg_beam_stream_reset(None, None, 2, 8, 10, 256, big, None, 0, None) == 1

    p.T, p.B = 4, 2
    adv = lambda K=8, th=1.0, M=10, state=256, n=big: L.asg_beam_stream_advance(None, ctypes.byref(p), ctypes.byref(gb), K, th, M,
                                                                                 state, n, 0, None)
    assert adv(K=0) == 1 and adv(th=-1.0) == 1 and adv(th=float("nan")) == 1 and adv(M=0) == 1 and adv(state=None) == 1
    assert adv(K=8193) == 2
    assert adv(n=sb(8, 2, 10) - 1) == 3
    assert L.asg_beam_stream_advance(None, None, ctypes.byref(gb), 8, 1.0, 10, 256, big, 0, None) == 1
    p.T = -1
    assert adv() == 1                                                # Tc < 0
    p.T, p.N = 4, 39
    assert adv() == 1                                                # not the graph's alphabet
    p.N, p.inputs = 40, None
    assert adv() == 1                                                # a chunk of frames without emissions
    p.T = 0
    assert adv() == 0                                                # no frames: nothing to read, nothing launched
    assert adv(n=16) == 3
    p.T, p.inputs, p.dtype = 4, 256, F64
    assert adv() == 1                                                # not the graph's dtype
    p.dtype = F32

    outs = (256,) * 7
    res = lambda K=8, B=2, M=10, state=256, n=big, o=outs: L.asg_beam_stream_result(None, ctypes.byref(gb), B, K, M, state, n, 1,
                                                                                    *o, 0, None)
    assert res(K=0) == 1 and res(M=0) == 1 and res(B=0) == 1 and res(state=None) == 1 and res(K=8193) == 2
    assert res(n=sb(8, 2, 10) - 1) == 3
    for i in range(7):
        assert res(o=outs[:i] + (None,) + outs[i + 1:]) == 1         # every output is required
    # float64 states
    g64, gb64 = _graph(_lib, dtype=F64)
    assert int(L.asg_beam_stream_state_bytes(ctypes.byref(gb64), 64, F64, 64, 400)) == want(64, e=8)


def test_public_argument_errors_come_before_any_device_work():
    import torch
    import torch_asg_amd as A
    g = A.TokenGraph.from_ngram(np.log(np.full((6, 6), 1.0 / 6)))
    tr = torch.zeros(5, 5)
    for kw in (dict(beam_size=0), dict(beam_size=4, beam_threshold=-0.5), dict(beam_size=4, beam_threshold=float("nan"))):
        with pytest.raises(ValueError):
            A.BeamStream(tr, g, 2, 10, **kw)
    with pytest.raises(ValueError):
        A.BeamStream(tr, g, 0, 10)
    with pytest.raises(ValueError):
        A.BeamStream(tr, g, 2, 0)
    with pytest.raises(TypeError):
        A.BeamStream(tr, "graph", 2, 10)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.BeamStream(tr, g, 2, 10)                                   # a stream lives on the device
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.ASGLoss(5).beam_stream(g, 2, 10)
    with pytest.raises(RuntimeError):
        A.BeamStream(tr, g, 2, 10, dtype=torch.float16, device="cuda:0")
