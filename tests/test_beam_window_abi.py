"""CPU tests of the C ABI and the Python surface of windowed streaming beam decoding (asg_beam_window_*,
`torch_asg_amd.BeamWindowStream`): the entry points exist and are declared, the size of a state follows the formula of the header
and does not depend on the length of an utterance, arguments are validated before anything touches a device -- no kernel is
launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = ("asg_beam_window_state_bytes", "asg_beam_window_reset", "asg_beam_window_advance", "asg_beam_window_result")


def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in WINDOW:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    assert int(L.asg_hip_version()) == 230
    import torch_asg_amd as A
    assert A.BeamWindowStream is not None and "BeamWindowStream" in A.__all__ and hasattr(A.ASGLoss, "beam_window_stream")
    assert A.BeamWindowCommit._fields == ("path", "states", "tokens", "token_lengths", "frames")
    assert A.BeamWindowResult._fields == ("scores", "path", "tokens", "token_lengths", "states", "frames", "committed", "status")


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
    sb = lambda K, B=64, W=128, P=32, dt=F32: int(L.asg_beam_window_state_bytes(ctypes.byref(gb), B, dt, K, W, P))
    a = lambda v: (v + 255) // 256 * 256

    def want(K, B=64, W=128, e=4):
        cap = max(min(g.Q, K * 40), 40)
        return B * (2 * a(W * K * 4) + a(g.Q * 8) + a(g.Q * e) + a(cap * e) + a(cap * 4) + 256 + a(K * (e + 4)))
    for K in (1, 64, 256, 1024, 8192):
        assert sb(K) == want(K)
    assert sb(64, 1, 1, 1) == want(64, 1, 1) and sb(64, 3, 130, 7) == want(64, 3, 130)
    assert sb(64, P=1) == sb(64, P=128) == sb(64)                    # the commit period takes no memory
    # the state of a stream of max_frames = W: the ring is all the back-pointers there are
    assert sb(256) == int(L.asg_beam_stream_state_bytes(ctypes.byref(gb), 64, F32, 256, 128))
    assert sb(256) < int(L.asg_beam_stream_state_bytes(ctypes.byref(gb), 64, F32, 256, 400))
    assert sb(0) == 0 and sb(-1) == 0 and sb(8193) == 0              # no beam; above K <= 8192
    assert sb(8, W=0) == 0 and sb(8, W=-5) == 0 and sb(8, B=0) == 0
    assert sb(8, P=0) == 0 and sb(8, P=-1) == 0 and sb(8, W=16, P=17) == 0 and sb(8, W=16, P=16) > 0
    assert sb(8, dt=F64) == 0 and sb(8, dt=7) == 0                   # not the graph's dtype
    assert int(L.asg_beam_window_state_bytes(None, 1, F32, 8, 10, 2)) == 0
    g.Q = 100
    assert sb(1 << 30) == sb(100) > 0                                # a beam above Q is Q
    g.Q = 65640

    big = 1 << 40
    reset = lambda K=8, B=2, W=10, P=2, state=256, n=big: L.asg_beam_window_reset(None, ctypes.byref(gb), B, K, W, P, state, n,
                                                                                  None, 0, None)
    assert reset(K=0) == 1 and reset(W=0) == 1 and reset(P=0) == 1 and reset(P=11) == 1 and reset(B=0) == 1
    assert reset(state=None) == 1
    assert reset(K=8193) == 2                                        # ASG_ERR_UNSUPPORTED
    assert reset(n=16) == 3 and reset(n=sb(8, 2, 10, 2) - 1) == 3    # ASG_ERR_WORKSPACE
    assert L.asg_beam_window_reset(None, None, 2, 8, 10, 2, 256, big, None, 0, None) == 1

    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.dtype = 4, 2, 40, F32
    p.inputs = p.transition = 256
    outs5 = (256,) * 5
    adv = lambda K=8, th=1.0, W=10, P=2, state=256, n=big, o=outs5: L.asg_beam_window_advance(
        None, ctypes.byref(p), ctypes.byref(gb), K, th, W, P, state, n, *o, 0, None)
    assert adv(K=0) == 1 and adv(th=-1.0) == 1 and adv(th=float("nan")) == 1 and adv(state=None) == 1
    assert adv(W=0) == 1 and adv(P=0) == 1 and adv(P=11) == 1
    assert adv(K=8193) == 2
    assert adv(n=sb(8, 2, 10, 2) - 1) == 3
    for i in range(5):
        assert adv(o=outs5[:i] + (None,) + outs5[i + 1:]) == 1       # every output is required
    assert L.asg_beam_window_advance(None, None, ctypes.byref(gb), 8, 1.0, 10, 2, 256, big, *outs5, 0, None) == 1
    p.T = -1
    assert adv() == 1                                                # Tc < 0
    p.T, p.N = 4, 39
    assert adv() == 1                                                # not the graph's alphabet
    p.N, p.inputs = 40, None
    assert adv() == 1                                                # a chunk of frames without emissions
    p.T, p.inputs, p.dtype = 4, 256, F64
    assert adv() == 1                                                # not the graph's dtype
    p.dtype = F32
    p.T = 0
    assert adv(n=16) == 3                                            # (Tc = 0 is a launch: it writes the empty outputs)

    outs = (256,) * 8
    res = lambda K=8, B=2, W=10, P=2, state=256, n=big, o=outs: L.asg_beam_window_result(None, ctypes.byref(gb), B, K, W, P, state,
                                                                                         n, 1, *o, 0, None)
    assert res(K=0) == 1 and res(W=0) == 1 and res(P=0) == 1 and res(P=11) == 1 and res(B=0) == 1 and res(state=None) == 1
    assert res(K=8193) == 2
    assert res(n=sb(8, 2, 10, 2) - 1) == 3
    for i in range(8):
        assert res(o=outs[:i] + (None,) + outs[i + 1:]) == 1         # every output is required, `committed` included
    # float64 states
    g64, gb64 = _graph(_lib, dtype=F64)
    assert int(L.asg_beam_window_state_bytes(ctypes.byref(gb64), 64, F64, 64, 128, 32)) == want(64, e=8)


def test_public_argument_errors_come_before_any_device_work():
    import torch
    import torch_asg_amd as A
    g = A.TokenGraph.from_ngram(np.log(np.full((6, 6), 1.0 / 6)))
    tr = torch.zeros(5, 5)
    for kw in (dict(beam_size=0), dict(beam_size=4, beam_threshold=-0.5), dict(beam_size=4, beam_threshold=float("nan"))):
        with pytest.raises(ValueError):
            A.BeamWindowStream(tr, g, 2, 10, **kw)
    for args in ((0, 10), (2, 0), (2, 10, 0), (2, 10, 11), (2, 10, -1)):
        with pytest.raises(ValueError):
            A.BeamWindowStream(tr, g, *args)
    with pytest.raises(TypeError):
        A.BeamWindowStream(tr, "graph", 2, 10)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.BeamWindowStream(tr, g, 2, 10)                             # a stream lives on the device
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.ASGLoss(5).beam_window_stream(g, 2, 10)
    with pytest.raises(RuntimeError):
        A.BeamWindowStream(tr, g, 2, 10, dtype=torch.float16, device="cuda:0")
