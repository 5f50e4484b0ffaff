"""CPU tests of the C ABI and the Python surface of the lattice-keeping beam stream (asg_beam_conf_stream_*,
`torch_asg_amd.BeamStream(..., keep_lattice=True)`): the entry points exist and are declared, the size of a state follows the
formula of the header, arguments are validated before anything touches a device -- no kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("asg_beam_conf_stream_state_bytes", "asg_beam_conf_stream_reset", "asg_beam_conf_stream_advance",
         "asg_beam_conf_stream_result", "asg_beam_conf_stream_nbest_work_bytes", "asg_beam_conf_stream_nbest",
         "asg_beam_conf_stream_confidence")


def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    assert int(L.asg_hip_version()) == _lib.ABI_VERSION == 230           # additions only: the version stays
    import torch_asg_amd as A
    assert "BeamStreamConfidence" in A.__all__
    assert A.BeamStreamConfidence._fields == ("scores", "path", "tokens", "token_lengths", "states", "token_frames",
                                              "token_confidences", "normalisers", "frames", "status")
    import inspect
    assert inspect.signature(A.BeamStream.__init__).parameters["keep_lattice"].default is False
    assert inspect.signature(A.ASGLoss.beam_stream).parameters["keep_lattice"].default is False
    sig = inspect.signature(A.BeamStream.result_confidence).parameters
    assert sig["frame_tolerance"].default == 0 and sig["final"].default is False


def _views(_lib, Q=65640, E=2559960, N=40, dtype=None):
    g = _lib.AsgTokenGraph()
    g.Q, g.E, g.N, g.dtype = Q, E, N, _lib.ASG_DTYPE_F32 if dtype is None else dtype
    for n in ("label", "state", "row", "src", "src_label", "start_w", "final_w", "edge_w"):
        setattr(g, n, 256)                                           # never dereferenced here
    gb = _lib.AsgTokenGraphBeam()
    gb.graph = ctypes.pointer(g)
    gb.num_start, gb.max_out = 40, 39
    for n in ("orow", "oarc", "ow", "start_q"):
        setattr(gb, n, 256)
    gl = _lib.AsgTokenGraphBeamLoss()
    gl.beam = ctypes.pointer(gb)
    gl.S, gl.start, gl.next = 1641, 0, 256
    return g, gb, gl


def test_the_state_formula_and_argument_validation_without_gpu():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32, F64 = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64
    g, gb, gl = _views(_lib)
    sb = lambda K, B=64, M=400, dt=F32: int(L.asg_beam_conf_stream_state_bytes(ctypes.byref(gl), B, dt, K, M))
    plain = lambda K, B=64, M=400, dt=F32: int(L.asg_beam_stream_state_bytes(ctypes.byref(gb), B, dt, K, M))
    a = lambda v: (v + 255) // 256 * 256

    def want(K, B=64, M=400, e=4, N=40):
        # the plain stream's slot, then cnt, the emissions, nu, U, A and two rows of beta
        return B * (plain(K, 1, M, F32 if e == 4 else F64) + a(4 * M) + a(e * M * N) + a(4 * M) + a(4 * M * K) + a(e * M * K)
                    + a(2 * e * K))
    for K in (1, 64, 256, 1024, 8192):
        assert sb(K) == want(K) > plain(K)
    assert sb(64, 1, 1) == want(64, 1, 1) and sb(64, 3, 130) == want(64, 3, 130)
    assert sb(0) == 0 and sb(-1) == 0 and sb(8193) == 0              # no beam; above K <= 8192
    assert sb(8, M=0) == 0 and sb(8, M=-5) == 0 and sb(8, B=0) == 0  # max_frames < 1
    assert sb(8, dt=F64) == 0 and sb(8, dt=7) == 0                   # not the graph's dtype
    assert int(L.asg_beam_conf_stream_state_bytes(None, 1, F32, 8, 10)) == 0
    gl.next = None
    assert sb(8) == 0                                                # the loss view's own table
    gl.next = 256
    g64, gb64, gl64 = _views(_lib, dtype=F64)
    assert int(L.asg_beam_conf_stream_state_bytes(ctypes.byref(gl64), 64, F64, 64, 400)) == 64 * (
        int(L.asg_beam_stream_state_bytes(ctypes.byref(gb64), 1, F64, 64, 400)) + 2 * a(1600) + a(8 * 400 * 40) + a(4 * 400 * 64)
        + a(8 * 400 * 64) + a(16 * 64))

    big = 1 << 40
    ref = ctypes.byref(gl)
    reset = lambda K=8, B=2, M=10, state=256, n=big: L.asg_beam_conf_stream_reset(None, ref, B, K, M, state, n, None, 0, None)
    assert reset(K=0) == 1 and reset(M=0) == 1 and reset(B=0) == 1 and reset(state=None) == 1
    assert reset(K=8193) == 2                                        # ASG_ERR_UNSUPPORTED
    assert reset(n=16) == 3 and reset(n=sb(8, 2, 10) - 1) == 3       # ASG_ERR_WORKSPACE: one byte short
    assert reset(n=plain(8, 2, 10)) == 3                             # a plain stream's state is too small
    assert L.asg_beam_conf_stream_reset(None, None, 2, 8, 10, 256, big, None, 0, None) == 1

    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.dtype = 4, 2, 40, F32
    p.inputs = p.transition = 256
    adv = lambda K=8, th=1.0, M=10, state=256, n=big: L.asg_beam_conf_stream_advance(None, ctypes.byref(p), ref, K, th, M, state, n,
                                                                                      0, None)
    assert adv(K=0) == 1 and adv(th=-1.0) == 1 and adv(th=float("nan")) == 1 and adv(M=0) == 1 and adv(state=None) == 1
    assert adv(K=8193) == 2 and adv(n=sb(8, 2, 10) - 1) == 3
    assert L.asg_beam_conf_stream_advance(None, None, ref, 8, 1.0, 10, 256, big, 0, None) == 1
    p.T = -1
    assert adv() == 1                                                # Tc < 0
    p.T, p.N = 4, 39
    assert adv() == 1                                                # not the graph's alphabet
    p.N, p.inputs = 40, None
    assert adv() == 1                                                # a chunk of frames without emissions
    p.T = 0
    assert adv() == 0 and adv(n=16) == 3                             # no frames: nothing launched; the state is still checked
    p.T, p.inputs = 4, 256

    outs = (256,) * 7
    res = lambda K=8, B=2, M=10, state=256, n=big, o=outs: L.asg_beam_conf_stream_result(None, ref, B, K, M, state, n, 1, *o, 0, None)
    assert res(K=0) == 1 and res(M=0) == 1 and res(B=0) == 1 and res(state=None) == 1 and res(K=8193) == 2
    assert res(n=sb(8, 2, 10) - 1) == 3
    for i in range(7):
        assert res(o=outs[:i] + (None,) + outs[i + 1:]) == 1         # every output is required

    nb = lambda K=8, B=2, M=10, n=3: int(L.asg_beam_conf_stream_nbest_work_bytes(ref, B, F32, K, M, n))
    assert nb() == int(L.asg_beam_stream_nbest_work_bytes(ctypes.byref(gb), 2, F32, 8, 10, 3)) > 0
    assert nb(n=0) == 0 and nb(n=8193) == 0 and nb(M=0) == 0
    o9 = (256,) * 9
    nbest = lambda K=8, M=10, state=256, n=big, nn=3, work=256, wn=big, o=o9: L.asg_beam_conf_stream_nbest(
        None, ref, 2, K, M, state, n, 1, nn, work, wn, *o, 0, None)
    assert nbest(nn=0) == 1 and nbest(nn=8193) == 2 and nbest(state=None) == 1 and nbest(work=None) == 1
    assert nbest(n=sb(8, 2, 10) - 1) == 3 and nbest(wn=nb() - 1) == 3

    ts = (ctypes.c_int64 * 2)(40, 1)
    o10 = (256,) * 10
    conf = lambda K=8, B=2, M=10, state=256, n=big, tr=256, st=ts, tol=0, o=o10: L.asg_beam_conf_stream_confidence(
        None, ref, B, K, M, state, n, tr, st, 1, tol, *o, 0, None)
    assert conf(tol=-1) == 1 and conf(tol=65) == 2                   # frame_tolerance in 0 .. 64
    assert conf(K=0) == 1 and conf(M=0) == 1 and conf(B=0) == 1 and conf(K=8193) == 2
    assert conf(state=None) == 1 and conf(tr=None) == 1 and conf(st=None) == 1
    assert conf(n=sb(8, 2, 10) - 1) == 3 and conf(n=plain(8, 2, 10)) == 3
    for i in range(10):
        assert conf(o=o10[:i] + (None,) + o10[i + 1:]) == 1          # every output is required
    assert L.asg_beam_conf_stream_confidence(None, None, 2, 8, 10, 256, big, 256, ts, 1, 0, *o10, 0, None) == 1


def test_public_argument_errors_come_before_any_device_work():
    import torch
    import torch_asg_amd as A
    g = A.TokenGraph.from_ngram(np.log(np.full((6, 6), 1.0 / 6)))
    tr = torch.zeros(5, 5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.BeamStream(tr, g, 2, 10, keep_lattice=True)                # a stream lives on the device
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.ASGLoss(5).beam_stream(g, 2, 10, keep_lattice=True)
    with pytest.raises(ValueError):
        A.BeamStream(tr, g, 2, 0, keep_lattice=True)
    s = A.BeamStream.__new__(A.BeamStream)                           # a stream built without the keyword: no state is touched
    s.keep_lattice = False
    with pytest.raises(RuntimeError, match="keep_lattice"):
        s.result_confidence()
    s.keep_lattice = True
    with pytest.raises(ValueError):
        s.result_confidence(frame_tolerance=-1)
