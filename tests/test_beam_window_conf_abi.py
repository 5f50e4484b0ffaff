"""CPU tests of the C ABI and the Python surface of the lattice-keeping window stream (asg_beam_conf_window_*,
`torch_asg_amd.BeamWindowStream(..., keep_lattice=True)`): the entry points exist and are declared, the size of a state follows
the formula of the header, arguments are validated before anything touches a device -- no kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("asg_beam_conf_window_state_bytes", "asg_beam_conf_window_reset", "asg_beam_conf_window_advance",
         "asg_beam_conf_window_result", "asg_beam_conf_window_nbest_work_bytes", "asg_beam_conf_window_nbest",
         "asg_beam_conf_window_confidence")


def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    assert int(L.asg_hip_version()) == _lib.ABI_VERSION == 230           # additions only: the version stays
    import inspect
    import torch_asg_amd as A
    assert "BeamWindowConfCommit" in A.__all__ and "BeamWindowConfidence" in A.__all__
    for f in (A.BeamWindowStream.__init__, A.ASGLoss.beam_window_stream):
        sig = inspect.signature(f).parameters
        assert sig["keep_lattice"].default is False and sig["frame_tolerance"].default == 0 and sig["max_chunk"].default is None
    assert inspect.signature(A.BeamWindowStream.result_confidence).parameters["final"].default is False


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
    ref = ctypes.byref(gl)
    sb = lambda K=8, B=64, W=128, P=32, tol=0, C=40, dt=F32: int(L.asg_beam_conf_window_state_bytes(ref, B, dt, K, W, P, tol, C))
    plain = lambda K, B=64, W=128, P=32, dt=F32: int(L.asg_beam_window_state_bytes(ctypes.byref(gb), B, dt, K, W, P))
    a = lambda v: (v + 255) // 256 * 256

    def want(K, B=64, W=128, P=32, tol=0, C=40, e=4, N=40):
        # the plain window's slot; the ring of RW rows: cnt, the emissions, nu, U, A; the attempt log; a beta pair per attempt
        RW, Lg = W + tol + 1 + C, C // P + 1
        return B * (plain(K, 1, W, P, F32 if e == 4 else F64) + a(4 * RW) + a(e * RW * N) + a(4 * RW) + a(4 * RW * K)
                    + a(e * RW * K) + a(24 * Lg) + Lg * a(2 * e * K))
    for K in (1, 64, 256, 1024, 8192):
        assert sb(K) == want(K) > plain(K)
    for W, P, tol, C in ((1, 1, 0, 1), (8, 3, 64, 5), (16, 16, 3, 1), (128, 1, 1, 400)):
        assert sb(64, 3, W, P, tol, C) == want(64, 3, W, P, tol, C)
    assert sb(0) == 0 and sb(-1) == 0 and sb(8193) == 0              # no beam; above K <= 8192
    assert sb(W=0) == 0 and sb(P=0) == 0 and sb(W=8, P=9) == 0 and sb(B=0) == 0
    assert sb(tol=-1) == 0 and sb(tol=65) == 0 and sb(tol=64) > 0    # frame_tolerance in 0 .. 64
    assert sb(C=0) == 0 and sb(C=-3) == 0 and sb(C=1) > 0            # max_chunk >= 1
    assert sb(P=1, C=65534) == want(8, P=1, C=65534) and sb(P=1, C=65535) == 0 and sb(P=2, C=131069) > 0 and sb(P=2, C=131070) == 0
    assert sb(dt=F64) == 0 and sb(dt=7) == 0                         # (above: at most 65535 log entries) not the graph's dtype
    assert int(L.asg_beam_conf_window_state_bytes(None, 1, F32, 8, 8, 2, 0, 4)) == 0
    gl.next = None
    assert sb() == 0                                                 # the loss view's own table
    gl.next = 256
    g64, gb64, gl64 = _views(_lib, dtype=F64)
    e, K, W, P, tol, C = 8, 64, 16, 3, 2, 7
    RW, Lg = W + tol + 1 + C, C // P + 1
    assert int(L.asg_beam_conf_window_state_bytes(ctypes.byref(gl64), 5, F64, K, W, P, tol, C)) == 5 * (
        int(L.asg_beam_window_state_bytes(ctypes.byref(gb64), 1, F64, K, W, P)) + 2 * a(4 * RW) + a(e * RW * 40) + a(4 * RW * K)
        + a(e * RW * K) + a(24 * Lg) + Lg * a(2 * e * K))

    big = 1 << 40
    shape = dict(W=8, P=2, tol=1, C=4)
    need = sb(8, 2, **shape)

    def reset(K=8, B=2, state=256, n=big, **kw):
        s = dict(shape, **kw)
        return L.asg_beam_conf_window_reset(None, ref, B, K, s["W"], s["P"], s["tol"], s["C"], state, n, None, 0, None)
    assert reset(K=0) == 1 and reset(W=0) == 1 and reset(P=9) == 1 and reset(B=0) == 1 and reset(state=None) == 1
    assert reset(tol=-1) == 1 and reset(C=0) == 1 and reset(tol=65) == 2 and reset(K=8193) == 2
    assert reset(P=1, C=65535) == 2                                  # more log entries than the pull's grid has rows
    assert reset(n=16) == 3 and reset(n=need - 1) == 3 and reset(n=plain(8, 2, 8, 2)) == 3
    assert L.asg_beam_conf_window_reset(None, None, 2, 8, 8, 2, 1, 4, 256, big, None, 0, None) == 1

    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.dtype = 4, 2, 40, F32
    p.inputs = p.transition = 256
    o7 = (256,) * 7

    def adv(K=8, th=1.0, state=256, n=big, o=o7, **kw):
        s = dict(shape, **kw)
        return L.asg_beam_conf_window_advance(None, ctypes.byref(p), ref, K, th, s["W"], s["P"], s["tol"], s["C"], state, n, *o, 0,
                                              None)
    assert adv(K=0) == 1 and adv(th=-1.0) == 1 and adv(th=float("nan")) == 1 and adv(W=0) == 1 and adv(state=None) == 1
    assert adv(tol=-1) == 1 and adv(tol=65) == 2 and adv(C=0) == 1 and adv(K=8193) == 2 and adv(n=need - 1) == 3
    assert adv(C=3) == 2                                             # Tc = 4 > max_chunk: ASG_ERR_UNSUPPORTED
    for i in range(7):
        assert adv(o=o7[:i] + (None,) + o7[i + 1:]) == 1             # every output is required
    assert L.asg_beam_conf_window_advance(None, None, ref, 8, 1.0, 8, 2, 1, 4, 256, big, *o7, 0, None) == 1
    p.T = -1
    assert adv() == 1                                                # Tc < 0
    p.T, p.N = 4, 39
    assert adv() == 1                                                # not the graph's alphabet
    p.N, p.inputs = 40, None
    assert adv() == 1                                                # a chunk of frames without emissions
    p.inputs, p.transition = 256, None
    assert adv() == 1
    p.transition = 256

    o8 = (256,) * 8

    def res(K=8, B=2, state=256, n=big, o=o8, **kw):
        s = dict(shape, **kw)
        return L.asg_beam_conf_window_result(None, ref, B, K, s["W"], s["P"], s["tol"], s["C"], state, n, 1, *o, 0, None)
    assert res(K=0) == 1 and res(W=0) == 1 and res(B=0) == 1 and res(state=None) == 1 and res(K=8193) == 2 and res(tol=65) == 2
    assert res(n=need - 1) == 3
    for i in range(8):
        assert res(o=o8[:i] + (None,) + o8[i + 1:]) == 1

    nb = lambda K=8, B=2, n=3, tol=1: int(L.asg_beam_conf_window_nbest_work_bytes(ref, B, F32, K, 8, 2, tol, 4, n))
    assert nb() == int(L.asg_beam_window_nbest_work_bytes(ctypes.byref(gb), 2, F32, 8, 8, 2, 3)) > 0
    assert nb(n=0) == 0 and nb(n=8193) == 0 and nb(tol=65) == 0
    o9 = (256,) * 9
    nbest = lambda state=256, n=big, nn=3, work=256, wn=big: L.asg_beam_conf_window_nbest(
        None, ref, 2, 8, 8, 2, 1, 4, state, n, 1, nn, work, wn, *o9, 0, None)
    assert nbest(nn=0) == 1 and nbest(nn=8193) == 2 and nbest(state=None) == 1 and nbest(work=None) == 1
    assert nbest(n=need - 1) == 3 and nbest(wn=nb() - 1) == 3

    ts = (ctypes.c_int64 * 2)(40, 1)
    o11 = (256,) * 11

    def conf(K=8, B=2, state=256, n=big, tr=256, st=ts, o=o11, **kw):
        s = dict(shape, **kw)
        return L.asg_beam_conf_window_confidence(None, ref, B, K, s["W"], s["P"], s["tol"], s["C"], state, n, tr, st, 1, *o, 0, None)
    assert conf(tol=-1) == 1 and conf(tol=65) == 2 and conf(C=0) == 1
    assert conf(K=0) == 1 and conf(W=0) == 1 and conf(B=0) == 1 and conf(K=8193) == 2
    assert conf(state=None) == 1 and conf(tr=None) == 1 and conf(st=None) == 1
    assert conf(n=need - 1) == 3 and conf(n=plain(8, 2, 8, 2)) == 3
    for i in range(11):
        assert conf(o=o11[:i] + (None,) + o11[i + 1:]) == 1          # every output is required
    assert L.asg_beam_conf_window_confidence(None, None, 2, 8, 8, 2, 1, 4, 256, big, 256, ts, 1, *o11, 0, None) == 1


def test_public_argument_errors_come_before_any_device_work():
    import torch
    import torch_asg_amd as A
    g = A.TokenGraph.from_ngram(np.log(np.full((6, 6), 1.0 / 6)))
    tr = torch.zeros(5, 5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.BeamWindowStream(tr, g, 2, 8, keep_lattice=True)           # a stream lives on the device
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.ASGLoss(5).beam_window_stream(g, 2, 8, keep_lattice=True, frame_tolerance=2, max_chunk=4)
    for kw in (dict(frame_tolerance=-1), dict(max_chunk=0)):
        with pytest.raises(ValueError):
            A.BeamWindowStream(tr, g, 2, 8, keep_lattice=True, **kw)
    s = A.BeamWindowStream.__new__(A.BeamWindowStream)               # a stream built without the keyword: no state is touched
    s.keep_lattice = False
    with pytest.raises(RuntimeError, match="keep_lattice"):
        s.result_confidence()
    s.keep_lattice, s.max_chunk = True, 4
    with pytest.raises(ValueError, match="max_chunk"):
        s.advance(torch.zeros(5, 2, 5))
