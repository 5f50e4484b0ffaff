"""CPU tests of the C ABI and the Python surface of windowed streaming beam decoding with a lexicon and a word LM
(asg_beam_word_window_*, `torch_asg_amd.BeamWordWindowStream`): the entry points exist and are declared, the size of a state
follows the formula of the header and has no term in the LM or in the length of an utterance, arguments are validated before
anything touches a device -- no kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = ("asg_beam_word_window_state_bytes", "asg_beam_word_window_reset", "asg_beam_word_window_advance",
          "asg_beam_word_window_result")


def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in WINDOW:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    assert int(L.asg_hip_version()) == 230 and "#define ASG_HIP_VERSION 230" in src       # additions only
    import torch_asg_amd as A
    for n in ("BeamWordWindowStream", "BeamWordWindowCommit", "BeamWordWindowResult"):
        assert getattr(A, n) is not None and n in A.__all__
    assert hasattr(A.ASGLoss, "beam_word_window_stream")
    assert A.BeamWordWindowCommit._fields == ("path", "states", "lm_states", "tokens", "token_lengths", "words", "word_lengths",
                                              "frames")
    assert A.BeamWordWindowResult._fields == ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words",
                                              "word_lengths", "frames", "committed", "status")
    assert A.BeamWordWindowStream.max_frames is None                 # no host-side frame bound


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


LM_ARRAYS = ("row", "word", "next", "backoff", "lw", "bw", "ew", "word_of_state")


def _lm(_lib, H=20001, A=400000, V=20000, S=60000, dtype=None):
    w = _lib.AsgWordLM()
    w.H, w.A, w.V, w.S, w.start, w.separator = H, A, V, S, 1, 39
    w.dtype = _lib.ASG_DTYPE_F32 if dtype is None else dtype
    for n in LM_ARRAYS:
        setattr(w, n, 256)
    return w


def _bad_lms(_lib):
    for n in LM_ARRAYS:
        m = _lm(_lib)
        setattr(m, n, None)
        yield m
    for kw in (dict(H=0), dict(A=-1), dict(V=0), dict(S=0)):
        yield _lm(_lib, **kw)
    for field, value in (("start", 20001), ("start", -1), ("separator", 40), ("separator", -1)):
        m = _lm(_lib)
        setattr(m, field, value)
        yield m


def test_sizes_and_argument_validation_without_gpu():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32, F64 = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64
    g, gb = _graph(_lib)
    w = _lm(_lib)
    G, LMW = ctypes.byref(gb), ctypes.byref(w)
    sb = lambda K, B=64, W=128, P=32, dt=F32, lm=w: int(L.asg_beam_word_window_state_bytes(G, ctypes.byref(lm), B, dt, K, W, P))
    a = lambda v: (v + 255) // 256 * 256

    def want(K, B=64, W=128, e=4):
        cap = max(K * 40, 40)
        C = 2
        while C < 2 * cap:
            C *= 2
        one_shot = 3 * a(W * K * 4) + 2 * a(C * 8) + a(C * e) + a(cap * e) + a(cap * 8) + a(cap * 4)
        return B * (one_shot + 256 + a(K * (e + 8)))
    for K in (1, 64, 256, 1024, 8192):
        assert sb(K) == want(K)
    assert sb(64, 1, 1, 1) == want(64, 1, 1) and sb(64, 3, 130, 7) == want(64, 3, 130) and sb(3, 2, 7, 7) == want(3, 2, 7)
    assert sb(64, P=1) == sb(64, P=128) == sb(64)                    # the commit period takes no memory
    # the state of a word stream of max_frames = W: the rings are all the back-pointers there are, whatever pos
    assert sb(256) == int(L.asg_beam_word_stream_state_bytes(G, LMW, 64, F32, 256, 128))
    assert sb(256) < int(L.asg_beam_word_stream_state_bytes(G, LMW, 64, F32, 256, 400))
    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.dtype = 128, 64, 40, F32
    p.inputs = p.transition = 256
    one = int(L.asg_beam_decode_words_work_bytes(ctypes.byref(p), G, LMW, 256))
    assert sb(256) == one + 64 * (256 + a(256 * 12))
    # no term in H, A, V or Q: the LM doubled, then a small graph, the same bytes
    assert sb(256, lm=_lm(_lib, H=40002, A=800000, V=40000)) == sb(256)
    g.Q = 100
    assert sb(256) == want(256) and sb(8192) == want(8192) > sb(100)             # and no clamp of the beam to Q
    g.Q = 65640
    assert sb(0) == 0 and sb(-1) == 0 and sb(8193) == 0              # no beam; above beam_size <= 8192
    assert sb(8, W=0) == 0 and sb(8, W=-5) == 0 and sb(8, B=0) == 0
    assert sb(8, P=0) == 0 and sb(8, P=-1) == 0 and sb(8, W=16, P=17) == 0 and sb(8, W=16, P=16) > 0
    assert sb(8, dt=F64) == 0 and sb(8, dt=7) == 0                   # not the graph's dtype
    assert sb(8, lm=_lm(_lib, dtype=F64)) == 0                       # not the LM's dtype
    assert int(L.asg_beam_word_window_state_bytes(None, LMW, 1, F32, 8, 10, 2)) == 0
    assert int(L.asg_beam_word_window_state_bytes(G, None, 1, F32, 8, 10, 2)) == 0
    assert sb(8, lm=_lm(_lib, H=(1 << 25) + 1)) == 0 and sb(8, lm=_lm(_lib, H=1 << 25)) > 0
    g.Q = (1 << 25) + 1
    assert sb(8) == 0
    g.Q = 65640
    # W beyond the bound of asg_beam_window_* (2^30 frames): refused as unsupported, as there
    assert sb(1, 1, (1 << 30) + 1, 1) == 0 and int(L.asg_beam_window_state_bytes(G, 1, F32, 1, (1 << 30) + 1, 1)) == 0
    assert L.asg_beam_window_reset(None, G, 1, 1, (1 << 30) + 1, 1, 256, 1 << 62, None, 0, None) == 2
    assert L.asg_beam_word_window_reset(None, G, LMW, 1, 1, (1 << 30) + 1, 1, 256, 1 << 62, None, 0, None) == 2
    assert L.asg_beam_word_window_reset(None, G, LMW, 1, 1, 1 << 30, 1, 256, 16, None, 0, None) == 3

    big = 1 << 40
    reset = lambda K=8, B=2, W=10, P=2, state=256, n=big, lm=w: L.asg_beam_word_window_reset(
        None, G, ctypes.byref(lm), B, K, W, P, state, n, None, 0, None)
    assert reset(K=0) == 1 and reset(W=0) == 1 and reset(P=0) == 1 and reset(P=11) == 1 and reset(B=0) == 1
    assert reset(state=None) == 1
    assert reset(K=8193) == 2                                        # ASG_ERR_UNSUPPORTED
    assert reset(lm=_lm(_lib, H=(1 << 25) + 1)) == 2 and reset(lm=_lm(_lib, A=1 << 31)) == 2
    assert reset(n=16) == 3 and reset(n=sb(8, 2, 10, 2) - 1) == 3    # ASG_ERR_WORKSPACE
    assert L.asg_beam_word_window_reset(None, None, LMW, 2, 8, 10, 2, 256, big, None, 0, None) == 1
    assert L.asg_beam_word_window_reset(None, G, None, 2, 8, 10, 2, 256, big, None, 0, None) == 1
    assert reset(lm=_lm(_lib, dtype=F64)) == 1
    for m in _bad_lms(_lib):
        assert reset(lm=m) == 1
    m = _lm(_lib, A=0)
    m.word = m.next = m.lw = None
    assert reset(lm=m, n=16) == 3                                    # an LM without arcs needs no arc arrays: only the buffer is short

    p.T, p.B = 4, 2
    outs8 = (256,) * 8
    adv = lambda K=8, th=1.0, W=10, P=2, state=256, n=big, o=outs8, lm=w: L.asg_beam_word_window_advance(
        None, ctypes.byref(p), G, ctypes.byref(lm), K, th, W, P, state, n, *o, 0, None)
    assert adv(K=0) == 1 and adv(th=-1.0) == 1 and adv(th=float("nan")) == 1 and adv(state=None) == 1
    assert adv(W=0) == 1 and adv(P=0) == 1 and adv(P=11) == 1
    assert adv(K=8193) == 2
    assert adv(n=sb(8, 2, 10, 2) - 1) == 3
    for i in range(8):
        assert adv(o=outs8[:i] + (None,) + outs8[i + 1:]) == 1       # every output is required
    assert L.asg_beam_word_window_advance(None, None, G, LMW, 8, 1.0, 10, 2, 256, big, *outs8, 0, None) == 1
    assert L.asg_beam_word_window_advance(None, ctypes.byref(p), None, LMW, 8, 1.0, 10, 2, 256, big, *outs8, 0, None) == 1
    assert L.asg_beam_word_window_advance(None, ctypes.byref(p), G, None, 8, 1.0, 10, 2, 256, big, *outs8, 0, None) == 1
    for m in _bad_lms(_lib):
        assert adv(lm=m) == 1
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
    p.T = 4

    outs = (256,) * 11
    res = lambda K=8, B=2, W=10, P=2, state=256, n=big, o=outs, lm=w: L.asg_beam_word_window_result(
        None, G, ctypes.byref(lm), B, K, W, P, state, n, 1, *o, 0, None)
    assert res(K=0) == 1 and res(W=0) == 1 and res(P=0) == 1 and res(P=11) == 1 and res(B=0) == 1 and res(state=None) == 1
    assert res(K=8193) == 2
    assert res(n=sb(8, 2, 10, 2) - 1) == 3
    assert L.asg_beam_word_window_result(None, None, LMW, 2, 8, 10, 2, 256, big, 1, *outs, 0, None) == 1
    assert L.asg_beam_word_window_result(None, G, None, 2, 8, 10, 2, 256, big, 1, *outs, 0, None) == 1
    for m in _bad_lms(_lib):
        assert res(lm=m) == 1
    for i in range(11):
        assert res(o=outs[:i] + (None,) + outs[i + 1:]) == 1         # every output is required, `committed` included
    # float64 states
    g64, gb64 = _graph(_lib, dtype=F64)
    w64 = _lm(_lib, dtype=F64)
    assert int(L.asg_beam_word_window_state_bytes(ctypes.byref(gb64), ctypes.byref(w64), 64, F64, 64, 128, 32)) == want(64, e=8)
    assert int(L.asg_beam_word_window_state_bytes(ctypes.byref(gb64), LMW, 64, F64, 64, 128, 32)) == 0


def test_public_argument_errors_come_before_any_device_work():
    import torch
    import torch_asg_amd as A
    lex = A.Lexicon([[0], [0, 1], [2]], 4, 3)
    lm = A.WordLM.null(3)
    tr = torch.zeros(4, 4)
    for kw in (dict(beam_size=0), dict(beam_size=4, beam_threshold=-0.5), dict(beam_size=4, beam_threshold=float("nan"))):
        with pytest.raises(ValueError):
            A.BeamWordWindowStream(tr, lex, lm, 2, 10, **kw)
    for args in ((0, 10), (2, 0), (2, 10, 0), (2, 10, 11), (2, 10, -1)):
        with pytest.raises(ValueError):
            A.BeamWordWindowStream(tr, lex, lm, *args)
    with pytest.raises(TypeError):
        A.BeamWordWindowStream(tr, lex.graph, lm, 2, 10)
    with pytest.raises(TypeError):
        A.BeamWordWindowStream(tr, lex, np.zeros(3), 2, 10)
    with pytest.raises(RuntimeError, match="knows"):
        A.BeamWordWindowStream(tr, lex, A.WordLM.null(2), 2, 10)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.BeamWordWindowStream(tr, lex, lm, 2, 10)                   # a stream lives on the device
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.ASGLoss(4).beam_word_window_stream(lex, lm, 2, 10)
    with pytest.raises(RuntimeError):
        A.BeamWordWindowStream(tr, lex, lm, 2, 10, dtype=torch.float16, device="cuda:0")
