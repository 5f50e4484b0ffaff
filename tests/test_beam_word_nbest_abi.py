"""CPU tests of the C ABI and the Python surface of the n-best over pairs (asg_beam_decode_words_nbest,
asg_beam_word_stream_nbest, `torch_asg_amd.beam_decode_words_nbest`, `BeamWordStream.result_nbest`): the entry points exist and
are declared, the workspaces follow the formulas of the header and have no term in the LM, arguments are validated before
anything touches a device -- no kernel is launched here."""
import ctypes
import os
import re

import pytest

from test_beam_word_stream_abi import LM_ARRAYS, _graph, _lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("asg_beam_decode_words_nbest_work_bytes", "asg_beam_decode_words_nbest", "asg_beam_word_stream_nbest_work_bytes",
         "asg_beam_word_stream_nbest")


def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in ENTRY:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    assert int(L.asg_hip_version()) == 230 and "#define ASG_HIP_VERSION 230" in src       # additions only
    import torch_asg_amd as A
    for n in ("BeamWordsNbest", "beam_decode_words_nbest", "BeamWordStreamNbest"):
        assert n in A.__all__ and getattr(A, n) is not None
    assert hasattr(A.ASGLoss, "beam_decode_words_nbest") and hasattr(A.BeamWordStream, "result_nbest")
    assert A.BeamWordsNbest._fields == ("scores", "emission_scores", "graph_scores", "lm_scores", "tokens", "token_lengths", "words",
                                        "word_lengths", "num_hyps", "path", "states", "lm_states")
    assert A.BeamWordStreamNbest._fields == ("scores", "graph_scores", "lm_scores", "tokens", "token_lengths", "words",
                                             "word_lengths", "num_hyps", "path", "states", "lm_states", "frames", "status")


def _bad_lms(_lib):
    for n in LM_ARRAYS:
        m = _lm(_lib)
        setattr(m, n, None)
        yield m
    for kw in (dict(H=0), dict(A=-1), dict(V=0), dict(S=0), dict(dtype=_lib.ASG_DTYPE_F64)):
        yield _lm(_lib, **kw)
    for field, v in (("start", 20001), ("start", -1), ("separator", 40), ("separator", -1)):
        m = _lm(_lib)
        setattr(m, field, v)
        yield m


def test_one_shot_sizes_and_argument_validation_without_gpu():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32, F64 = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64
    g, gb = _graph(_lib)
    w = _lm(_lib)
    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.dtype = 400, 64, 40, F32
    p.inputs = p.transition = 256
    wb = lambda K, nb, lm=w: int(L.asg_beam_decode_words_nbest_work_bytes(ctypes.byref(p), ctypes.byref(gb), ctypes.byref(lm), K, nb))
    one = lambda K: int(L.asg_beam_decode_words_work_bytes(ctypes.byref(p), ctypes.byref(gb), ctypes.byref(w), K))
    a = lambda v: (v + 255) // 256 * 256

    def want(K, nb, T=400, B=64, e=4):
        return one(K) + B * (a(8 + K * (e + 8)) + a(T * min(nb, K) * 4)) + 3 * a(B * 8) + a(5 * B * T * 8)
    for K, nb in ((1, 1), (64, 10), (256, 100), (256, 256), (256, 8192), (1024, 1), (8192, 8192)):
        assert wb(K, nb) == want(K, nb), (K, nb)
    assert wb(256, 300) == wb(256, 256)                              # nbest > beam_size adds padding rows, not workspace
    # no term in H, A, V or Q: the LM doubled, then a small graph, the same bytes
    assert wb(256, 10, _lm(_lib, H=40002, A=800000, V=40000)) == wb(256, 10)
    g.Q = 100
    assert wb(256, 10) == want(256, 10)
    g.Q = 65640
    assert wb(256, 0) == 0 and wb(256, -3) == 0 and wb(256, 8193) == 0 and wb(0, 4) == 0 and wb(8193, 4) == 0
    for m in _bad_lms(_lib):
        assert wb(8, 4, m) == 0
    assert int(L.asg_beam_decode_words_nbest_work_bytes(None, ctypes.byref(gb), ctypes.byref(w), 8, 4)) == 0
    assert int(L.asg_beam_decode_words_nbest_work_bytes(ctypes.byref(p), None, ctypes.byref(w), 8, 4)) == 0
    assert int(L.asg_beam_decode_words_nbest_work_bytes(ctypes.byref(p), ctypes.byref(gb), None, 8, 4)) == 0

    big = 1 << 50
    outs = (256,) * 12
    p.T, p.B = 8, 2
    call = lambda K=8, th=1.0, nb=4, work=256, n=big, o=outs, lm=w, pp=p, gg=gb: L.asg_beam_decode_words_nbest(
        None, None if pp is None else ctypes.byref(pp), None if gg is None else ctypes.byref(gg),
        None if lm is None else ctypes.byref(lm), K, th, nb, work, n, *o, 0, None)
    assert call(nb=0) == 1 and call(nb=-1) == 1 and call(nb=8193) == 2
    assert call(K=0) == 1 and call(K=8193) == 2 and call(th=-1.0) == 1 and call(th=float("nan")) == 1 and call(work=None) == 1
    assert call(pp=None) == 1 and call(gg=None) == 1 and call(lm=None) == 1
    assert call(n=wb(8, 4) - 1) == 3 and call(n=16) == 3
    for m in _bad_lms(_lib):
        assert call(lm=m) == 1
    assert call(lm=_lm(_lib, H=(1 << 25) + 1)) == 2
    optional = {4, 7, 8}                                             # path, states, lm_states may be NULL
    for i in range(12):
        rc = call(o=outs[:i] + (None,) + outs[i + 1:], n=16)
        assert rc == (3 if i in optional else 1), i                  # (a NULL optional output passes on to the workspace check)
    p.dtype = F64
    assert call() == 1                                               # not the graph's dtype
    p.dtype = F32
    # float64
    g64, gb64 = _graph(_lib, dtype=F64)
    w64 = _lm(_lib, dtype=F64)
    p.T, p.B, p.dtype = 400, 64, F64
    got = int(L.asg_beam_decode_words_nbest_work_bytes(ctypes.byref(p), ctypes.byref(gb64), ctypes.byref(w64), 64, 10))
    base = int(L.asg_beam_decode_words_work_bytes(ctypes.byref(p), ctypes.byref(gb64), ctypes.byref(w64), 64))
    assert got == base + 64 * (a(8 + 64 * 16) + a(400 * 10 * 4)) + 3 * a(64 * 8) + a(5 * 64 * 400 * 8)


def test_stream_sizes_and_argument_validation_without_gpu():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32, F64 = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64
    g, gb = _graph(_lib)
    w = _lm(_lib)
    a = lambda v: (v + 255) // 256 * 256
    wb = lambda K, nb, B=64, M=400, dt=F32, lm=w: int(L.asg_beam_word_stream_nbest_work_bytes(ctypes.byref(gb), ctypes.byref(lm), B, dt,
                                                                                             K, M, nb))
    for K, nb, B, M in ((1, 1, 1, 1), (64, 10, 64, 400), (256, 256, 3, 130), (256, 8192, 2, 7), (8192, 8192, 1, 5)):
        assert wb(K, nb, B, M) == B * a(M * min(K, nb) * 4)
    assert wb(256, 10, lm=_lm(_lib, H=40002, A=800000, V=40000)) == wb(256, 10)
    assert wb(256, 0) == 0 and wb(256, 8193) == 0 and wb(0, 4) == 0 and wb(8193, 4) == 0 and wb(8, 4, B=0) == 0 and wb(8, 4, M=0) == 0
    assert wb(8, 4, dt=F64) == 0 and wb(8, 4, lm=_lm(_lib, dtype=F64)) == 0
    assert int(L.asg_beam_word_stream_nbest_work_bytes(None, ctypes.byref(w), 1, F32, 8, 10, 4)) == 0
    assert int(L.asg_beam_word_stream_nbest_work_bytes(ctypes.byref(gb), None, 1, F32, 8, 10, 4)) == 0
    sb = int(L.asg_beam_word_stream_state_bytes(ctypes.byref(gb), ctypes.byref(w), 2, F32, 8, 10))
    big = 1 << 50
    outs = (256,) * 13
    call = lambda K=8, B=2, M=10, state=256, n=big, nb=4, work=256, wn=big, o=outs, lm=w, gg=gb: L.asg_beam_word_stream_nbest(
        None, None if gg is None else ctypes.byref(gg), None if lm is None else ctypes.byref(lm), B, K, M, state, n, 1, nb, work, wn,
        *o, 0, None)
    assert call(nb=0) == 1 and call(nb=8193) == 2 and call(K=0) == 1 and call(K=8193) == 2 and call(M=0) == 1 and call(B=0) == 1
    assert call(state=None) == 1 and call(work=None) == 1 and call(gg=None) == 1 and call(lm=None) == 1
    assert call(n=sb - 1) == 3 and call(wn=wb(8, 4, 2, 10) - 1) == 3
    for m in _bad_lms(_lib):
        assert call(lm=m) == 1
    optional = {3, 6, 7}                                             # path, states, lm_states may be NULL
    for i in range(13):
        rc = call(o=outs[:i] + (None,) + outs[i + 1:], wn=16)
        assert rc == (3 if i in optional else 1), i


def test_public_argument_errors_come_before_any_device_work():
    import torch
    import torch_asg_amd as A
    lex = A.Lexicon([[0], [0, 1], [2]], 4, 3)
    lm = A.WordLM.null(3)
    x, tr = torch.zeros(5, 2, 4), torch.zeros(4, 4)
    for nbest in (0, -2):
        with pytest.raises(ValueError, match="nbest"):
            A.beam_decode_words_nbest(x, tr, lex, lm, beam_size=4, nbest=nbest)
        with pytest.raises(ValueError, match="nbest"):
            A.ASGLoss(4).beam_decode_words_nbest(x, lex, lm, beam_size=4, nbest=nbest)
    for kw in (dict(beam_size=0), dict(beam_size=4, beam_threshold=-0.5), dict(beam_size=4, beam_threshold=float("nan"))):
        with pytest.raises(ValueError):
            A.beam_decode_words_nbest(x, tr, lex, lm, nbest=2, **kw)
    with pytest.raises(RuntimeError):
        A.beam_decode_words_nbest(x, tr, lex, lm, beam_size=4, nbest=2)          # CPU tensors: there is no CPU implementation
