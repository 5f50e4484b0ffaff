"""CPU tests of the C ABI and the Python surface of the n-best list of the windowed word-LM beam stream
(asg_beam_word_window_nbest, asg_beam_word_window_nbest_la, `BeamWordWindowStream.result_nbest`): the entry points exist and are
declared, the scratch follows the formula of the header, arguments are validated before anything touches a device -- no kernel is
launched here."""
import ctypes
import os
import re

import pytest

from test_beam_word_la_cpu import _la
from test_beam_word_window_abi import _bad_lms, _graph, _lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("asg_beam_word_window_nbest_work_bytes", "asg_beam_word_window_nbest", "asg_beam_word_window_nbest_la")


def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    assert int(L.asg_hip_version()) == 230 and "#define ASG_HIP_VERSION 230" in src       # additions only
    # behind asg_beam_word_window_result_la, and the two notes that it was missing are gone
    assert src.index("int asg_beam_word_window_result_la(") < src.index("size_t asg_beam_word_window_nbest_work_bytes(")
    assert "Not here: n-best from the window" not in src
    import torch_asg_amd as A
    assert "BeamWordWindowNbest" in A.__all__
    assert A.BeamWordWindowNbest._fields == ("scores", "tokens", "token_lengths", "words", "word_lengths", "num_hyps", "path",
                                             "states", "lm_states", "frames", "committed", "status")
    assert "no n-best" not in A.BeamWordWindowStream.__doc__
    assert len(L.asg_beam_word_window_nbest_la.argtypes) == len(L.asg_beam_word_window_nbest.argtypes) + 1


def _a256(v):
    return (v + 255) // 256 * 256


def test_sizes_and_argument_validation_without_gpu():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32, F64 = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64
    g, gb = _graph(_lib)
    w = _lm(_lib)
    G, LMW = ctypes.byref(gb), ctypes.byref(w)
    wb = lambda K, nbest, B=64, W=128, P=32, dt=F32, lm=w: int(  # noqa: E731
        L.asg_beam_word_window_nbest_work_bytes(G, ctypes.byref(lm), B, dt, K, W, P, nbest))
    for K, nbest, B, W in ((256, 100, 64, 128), (256, 1, 1, 128), (64, 100, 3, 65), (8192, 8192, 2, 7), (1, 5, 2, 1)):
        assert wb(K, nbest, B, W, 1) == B * _a256(W * min(nbest, K) * 4)
    assert wb(256, 10, P=1) == wb(256, 10, P=128)                    # the commit period takes no memory
    g.Q = 100
    assert wb(256, 500) == 64 * _a256(128 * 256 * 4)                 # no clamp of the beam to Q
    g.Q = 65640
    # 0 for whatever the call refuses
    assert wb(256, 0) == 0 and wb(256, -3) == 0 and wb(256, 8193) == 0
    assert wb(0, 1) == 0 and wb(8193, 1) == 0 and wb(8, 1, B=0) == 0 and wb(8, 1, W=0) == 0 and wb(8, 1, dt=F64) == 0
    assert wb(8, 1, P=0) == 0 and wb(8, 1, W=16, P=17) == 0
    assert int(L.asg_beam_word_window_nbest_work_bytes(None, LMW, 1, F32, 8, 10, 2, 1)) == 0
    assert int(L.asg_beam_word_window_nbest_work_bytes(G, None, 1, F32, 8, 10, 2, 1)) == 0
    assert all(wb(8, 1, lm=bad) == 0 for bad in _bad_lms(_lib))
    # the state is not widened for the call
    assert int(L.asg_beam_word_window_state_bytes(G, LMW, 64, F32, 256, 128, 32)) == \
        int(L.asg_beam_word_stream_state_bytes(G, LMW, 64, F32, 256, 128))

    big = 1 << 40
    # scores, path, tokens, token_lengths, states, lm_states, words, word_lengths, num_hyps, frames, committed, status
    outs = (256,) * 12
    sb = int(L.asg_beam_word_window_state_bytes(G, LMW, 2, F32, 8, 10, 2))
    la = _la(_lib, S=w.S, H=w.H)

    def call(K=8, B=2, W=10, P=2, state=256, n=big, nbest=3, work=256, wn=big, o=outs, lm=w, look=None, final=0, graph=G):
        if look is None:
            return L.asg_beam_word_window_nbest(None, graph, ctypes.byref(lm), B, K, W, P, state, n, final, nbest, work, wn, *o, 0,
                                                None)
        return L.asg_beam_word_window_nbest_la(None, graph, ctypes.byref(lm), look, B, K, W, P, state, n, final, nbest, work, wn, *o,
                                               0, None)
    for look in (None, ctypes.byref(la)):
        # anything the _result call refuses: that call's own error
        assert call(K=0, look=look) == 1 and call(W=0, look=look) == 1 and call(P=0, look=look) == 1 and call(P=11, look=look) == 1
        assert call(B=0, look=look) == 1 and call(state=None, look=look) == 1 and call(K=8193, look=look) == 2
        assert all(call(lm=bad, look=look) == 1 for bad in _bad_lms(_lib))
        assert call(n=sb - 1, look=look) == 3
        assert call(graph=None, look=look) == 1
        # the list's own
        assert call(nbest=0, look=look) == 1 and call(nbest=-1, look=look) == 1 and call(nbest=8193, look=look) == 2
        assert call(work=None, look=look) == 1
        need = 2 * _a256(10 * 3 * 4)
        assert wb(8, 3, 2, 10, 2) == need and call(wn=need - 1, look=look) == 3 and call(wn=0, look=look) == 3    # one byte short
        for final in (0, 1):
            for i in range(12):
                if i not in (1, 4, 5):                               # path, states and lm_states may be NULL
                    assert call(o=outs[:i] + (None,) + outs[i + 1:], look=look, final=final) == 1
    # the look-ahead view is checked behind the LM: a NULL one, another dtype, S or H other than the LM's, a NULL array
    L.asg_beam_word_window_nbest_la.argtypes  # (bound: the plain call's with the view behind the LM)
    assert L.asg_beam_word_window_nbest_la(None, G, LMW, None, 2, 8, 10, 2, 256, big, 0, 3, 256, big, *outs, 0, None) == 1
    for bad in (_la(_lib, S=w.S, H=w.H, dtype=F64), _la(_lib, S=w.S + 1, H=w.H), _la(_lib, S=w.S, H=w.H + 1)):
        assert call(look=ctypes.byref(bad)) == 1
    bad = _la(_lib, S=w.S, H=w.H)
    bad.tab = None
    assert call(look=ctypes.byref(bad)) == 1
    assert call(nbest=0, look=ctypes.byref(bad)) == 1 and call(nbest=8193, look=ctypes.byref(bad)) == 2    # (nbest comes first)
    # float64 views
    g64, gb64 = _graph(_lib, dtype=F64)
    w64 = _lm(_lib, dtype=F64)
    assert int(L.asg_beam_word_window_nbest_work_bytes(ctypes.byref(gb64), ctypes.byref(w64), 4, F64, 64, 50, 5, 10)) == \
        4 * _a256(50 * 10 * 4)


def test_public_argument_errors_come_before_any_device_work():
    import torch_asg_amd as A
    cls = A.BeamWordWindowStream
    s = cls.__new__(cls)                                             # a stream whose constructor never ran: nbest is checked first
    for bad in (0, -1):
        with pytest.raises(ValueError, match="nbest"):
            cls.result_nbest(s, bad)
        with pytest.raises(ValueError, match="nbest"):
            cls.result_nbest(s, bad, final=True, return_alignments=True)
    # the growing stream with a look-ahead keeps its raise
    g = A.BeamWordStream.__new__(A.BeamWordStream)
    g.lookahead = object()
    with pytest.raises(NotImplementedError):
        A.BeamWordStream.result_nbest(g, 3)
