"""CPU tests of the C ABI and the Python surface of the lattice-keeping word-LM beam stream (asg_beam_word_conf_stream_*,
`torch_asg_amd.BeamWordStream(..., keep_lattice=True)`): the entry points exist and are declared, the size of a state follows the
formula of the header and has no term in the LM, arguments are validated before anything touches a device -- no kernel is
launched here."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from beam_word_cases import arpa_lm, small_lexicon
from test_beam_word_la_cpu import _la
from test_beam_word_loss_cpu import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("asg_beam_word_conf_stream_state_bytes", "asg_beam_word_conf_stream_reset", "asg_beam_word_conf_stream_advance",
         "asg_beam_word_conf_stream_advance_la", "asg_beam_word_conf_stream_result", "asg_beam_word_conf_stream_result_la",
         "asg_beam_word_conf_stream_nbest", "asg_beam_word_conf_stream_nbest_la", "asg_beam_word_conf_stream_confidence",
         "asg_beam_word_conf_stream_confidence_la", "asg_beam_word_conf_stream_nbest_work_bytes")
FIELDS = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths", "word_frames",
          "word_confidences", "normalisers", "frames", "status")


def test_entry_points_are_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS, n
    assert int(L.asg_hip_version()) == _lib.ABI_VERSION == 230           # additions only: the version stays
    for n in ("advance", "result", "nbest", "confidence"):               # the look-ahead view goes behind the LM
        plain = getattr(L, "asg_beam_word_conf_stream_" + n).argtypes
        at = plain.index(ctypes.POINTER(_lib.AsgWordLM)) + 1
        assert getattr(L, "asg_beam_word_conf_stream_%s_la" % n).argtypes == (plain[:at] + [ctypes.POINTER(_lib.AsgWordLookahead)]
                                                                              + plain[at:])
    import torch_asg_amd as A
    assert "BeamWordStreamConfidence" in A.__all__ and A.BeamWordStreamConfidence._fields == FIELDS
    assert set(A.BeamWordStreamResult._fields) <= set(FIELDS)
    assert inspect.signature(A.BeamWordStream.__init__).parameters["keep_lattice"].default is False
    assert inspect.signature(A.ASGLoss.beam_word_stream).parameters["keep_lattice"].default is False
    sig = inspect.signature(A.BeamWordStream.result_confidence).parameters
    assert sig["frame_tolerance"].default == 0 and sig["final"].default is False


def _bytes(L, gb, w, B, dt, K, M, name="asg_beam_word_conf_stream_state_bytes"):
    return int(getattr(L, name)(ctypes.byref(gb), ctypes.byref(w), B, dt, K, M))


def test_the_state_formula_has_no_term_in_the_lm():
    from torch_asg_amd import _lib
    lex = small_lexicon()
    small, big = arpa_lm(5, 2, 1), arpa_lm(5, 3, 1, keep=(1.0, 1.0, 1.0))
    assert big.H > 2 * small.H and big.A > 2 * small.A                   # the LM doubled
    a = lambda v: (v + 255) // 256 * 256                                 # noqa: E731
    N = lex.graph.N
    for dtype, e, dt in ((torch.float32, 4, _lib.ASG_DTYPE_F32), (torch.float64, 8, _lib.ASG_DTYPE_F64)):
        L, _, gb, w, keep = _abi(lex, small, 4, 2, dtype)
        _, _, gb2, w2, keep2 = _abi(lex, big, 4, 2, dtype)
        for B, K, M in ((64, 64, 400), (64, 256, 400), (1, 1, 1), (3, 300, 130), (2, 6816, 5)):
            plain = _bytes(L, gb, w, 1, dt, K, M, "asg_beam_word_stream_state_bytes")
            got = _bytes(L, gb, w, B, dt, K, M)
            assert got == _bytes(L, gb2, w2, B, dt, K, M) > B * plain > 0
            assert got == B * (plain + a(4 * M) + a(e * M * N) + a(4 * M) + a(8 * M * K) + a(e * M * K) + a(2 * e * K))
        other = _lib.ASG_DTYPE_F64 if e == 4 else _lib.ASG_DTYPE_F32
        assert _bytes(L, gb, w, 2, other, 8, 10) == 0 and _bytes(L, gb, w, 2, 7, 8, 10) == 0   # not the graph's dtype
        for bad in ((0, 8, 10), (2, 0, 10), (2, -1, 10), (2, 8, 0), (2, 8, -5), (2, 8193, 10)):
            assert _bytes(L, gb, w, bad[0], dt, bad[1], bad[2]) == 0
        # the beam the lattice pass holds in LDS: the plain stream goes on to 8192
        fits = 8179 if e == 4 else 6816
        assert _bytes(L, gb, w, 1, dt, fits, 3) > 0 and _bytes(L, gb, w, 1, dt, fits + 1, 3) == 0
        assert _bytes(L, gb, w, 1, dt, fits + 1, 3, "asg_beam_word_stream_state_bytes") > 0
        assert int(L.asg_beam_word_conf_stream_state_bytes(None, ctypes.byref(w), 1, dt, 8, 10)) == 0
        assert int(L.asg_beam_word_conf_stream_state_bytes(ctypes.byref(gb), None, 1, dt, 8, 10)) == 0


@pytest.mark.parametrize("with_la", [False, True], ids=["plain", "la"])
def test_every_argument_check_of_every_entry_point(with_la):
    from torch_asg_amd import _lib
    lex, lm = small_lexicon(), arpa_lm(5, 2, 1)
    L, p, gb, w, keep = _abi(lex, lm, 4, 2)
    F32 = _lib.ASG_DTYPE_F32
    la = _la(_lib, S=w.S, H=w.H, A=w.A, levels=1)
    look = (ctypes.byref(la),) if with_la else ()
    sfx = "_la" if with_la else ""
    g, wr = ctypes.byref(gb), ctypes.byref(w)
    big = 1 << 40
    sb = _bytes(L, gb, w, 2, F32, 8, 10)
    plain = _bytes(L, gb, w, 2, F32, 8, 10, "asg_beam_word_stream_state_bytes")
    assert sb > plain > 0
    fits = 8179

    if not with_la:
        reset = lambda K=8, B=2, M=10, state=256, n=big: L.asg_beam_word_conf_stream_reset(None, g, wr, B, K, M, state, n, None, 0,  # noqa: E731
                                                                                           None)
        assert reset(K=0) == 1 and reset(M=0) == 1 and reset(B=0) == 1 and reset(state=None) == 1
        assert reset(K=8193) == 2 and reset(K=fits + 1) == 2             # ASG_ERR_UNSUPPORTED: beyond beam_word_loss_fits
        assert reset(n=16) == 3 and reset(n=sb - 1) == 3 and reset(n=plain) == 3      # one byte short; a plain stream's state
        assert L.asg_beam_word_conf_stream_reset(None, None, wr, 2, 8, 10, 256, big, None, 0, None) == 1
        assert L.asg_beam_word_conf_stream_reset(None, g, None, 2, 8, 10, 256, big, None, 0, None) == 1

    fn = getattr(L, "asg_beam_word_conf_stream_advance" + sfx)
    adv = lambda K=8, th=1.0, M=10, state=256, n=big, pp=ctypes.byref(p), lk=look: fn(None, pp, g, wr, *lk, K, th, M, state, n, 0,  # noqa: E731
                                                                                   None)
    assert adv(K=0) == 1 and adv(th=-1.0) == 1 and adv(th=float("nan")) == 1 and adv(M=0) == 1 and adv(state=None) == 1
    assert adv(K=8193) == 2 and adv(K=fits + 1) == 2 and adv(n=sb - 1) == 3 and adv(n=plain) == 3 and adv(pp=None) == 1
    if with_la:
        assert adv(lk=(None,)) == 1
        la.H += 1
        assert adv() == 1                                                # not this LM's look-ahead
        la.H -= 1
        assert adv(K=0, lk=(None,)) == 1 and adv(K=8193, lk=(None,)) == 2          # the stream's checks come first
    N, inputs = p.N, p.inputs
    p.T = -1
    assert adv() == 1                                                    # Tc < 0
    p.T, p.N = 4, N - 1
    assert adv() == 1                                                    # not the lexicon's alphabet
    p.N, p.inputs = N, None
    assert adv() == 1                                                    # a chunk of frames without emissions
    p.T = 0
    assert adv() == 0 and adv(n=16) == 3                                 # no frames: nothing launched; the state is still checked
    p.T, p.inputs = 4, inputs

    fn_r = getattr(L, "asg_beam_word_conf_stream_result" + sfx)
    outs = (256,) * 10
    res = lambda K=8, B=2, M=10, state=256, n=big, o=outs, lk=look: fn_r(None, g, wr, *lk, B, K, M, state, n, 1, *o, 0, None)  # noqa: E731
    assert res(K=0) == 1 and res(M=0) == 1 and res(B=0) == 1 and res(state=None) == 1
    assert res(K=8193) == 2 and res(K=fits + 1) == 2 and res(n=sb - 1) == 3 and res(n=plain) == 3
    for i in range(10):
        assert res(o=outs[:i] + (None,) + outs[i + 1:]) == 1             # every output is required
    if with_la:
        assert res(lk=(None,)) == 1

    nb = lambda K=8, B=2, M=10, n=3: int(L.asg_beam_word_conf_stream_nbest_work_bytes(g, wr, B, F32, K, M, n))  # noqa: E731
    assert nb() == int(L.asg_beam_word_stream_nbest_work_bytes(g, wr, 2, F32, 8, 10, 3)) > 0
    assert nb(n=0) == 0 and nb(n=8193) == 0 and nb(M=0) == 0 and nb(K=fits + 1) == 0
    fn_n = getattr(L, "asg_beam_word_conf_stream_nbest" + sfx)
    o13 = (256,) * 13
    nbest = lambda K=8, M=10, state=256, n=big, nn=3, work=256, wn=big, o=o13, lk=look: fn_n(  # noqa: E731
        None, g, wr, *lk, 2, K, M, state, n, 1, nn, work, wn, *o, 0, None)
    assert nbest(nn=0) == 1 and nbest(nn=8193) == 2 and nbest(state=None) == 1 and nbest(work=None) == 1 and nbest(K=fits + 1) == 2
    assert nbest(n=sb - 1) == 3 and nbest(wn=nb() - 1) == 3 and nbest(K=0) == 1
    for i in (0, 1, 2, 4, 5, 8, 9, 10, 11, 12):                          # (path, states and lm_states may be null)
        assert nbest(o=o13[:i] + (None,) + o13[i + 1:]) == 1
    for i in (3, 6, 7):                                                  # ... and then the next check is the state's size
        assert nbest(o=o13[:i] + (None,) + o13[i + 1:], n=sb - 1) == 3
    if with_la:
        assert nbest(lk=(None,)) == 1

    fn_c = getattr(L, "asg_beam_word_conf_stream_confidence" + sfx)
    ts = (ctypes.c_int64 * 2)(N, 1)
    o13c = (256,) * 13
    conf = lambda K=8, B=2, M=10, state=256, n=big, tr=256, st=ts, tol=0, o=o13c, lk=look, fin=1: fn_c(  # noqa: E731
        None, g, wr, *lk, B, K, M, state, n, tr, st, fin, tol, *o, 0, None)
    assert conf(tol=-1) == 1 and conf(tol=65) == 2                       # frame_tolerance in 0 .. 64
    assert conf(tol=-1, fin=0) == 1 and conf(tol=65, fin=0) == 2
    assert conf(K=0) == 1 and conf(M=0) == 1 and conf(B=0) == 1 and conf(K=8193) == 2 and conf(K=fits + 1) == 2
    assert conf(state=None) == 1 and conf(tr=None) == 1 and conf(st=None) == 1
    assert conf(n=sb - 1) == 3 and conf(n=plain) == 3                    # one byte short; a plain stream's state
    assert conf(tol=65, n=sb - 1) == 2 and conf(tol=64, n=sb - 1) == 3   # the tolerance comes before the buffers
    for i in range(13):
        assert conf(o=o13c[:i] + (None,) + o13c[i + 1:]) == 1              # every output is required
    if with_la:
        assert conf(lk=(None,)) == 1 and conf(lk=(None,), tol=65) == 1   # the look-ahead comes before the tolerance
    args = (2, 8, 10, 256, big, 256, ts, 1, 0) + o13c + (0, None)
    assert fn_c(None, None, wr, *look, *args) == 1 and fn_c(None, g, None, *look, *args) == 1


def test_public_argument_errors_come_before_any_device_work():
    import torch_asg_amd as A
    lex, lm = small_lexicon(), arpa_lm(5, 2, 1)
    tr = torch.zeros(5, 5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.BeamWordStream(tr, lex, lm, 2, 10, keep_lattice=True)          # a stream lives on the device
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.ASGLoss(5).beam_word_stream(lex, lm, 2, 10, keep_lattice=True)
    with pytest.raises(ValueError):
        A.BeamWordStream(tr, lex, lm, 2, 0, keep_lattice=True)
    s = A.BeamWordStream.__new__(A.BeamWordStream)                       # a stream built without the keyword: no state is touched
    s.keep_lattice = False
    with pytest.raises(RuntimeError, match="keep_lattice"):
        s.result_confidence()
    with pytest.raises(RuntimeError, match="keep_lattice"):
        s.result_confidence(frame_tolerance=-1)
    s.keep_lattice = True
    with pytest.raises(ValueError):
        s.result_confidence(frame_tolerance=-1)
    assert A.BeamWordStream._API == "asg_beam_word_stream"               # the class keeps the plain family; the keyword switches
