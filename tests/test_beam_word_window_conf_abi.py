"""CPU tests of the C ABI of the lattice-keeping word window stream (asg_beam_word_conf_window_*,
`torch_asg_amd.BeamWordWindowStream(..., keep_lattice=True)`): the entry points exist and are bound, the size of a state follows
the formula of the header, and every argument check of the family answers in the header's error order -- no kernel is launched."""
import ctypes

import pytest
import torch

from beam_word_cases import arpa_lm, small_lexicon
from test_beam_word_la_cpu import _la
from test_beam_word_loss_cpu import _abi

NAMES = ("state_bytes", "reset", "advance", "advance_la", "result", "result_la", "nbest_work_bytes", "nbest", "nbest_la",
         "confidence", "confidence_la")


def test_the_state_formula():
    from torch_asg_amd import _lib
    lex, lm = small_lexicon(), arpa_lm(5, 2, 1)
    N = lex.graph.N
    a = lambda v: (v + 255) // 256 * 256                                   # noqa: E731
    for dtype, e, dt in ((torch.float32, 4, _lib.ASG_DTYPE_F32), (torch.float64, 8, _lib.ASG_DTYPE_F64)):
        L, _, gb, w, keep = _abi(lex, lm, 4, 2, dtype)
        assert all(hasattr(L, "asg_beam_word_conf_window_" + n) and "asg_beam_word_conf_window_" + n in _lib.SYMBOLS for n in NAMES)
        assert int(L.asg_hip_version()) == 230                             # additions only
        g, wr = ctypes.byref(gb), ctypes.byref(w)
        for B, K, W, P, tol, C in ((64, 256, 128, 32, 3, 40), (3, 65, 8, 2, 64, 5)):
            RW, Lg = W + tol + 1 + C, C // P + 1
            PW = int(L.asg_beam_word_window_state_bytes(g, wr, 1, dt, K, W, P))
            assert PW > 0 and int(L.asg_beam_word_conf_window_state_bytes(g, wr, B, dt, K, W, P, tol, C)) == B * (
                PW + a(4 * RW) + a(e * RW * N) + a(4 * RW) + a(8 * RW * K) + a(e * RW * K) + a(24 * Lg) + Lg * a(2 * e * K))


@pytest.mark.parametrize("with_la", [False, True], ids=["plain", "la"])
def test_every_argument_check_in_the_error_order_of_the_header(with_la):
    from torch_asg_amd import _lib
    lex, lm = small_lexicon(), arpa_lm(5, 2, 1)
    L, p, gb, w, keep = _abi(lex, lm, 4, 2)
    F32, big, fits = _lib.ASG_DTYPE_F32, 1 << 40, 8179
    la = _la(_lib, S=w.S, H=w.H, A=w.A, levels=1)
    look, sfx = ((ctypes.byref(la),), "_la") if with_la else ((), "")
    g, wr = ctypes.byref(gb), ctypes.byref(w)
    shape = dict(W=8, P=2, tol=1, C=4)
    sh = lambda kw: tuple(dict(shape, **kw)[k] for k in ("W", "P", "tol", "C"))         # noqa: E731
    sb = lambda B=2, K=8, dt=F32, **kw: int(L.asg_beam_word_conf_window_state_bytes(g, wr, B, dt, K, *sh(kw)))   # noqa: E731
    need, plain = sb(), int(L.asg_beam_word_window_state_bytes(g, wr, 2, F32, 8, 8, 2))
    assert need > plain > 0
    # the shape of the state: the plain window's checks, then INVALID, then UNSUPPORTED, then the lattice pass' bound on the beam
    assert sb(B=0) == sb(K=0) == sb(W=0) == sb(P=0) == sb(P=9) == sb(K=8193) == sb(dt=7) == 0
    assert sb(tol=-1) == sb(C=0) == sb(tol=65) == sb(P=1, C=65535) == sb(K=fits + 1) == 0
    assert sb(tol=64) > 0 and sb(P=1, C=65534) > 0 and sb(K=fits) > 0
    assert int(L.asg_beam_word_conf_window_state_bytes(None, wr, 2, F32, 8, 8, 2, 1, 4)) == 0
    assert int(L.asg_beam_word_conf_window_state_bytes(g, None, 2, F32, 8, 8, 2, 1, 4)) == 0

    def common(call):
        """The checks every call of the family starts with, in their order (1 INVALID, 2 UNSUPPORTED, 3 WORKSPACE)."""
        assert call(K=0) == 1 and call(W=0) == 1 and call(P=9) == 1 and call(K=8193) == 2
        assert call(tol=-1) == 1 and call(C=0) == 1 and call(tol=-1, K=8193) == 2         # the window's own checks come first
        assert call(tol=65) == 2 and call(P=1, C=65535) == 2 and call(K=fits + 1) == 2 and call(tol=-1, K=fits + 1) == 1
        assert call(state=None) == 1 and call(n=need - 1) == 3 and call(n=plain) == 3 and call(state=None, n=16) == 1
        if with_la:
            assert call(lk=(None,)) == 1 and call(lk=(None,), tol=65) == 2 and call(lk=(None,), state=None) == 1

    if not with_la:
        reset = lambda K=8, B=2, state=256, n=big, **kw: L.asg_beam_word_conf_window_reset(  # noqa: E731
            None, g, wr, B, K, *sh(kw), state, n, None, 0, None)
        common(reset)
        assert reset(B=0) == 1

    fn_a, o10 = getattr(L, "asg_beam_word_conf_window_advance" + sfx), (256,) * 10
    adv = lambda K=8, th=1.0, state=256, n=big, o=o10, pp=ctypes.byref(p), lk=look, **kw: fn_a(  # noqa: E731
        None, pp, g, wr, *lk, K, th, *sh(kw), state, n, *o, 0, None)
    common(adv)
    assert adv(pp=None) == 1 and adv(th=-1.0) == 1 and adv(th=float("nan")) == 1
    assert adv(C=3) == 2 and adv(C=3, th=-1.0) == 2 and adv(C=3, state=None) == 2       # Tc = 4 > max_chunk, before the rest
    for i in range(10):
        assert adv(o=o10[:i] + (None,) + o10[i + 1:]) == 1 and adv(o=o10[:i] + (None,) + o10[i + 1:], n=16) == 1
    N, inputs, tr = p.N, p.inputs, p.transition
    p.T = -1
    assert adv() == 1 and adv(C=3) == 1                                  # Tc < 0
    p.T, p.N = 4, N - 1
    assert adv() == 1                                                    # not the lexicon's alphabet
    p.N, p.inputs = N, None
    assert adv() == 1                                                    # a chunk of frames without emissions
    p.T, p.transition = 0, None
    assert adv() == 1 and adv(n=16) == 1                                 # the catch-up reads the transition also without frames
    p.T, p.inputs, p.transition = 4, inputs, tr

    fn_r, o11 = getattr(L, "asg_beam_word_conf_window_result" + sfx), (256,) * 11
    res = lambda K=8, B=2, state=256, n=big, o=o11, lk=look, **kw: fn_r(None, g, wr, *lk, B, K, *sh(kw), state, n, 1, *o, 0, None)  # noqa: E731
    common(res)
    for i in range(11):
        assert res(o=o11[:i] + (None,) + o11[i + 1:]) == 1

    nb = lambda n=3, **kw: int(L.asg_beam_word_conf_window_nbest_work_bytes(g, wr, 2, F32, 8, *sh(kw), n))   # noqa: E731
    assert nb() == int(L.asg_beam_word_window_nbest_work_bytes(g, wr, 2, F32, 8, 8, 2, 3)) > 0
    assert nb(n=0) == 0 and nb(n=8193) == 0 and nb(tol=65) == 0 and nb(C=0) == 0
    fn_n, o12 = getattr(L, "asg_beam_word_conf_window_nbest" + sfx), (256,) * 12
    nbest = lambda K=8, state=256, n=big, nn=3, work=256, wn=big, o=o12, lk=look, **kw: fn_n(  # noqa: E731
        None, g, wr, *lk, 2, K, *sh(kw), state, n, 1, nn, work, wn, *o, 0, None)
    common(nbest)
    assert nbest(nn=0) == 1 and nbest(nn=8193) == 2 and nbest(nn=0, tol=65) == 2 and nbest(work=None) == 1
    assert nbest(wn=nb() - 1) == 3 and nbest(n=need - 1, wn=nb() - 1) == 3
    for i in (0, 2, 3, 6, 7, 8, 9, 10, 11):                              # (path, states and lm_states may be null)
        assert nbest(o=o12[:i] + (None,) + o12[i + 1:]) == 1

    fn_c, ts, o14 = getattr(L, "asg_beam_word_conf_window_confidence" + sfx), (ctypes.c_int64 * 2)(N, 1), (256,) * 14
    conf = lambda K=8, B=2, state=256, n=big, tr=256, st=ts, o=o14, lk=look, fin=1, **kw: fn_c(  # noqa: E731
        None, g, wr, *lk, B, K, *sh(kw), state, n, tr, st, fin, *o, 0, None)
    common(conf)
    assert conf(B=0) == 1 and conf(tr=None) == 1 and conf(st=None) == 1 and conf(tr=None, n=16) == 1
    for i in range(14):
        assert conf(o=o14[:i] + (None,) + o14[i + 1:]) == 1              # every output is required
