"""CPU tests of Viterbi decoding over the full lattice: the test-side reference decoder (tests/decode_ref.py) against exhaustive
path enumeration and the oracle, and the C ABI of asg_viterbi_decode (sizes, argument checks) -- no kernel is launched here."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from decode_ref import decode_ref, path_score
from oracle import asg_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enumerate(x_b, tr, L):
    """(best score, every label sequence that reaches it) over all N^L paths, scored in the kernels' order."""
    N = x_b.shape[1]
    best, arg = -np.inf, []
    for p in itertools.product(range(N), repeat=L):
        s = path_score(x_b, tr, p)
        if s > best:
            best, arg = s, [p]
        elif s == best and s > -np.inf:
            arg.append(p)
    return best, arg


def _collapse(p):
    return [int(v) for i, v in enumerate(p) if i == 0 or p[i - 1] != v]


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_decoder_against_exhaustive_enumeration(seed, dtype):
    rng = np.random.default_rng(500 + seed)
    for _ in range(25):
        T, B, N = int(rng.integers(1, 7)), int(rng.integers(1, 4)), int(rng.integers(1, 5))
        x = rng.normal(size=(T, B, N)).astype(dtype)
        tr = rng.normal(size=(N, N)).astype(dtype)
        if rng.random() < 0.4:                                   # masked labels
            x[rng.random(size=x.shape) < 0.3] = -np.inf
        il = rng.integers(0, T + 1, size=B)
        il[0] = T
        if B > 1:
            il[1] = rng.choice([0, 1])
        sc, path, tok, tl = decode_ref(x, tr, il)
        for b in range(B):
            L = int(il[b])
            assert (path[b, L:] == -1).all()
            if L == 0:
                assert sc[b] == -np.inf and (path[b] == -1).all() and tl[b] == 0 and (tok[b] == -1).all()
                continue
            best, arg = _enumerate(x[:, b], tr, L)
            if best == -np.inf:
                assert sc[b] == -np.inf and (path[b] == -1).all() and tl[b] == 0 and (tok[b] == -1).all()
                continue
            assert sc[b] == best
            p = tuple(int(v) for v in path[b, :L])
            assert p in arg
            assert path_score(x[:, b], tr, p) == sc[b]
            c = _collapse(p)
            assert tl[b] == len(c) and list(tok[b, :len(c)]) == c and (tok[b, len(c):] == -1).all()


def test_reference_decoder_tie_rule_by_hand():
    # everything zero: every path ties; the smallest index wins at the end and at every back-pointer -> all label 0
    x = np.zeros((4, 1, 3), np.float32)
    sc, path, tok, tl = decode_ref(x, np.zeros((3, 3), np.float32))
    assert sc[0] == 0 and list(path[0]) == [0, 0, 0, 0] and list(tok[0]) == [0, -1, -1, -1] and tl[0] == 1
    # frame 0 prefers label 2, frame 1 ties labels 1 and 2 (score 3 either way with these moves): smallest index -> 1
    x = np.array([[0, 0, 1], [0, 2, 2]], np.float64)[:, None, :]
    tr = np.zeros((3, 3))
    sc, path, tok, tl = decode_ref(x, tr)
    assert sc[0] == 3 and list(path[0]) == [2, 1] and list(tok[0]) == [2, 1] and tl[0] == 2
    # the back-pointer tie: label 1 at the last frame is reached from 0 (score 1 + 1) and from 2 (score 1 + 1): take 0
    x = np.array([[1, -5, 1], [-9, 0, -9]], np.float64)[:, None, :]
    tr = np.array([[0, 0, 0], [1, 0, 1], [0, 0, 0]], np.float64)
    sc, path, tok, tl = decode_ref(x, tr)
    assert sc[0] == 2 and list(path[0]) == [0, 1]
    # a repeated label collapses; the collapse is of consecutive frames only
    x = np.array([[5, 0], [5, 0], [0, 5], [5, 0]], np.float64)[:, None, :]
    sc, path, tok, tl = decode_ref(x, np.zeros((2, 2)))
    assert list(path[0]) == [0, 0, 1, 0] and list(tok[0]) == [0, 1, 0, -1] and tl[0] == 3
    # an all -inf frame: no finite path
    x = np.zeros((3, 1, 2))
    x[1] = -np.inf
    sc, path, tok, tl = decode_ref(x, np.zeros((2, 2)))
    assert sc[0] == -np.inf and (path == -1).all() and (tok == -1).all() and tl[0] == 0


@pytest.mark.parametrize("seed", range(4))
def test_reference_decoder_against_the_oracle(seed):
    rng = np.random.default_rng(900 + seed)
    T, B, N, S = 30, 5, 7, 6
    x = rng.normal(size=(T, B, N))
    tr = rng.normal(size=(N, N))
    il = rng.integers(S, T + 1, size=B)
    sc, path, tok, tl = decode_ref(x, tr, il)
    # the best path over the full lattice beats the best alignment of any transcript ...
    tg = rng.integers(0, N, size=(B, S))
    ali = orc.viterbi(x, tg, tr, il, np.full(B, S))[0]
    assert (sc >= ali).all()
    # ... and IS the best alignment of its own tokens (same additions along the same path: exactly equal)
    tl_c = np.maximum(tl, 1)
    own = orc.viterbi(x, np.where(tok >= 0, tok, 0), tr, il, tl_c)[0]
    assert (own == sc).all()
    # ... and never beats the log-sum over all paths (float64, a few ulps of slack)
    full = orc.full_forward(x, tr, il)[0]
    assert (sc <= full + 4 * np.spacing(np.abs(full))).all()


# ---- the C ABI: no kernel is launched -------------------------------------------------------------------------------------
def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(asg_[a-z_]+)\s*\(", src))


def test_header_and_library_declare_and_export_the_decoder():
    from torch_asg_amd import _lib
    names = _declared_symbols()
    assert {"asg_viterbi_decode", "asg_viterbi_decode_work_bytes"} <= names
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "asg_viterbi_decode") and hasattr(L, "asg_viterbi_decode_work_bytes")
    assert {"asg_viterbi_decode", "asg_viterbi_decode_work_bytes"} <= set(_lib.SYMBOLS)


def _problem(T, B, N, dtype):
    from torch_asg_amd import _lib
    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.S = T, B, N, 0
    p.dtype = dtype
    p.inputs, p.transition = 16, 16          # never dereferenced: only sizes / checks
    return p


def _expected_work(T, B, N, e):
    resident = N <= (256 if e == 4 else 128)
    if resident:
        return B * T * N
    P = (N + 63) // 64 * 64
    return (P * P * e + 255) // 256 * 256 + T * B * P * e


@pytest.mark.parametrize("T,B,N", [(400, 64, 40), (7, 3, 1), (100, 5, 128), (50, 2, 200), (60, 4, 256), (64, 4, 257),
                                   (400, 64, 1000), (2000, 32, 10000)])
def test_decode_work_bytes_follow_the_documented_formula(T, B, N):
    from torch_asg_amd import _lib
    L = _lib.lib()
    for dt, e in ((_lib.ASG_DTYPE_F32, 4), (_lib.ASG_DTYPE_F64, 8)):
        p = _problem(T, B, N, dt)
        assert L.asg_viterbi_decode_work_bytes(ctypes.byref(p)) == _expected_work(T, B, N, e)


def test_decode_argument_validation():
    from torch_asg_amd import _lib
    L = _lib.lib()
    p = _problem(10, 2, 40, _lib.ASG_DTYPE_F32)
    assert L.asg_viterbi_decode_work_bytes(None) == 0
    assert L.asg_viterbi_decode(None, None, None, 0, None, None, None, None, 0, None) == 1
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.addressof(buf)
    # null output / work buffers
    assert L.asg_viterbi_decode(None, ctypes.byref(p), None, 1 << 12, a, a, a, a, 0, None) == 1
    assert L.asg_viterbi_decode(None, ctypes.byref(p), a, 1 << 12, None, a, a, a, 0, None) == 1
    assert L.asg_viterbi_decode(None, ctypes.byref(p), a, 1 << 12, a, None, a, a, 0, None) == 1
    assert L.asg_viterbi_decode(None, ctypes.byref(p), a, 1 << 12, a, a, None, a, 0, None) == 1
    assert L.asg_viterbi_decode(None, ctypes.byref(p), a, 1 << 12, a, a, a, None, 0, None) == 1
    # a workspace one byte short
    need = L.asg_viterbi_decode_work_bytes(ctypes.byref(p))
    assert need == 10 * 2 * 40
    assert L.asg_viterbi_decode(None, ctypes.byref(p), a, need - 1, a, a, a, a, 0, None) == 3
    # bad dtype, empty shapes, no emissions
    p.dtype = 7
    assert L.asg_viterbi_decode_work_bytes(ctypes.byref(p)) == 0
    assert L.asg_viterbi_decode(None, ctypes.byref(p), a, 1 << 12, a, a, a, a, 0, None) == 1
    p = _problem(0, 2, 40, _lib.ASG_DTYPE_F32)
    assert L.asg_viterbi_decode(None, ctypes.byref(p), a, 1 << 12, a, a, a, a, 0, None) == 1
    p = _problem(10, 2, 40, _lib.ASG_DTYPE_F32)
    p.inputs = None
    assert L.asg_viterbi_decode(None, ctypes.byref(p), a, 1 << 12, a, a, a, a, 0, None) == 1


def test_decode_sizes_beyond_the_loss_state_limits():
    # the loss refuses T*B*N*e >= 4 GiB on the small path (32-bit state offsets); decoding keeps no such state: T*B*N bytes
    from torch_asg_amd import _lib
    L = _lib.lib()
    p = _problem(100000, 20000, 40, _lib.ASG_DTYPE_F32)
    assert L.asg_viterbi_decode_work_bytes(ctypes.byref(p)) == 100000 * 20000 * 40
    p = _problem(10, 2, (1 << 22) + 1, _lib.ASG_DTYPE_F32)
    assert L.asg_viterbi_decode_work_bytes(ctypes.byref(p)) == 0
