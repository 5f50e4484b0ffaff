"""GPU tests (-m gpu) of the two tropical-semiring kernels at the sizes where they change shape:
`viterbi_align` (csrc/asg_viterbi.hip) at every kernel and strip edge, under ties, at the 64-frame backtrace blocks, around its
prefetch rings, with -inf, strides, capture and 16-bit emissions; `viterbi_decode` (csrc/asg_decode.hip) in every resident
instantiation, on both sides of both route switches, under ties across slices, at the backtrace and collapse blocks, with
back-pointers above 127 and over the streaming grid.  Adds and compares only: every result is bit-equal to the numpy
restatements (tests/viterbi_ref.py, tests/decode_ref.py) in both dtypes; no tolerance appears.  The inputs and the regime
arithmetic are tests/viterbi_regime_cases.py; tests/test_viterbi_regimes_cpu.py asserts that every case bites."""
import numpy as np
import pytest
import torch

import viterbi_regime_cases as C
from viterbi_ref import labels_of, viterbi_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = pytest.mark.parametrize("dtype", C.DTYPES)


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _equal_align(out, ref, tg, what):
    """scores and positions bit-equal to the restatement; labels = targets gathered at the positions, -1 where they are -1."""
    sc, pos, lab = [o.cpu().numpy() for o in out]
    rs, rp = ref
    assert sc.dtype == rs.dtype and pos.dtype == lab.dtype == np.int64
    assert np.array_equal(sc, rs), "scores %s" % what
    assert np.array_equal(pos, rp), "positions %s: %d frames differ" % (what, (pos != rp).sum())
    assert np.array_equal(lab, labels_of(tg, rp)), "labels %s" % what


def _align(c):
    out = _asg().viterbi_align(_dev(c.x), _dev(c.tg), _dev(c.tr), _dev(c.il), _dev(c.tl))
    torch.cuda.synchronize()
    rs, rp = c.ref()
    _equal_align(out, (rs, rp), c.tg[:, :c.T], repr(c))
    assert (rp[np.arange(c.T)[None, :] >= np.minimum(c.il, c.T)[:, None]] == -1).all()           # -1 behind the length
    return out


# ---- the aligner -------------------------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("S", C.KERNEL_S)
def test_align_every_kernel_on_both_sides_of_its_edges(S, dtype):
    c = C.kernel_case(S, dtype)
    want = ("small", 1) if S <= 64 else ("wide", 1 if S <= 1024 else (4 if S <= 4096 else 8))
    assert (c.kernel.kind, c.kernel.KP) == want and c.kernel.nw == (S + 63) // 64
    assert (c.T, c.B) == (S + 3, 3) and list(c.tl[:2]) == [S, 1]
    _align(c)


@DT
@pytest.mark.parametrize("S", C.SINGLE_S)
def test_align_a_single_alignment(S, dtype):
    c = C.kernel_case(S, dtype, True)
    assert c.T == S == c.tl[0]
    sc, pos, lab = _align(c)
    assert pos[0].tolist() == list(range(S))


@DT
@pytest.mark.parametrize("T,S", C.TIE_TS, ids=["S%d" % s for _, s in C.TIE_TS])
def test_align_ties_keep_stay(T, S, dtype):
    c = C.align_tie_case(T, S, dtype)
    assert c.kernel == C.align_kernel(S) and float(np.abs(c.x).max()) == 2 and float(np.abs(c.tr).max()) == 1
    _align(c)


@DT
@pytest.mark.parametrize("T,S", C.CHUNK_TS, ids=["S%d" % s for _, s in C.CHUNK_TS])
def test_align_lengths_at_the_backtrace_blocks_and_strip_words(T, S, dtype):
    c = C.chunk_case(T, S, dtype)
    assert list(c.il) == C.chunk_lengths(T) and c.kernel.kind == ("small" if S <= 64 else "wide")
    _align(c)


@DT
def test_align_lengths_around_the_prefetch_rings(dtype):
    for c, PF in ((C.ring_case(20, dtype, 0), 16), (C.ring_case(20, dtype, 1), 16), (C.ring_case(300, dtype), 8),
                  (C.ring_case(1025, dtype), 2)):
        assert c.kernel.PF == PF
        _align(c)


@DT
@pytest.mark.parametrize("S", C.INF_S)
def test_align_masked_emissions(S, dtype):
    c = C.inf_case(S, dtype)
    assert c.kernel.kind == "wide"
    sc, pos, lab = _align(c)
    assert torch.isfinite(sc[:3]).all()
    assert sc[3] == -float("inf") and bool((pos[3] == -1).all()) and bool((lab[3] == -1).all())


@DT
@pytest.mark.parametrize("S", C.HOST_S)
def test_align_strided_emissions_transition_and_targets(S, dtype):
    c = C.host_case(S, dtype)
    xb = _dev(c.x.transpose(1, 0, 2))                          # [B,T,N] storage ...
    x = xb.transpose(0, 1)                                     # ... viewed time-major
    tr = _dev(c.tr.T).t()                                      # a transposed transition
    wide = torch.full((c.B, 2 * c.S), -7, dtype=torch.int64, device=DEV)
    wide[:, ::2] = _dev(c.tg)
    tg = wide[:, ::2]                                          # every second column of a wider tensor
    assert not x.is_contiguous() and not tr.is_contiguous() and not tg.is_contiguous()
    out = _asg().viterbi_align(x, tg, tr, _dev(c.il), _dev(c.tl))
    torch.cuda.synchronize()
    _equal_align(out, c.ref(), c.tg, repr(c))


@DT
@pytest.mark.parametrize("S", C.HOST_S)
def test_align_captured_call_replays_with_fresh_values(S, dtype):
    A = _asg()
    c = C.host_case(S, dtype)
    xs, tgs, trs, ils, tls = _dev(c.x), _dev(c.tg), _dev(c.tr), _dev(c.il), _dev(c.tl)
    A.viterbi_align(xs, tgs, trs, ils, tls)                    # warm call outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = A.viterbi_align(xs, tgs, trs, ils, tls)
    for seed in (1, 2):
        c2 = C.host_case(S, dtype, seed)
        xs.copy_(_dev(c2.x))
        tgs.copy_(_dev(c2.tg))
        ils.copy_(_dev(c2.il))
        tls.copy_(_dev(c2.tl))
        g.replay()
        torch.cuda.synchronize()
        eager = A.viterbi_align(xs, tgs, trs, ils, tls)
        for u, v in zip(outs, eager):
            assert torch.equal(u, v)
        _equal_align(outs, viterbi_ref(c2.x, c2.tg, c.tr, c2.il, c2.tl), c2.tg, "replay %d of %r" % (seed, c))


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@DT
@pytest.mark.parametrize("S", C.HOST_S)
def test_align_16_bit_emissions_as_their_widening(S, dtype, half):
    A = _asg()
    c = C.host_case(S, dtype)
    xh = _dev(c.x).to(half)
    wide = xh.to(getattr(torch, dtype))
    tg, tr, il, tl = _dev(c.tg), _dev(c.tr), _dev(c.il), _dev(c.tl)
    a = A.viterbi_align(xh, tg, tr, il, tl)
    b = A.viterbi_align(wide, tg, tr, il, tl)
    assert a[0].dtype == tr.dtype                              # scores in the transition's dtype
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    _equal_align(a, viterbi_ref(wide.cpu().numpy(), c.tg, c.tr, c.il, c.tl), c.tg, "%s of %r" % (half, c))


# ---- the decoder -------------------------------------------------------------------------------------------------------------------
def _decode(c):
    """Decode on the GPU; the four outputs bit-equal to decode_ref.  Returns them (device tensors)."""
    out = _asg().viterbi_decode(_dev(c.x), _dev(c.tr), _dev(c.il))
    torch.cuda.synchronize()
    ref = c.ref()
    assert out[0].cpu().numpy().dtype == ref[0].dtype
    for o, r, name in zip(out, ref, ("scores", "path", "tokens", "token_lengths")):
        got = o.cpu().numpy()
        assert np.array_equal(got, r), "%s of %r: %d entries differ" % (name, c, (got != r).sum())
    return out


def _route_of(N, dtype):
    e = C.elem_of(dtype)
    if N <= 64:
        return ("res", (N + 7) // 8 * 8, 1)
    if N <= 128:
        return ("res", 64, 2)
    if N <= 256 and e == 4:
        return ("res", 64, 4)
    return ("str", (N + 63) // 64 * 64)


@pytest.mark.parametrize("integer", [False, True], ids=["rand", "int"])
@DT
@pytest.mark.parametrize("N", C.INSTANCE_N)
def test_decode_every_instantiation_and_both_route_switches(N, dtype, integer):
    A = _asg()
    c = C.instance_case(N, dtype, integer)
    r = c.route
    assert _route_of(N, dtype) == (("res", r.NP, r.KS) if isinstance(r, C.Resident) else ("str", r.PAD))
    assert (c.T, c.B) == (70, 4) and list(c.il) == [70, 0, 1, 64]
    sc, path, tok, tl = _decode(c)
    # the aligner on the decoded tokens returns the decode score bit for bit (the same additions along the same path)
    x, tr, il = _dev(c.x), _dev(c.tr), _dev(c.il)
    asc, pos, lab = A.viterbi_align(x, tok.clamp(min=0), tr, il, tl)
    assert torch.equal(asc, sc)
    if not integer:                                            # continuous emissions: no ties, the alignment IS the path
        ok = tl > 0
        assert torch.equal(lab[ok], path[ok])


@pytest.mark.parametrize("dtype,N", [(d, n) for d in C.DTYPES for n in C.SLICE_TIE_N[d]],
                         ids=["%s_N%d" % (d, n) for d in C.DTYPES for n in C.SLICE_TIE_N[d]])
def test_decode_ties_across_slices(dtype, N):
    c = C.slice_tie_case(N, dtype)
    assert isinstance(c.route, C.Resident) and c.route.KS == (2 if N <= 128 else 4)
    _decode(c)


@DT
@pytest.mark.parametrize("N", C.BLOCK_N)
def test_decode_lengths_at_the_backtrace_and_collapse_blocks(N, dtype):
    c = C.block_case(N, dtype)
    assert list(c.il) == list(C.BLOCK_LENGTHS) and c.T == 130
    sc, path, tok, tl = _decode(c)
    path = path.cpu().numpy()
    for b in range(c.B):
        assert np.array_equal(path[b, :c.il[b]], c.schedule[b, :c.il[b]])


def test_decode_uint8_back_pointers_above_127():
    c = C.uint8_case()
    assert c.route == (64, 4, False, 1024)
    _decode(c)


@pytest.mark.parametrize("N", C.STREAM_N)
@pytest.mark.parametrize("dtype,B", [(d, b) for d in C.DTYPES for b in C.STREAM_B[d]],
                         ids=["%s_B%d" % (d, b) for d in C.DTYPES for b in C.STREAM_B[d]])
def test_decode_streaming_grid(N, dtype, B):
    c = C.stream_case(N, B, dtype)
    r = c.route
    assert isinstance(r, C.Streaming) and r.nrt == (5 if N == 257 else 9)
    assert r.UB == (8 if dtype == "float64" else (4 if B <= 4 else (8 if B <= 8 else 16))) and r.ngr == -(-B // r.UB)
    _decode(c)
