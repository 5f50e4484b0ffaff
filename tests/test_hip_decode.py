"""GPU tests (-m gpu) of Viterbi decoding over the full lattice (`torch_asg_amd.viterbi_decode`, csrc/asg_decode.hip): scores,
paths, tokens and token lengths bit-identical to the test-side numpy decoder (tests/decode_ref.py) across both routes, the
exact agreement with the force aligner on the decoded tokens, capture and replay, and the error behaviour."""
import numpy as np
import pytest
import torch

from decode_ref import decode_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _case(T, B, N, seed, dtype=torch.float32, integer=False):
    g = torch.Generator().manual_seed(seed)
    if integer:
        x = torch.randint(-2, 3, (T, B, N), generator=g).to(dtype)
        tr = torch.randint(-1, 2, (N, N), generator=g).to(dtype)
    else:
        x = torch.randn(T, B, N, generator=g, dtype=torch.float64).to(dtype)
        tr = torch.randn(N, N, generator=g, dtype=torch.float64).to(dtype)
    il = torch.randint(0, T + 1, (B,), generator=g)
    il[0] = T
    if B > 1:
        il[1] = 0
    if B > 2:
        il[2] = 1
    return x, tr, il


def _check(x, tr, il, what=""):
    """Decode on the GPU and compare with the reference decoder bit for bit; returns the GPU results (CPU tensors)."""
    out = _asg().viterbi_decode(x.to(DEV), tr.to(DEV), il.to(DEV) if il is not None else None)
    torch.cuda.synchronize()
    sc, path, tok, tl = [o.cpu() for o in out]
    rs, rp, rt, rl = decode_ref(x.numpy(), tr.numpy(), None if il is None else il.numpy())
    assert sc.dtype == x.dtype and path.dtype == tok.dtype == tl.dtype == torch.int64
    assert np.array_equal(sc.numpy(), rs), "scores %s" % what
    assert np.array_equal(path.numpy(), rp), "path %s" % what
    assert np.array_equal(tok.numpy(), rt), "tokens %s" % what
    assert np.array_equal(tl.numpy(), rl), "token_lengths %s" % what
    return sc, path, tok, tl


# (N, T, B): every route boundary -- one wavefront (N <= 64), a workgroup of slices (65..256 in float32, 65..128 in float64),
# the streaming route beyond
SHAPES = [(1, 1000, 96), (2, 300, 96), (40, 1000, 96), (63, 200, 32), (64, 200, 32), (65, 200, 24), (128, 300, 16),
          (256, 200, 8), (257, 100, 8), (1000, 50, 5), (3000, 20, 3)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N,T,B", SHAPES, ids=["N%d" % s[0] for s in SHAPES])
def test_bit_identical_to_the_reference_decoder(N, T, B, dtype):
    x, tr, il = _case(T, B, N, 1000 + N, dtype)
    _check(x, tr, il, "random")
    _check(x, tr, None, "no lengths")


# the streaming route with several utterance groups per frame (float32: 16 utterances per workgroup, float64: 8), and one
# utterance alone on every route
GROUPS = [(300, 100, 20, torch.float32), (1000, 20, 33, torch.float32), (300, 100, 20, torch.float64),
          (1000, 20, 17, torch.float64)]


@pytest.mark.parametrize("N,T,B,dtype", GROUPS, ids=["N%d_B%d_%s" % (g[0], g[2], str(g[3])[6:]) for g in GROUPS])
def test_streaming_route_with_several_utterance_groups(N, T, B, dtype):
    x, tr, il = _case(T, B, N, 2000 + N + B, dtype)
    _check(x, tr, il, "groups")


SINGLE = [(40, 300, torch.float32), (100, 200, torch.float32), (200, 200, torch.float32), (100, 200, torch.float64),
          (300, 60, torch.float32), (1000, 30, torch.float64)]


@pytest.mark.parametrize("N,T,dtype", SINGLE, ids=["N%d_%s" % (g[0], str(g[2])[6:]) for g in SINGLE])
def test_one_utterance(N, T, dtype):
    x, tr, il = _case(T, 1, N, 3000 + N, dtype)
    _check(x, tr, il, "B=1")
    _check(x, tr, torch.tensor([T // 2]), "B=1, shorter")


@pytest.mark.parametrize("N", [3, 40, 200, 300])
def test_integer_inputs_force_ties(N):
    for dtype in (torch.float32, torch.float64):
        x, tr, il = _case(60, 6, N, 77 + N, dtype, integer=True)
        _check(x, tr, il, "ties")


def test_large_alphabet_reduced_cfg5():
    x, tr, il = _case(24, 3, 10000, 5)
    _check(x, tr, il, "N=10000")


@pytest.mark.parametrize("N", [40, 300])
def test_strided_batch_major_inputs(N):
    g = torch.Generator().manual_seed(N)
    xb = torch.randn(5, 70, N, generator=g)                   # [B,T,N] ...
    x = xb.transpose(0, 1)                                    # ... viewed time-major
    assert not x.is_contiguous()
    tr = torch.randn(N, N, generator=g).t()                   # a strided transition too
    il = torch.tensor([70, 0, 1, 33, 69])
    out = _asg().viterbi_decode(xb.to(DEV).transpose(0, 1), tr.to(DEV), il.to(DEV))
    ref = decode_ref(x.numpy(), tr.numpy(), il.numpy())
    for o, r in zip(out, ref):
        assert np.array_equal(o.cpu().numpy(), r)


@pytest.mark.parametrize("N", [40, 100, 500])
def test_masked_labels_and_an_impossible_utterance(N):
    for dtype in (torch.float32, torch.float64):
        x, tr, il = _case(80, 6, N, 3 + N, dtype)
        g = torch.Generator().manual_seed(N)
        x[torch.rand(x.shape, generator=g) < 0.5] = -float("inf")
        il[3] = 80
        x[40, 3, :] = -float("inf")                            # utterance 3: a frame with every label masked
        sc, path, tok, tl = _check(x, tr, il, "masked")
        assert sc[3] == -float("inf") and (path[3] == -1).all() and (tok[3] == -1).all() and tl[3] == 0


@pytest.mark.parametrize("N", [40, 65, 300])
def test_force_aligner_on_the_decoded_tokens_returns_the_decode_score(N):
    A = _asg()
    for dtype in (torch.float32, torch.float64):
        x, tr, il = _case(120, 8, N, 11 + N, dtype)
        xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
        sc, path, tok, tl = A.viterbi_decode(xd, trd, ild)
        asc, pos, labels = A.viterbi_align(xd, tok.clamp(min=0), trd, ild, tl)
        assert torch.equal(asc, sc)                            # same additions along the same path
        ok = tl > 0
        assert torch.equal(labels[ok], path[ok])               # continuous inputs: no ties


def test_module_method_equals_the_functional_form():
    A = _asg()
    x, tr, il = _case(100, 7, 40, 4)
    m = A.ASGLoss(40).to(DEV)
    with torch.no_grad():
        m.transition.copy_(tr)
    a = m.viterbi_decode(x.to(DEV), il.to(DEV))
    b = A.viterbi_decode(x.to(DEV), m.transition, il.to(DEV))
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert not a[0].requires_grad


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
def test_half_inputs_decode_as_their_float32_widening(half):
    A = _asg()
    x, tr, il = _case(90, 5, 40, 8)
    xh = x.to(half).to(DEV)
    a = A.viterbi_decode(xh, tr.to(DEV), il.to(DEV))
    b = A.viterbi_decode(xh.float(), tr.to(DEV), il.to(DEV))
    assert a[0].dtype == torch.float32
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("N", [40, 300])
def test_path_is_invariant_under_log_softmax(N):
    A = _asg()
    x, tr, il = _case(100, 6, N, 21 + N)
    xd = x.to(DEV)
    a = A.viterbi_decode(xd, tr.to(DEV), il.to(DEV))
    b = A.viterbi_decode(torch.log_softmax(xd, dim=-1), tr.to(DEV), il.to(DEV))
    for u, v in zip(a[1:], b[1:]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("N", [40, 1000])
def test_captured_decode_replays_with_fresh_values(N):
    A = _asg()
    T, B = 60, 6
    x, tr, il = _case(T, B, N, 50)
    xs, trs, ils = x.to(DEV), tr.to(DEV), il.to(DEV)
    A.viterbi_decode(xs, trs, ils)                                 # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = A.viterbi_decode(xs, trs, ils)
    for seed in (51, 52):
        x2, _, il2 = _case(T, B, N, seed)
        il2[4] = 0
        xs.copy_(x2.to(DEV))
        ils.copy_(il2.to(DEV))
        g.replay()
        torch.cuda.synchronize()
        eager = A.viterbi_decode(xs, trs, ils)
        for u, v in zip(outs, eager):
            assert torch.equal(u, v)
        ref = decode_ref(x2.numpy(), tr.numpy(), il2.numpy())
        for u, r in zip(outs, ref):
            assert np.array_equal(u.cpu().numpy(), r)


def test_errors():
    A = _asg()
    x, tr, il = _case(10, 2, 5, 0)
    with pytest.raises(RuntimeError):
        A.viterbi_decode(x, tr, il)                                # CPU tensors
    with pytest.raises(RuntimeError):
        A.viterbi_decode(x.to(DEV), torch.zeros(5, 4, device=DEV), il.to(DEV))
    with pytest.raises(RuntimeError):
        A.viterbi_decode(x.to(DEV), tr.double().to(DEV), il.to(DEV))
    with pytest.raises(RuntimeError):
        A.viterbi_decode(x.to(DEV), tr.to(DEV), il[:1].to(DEV))
    with pytest.raises(RuntimeError):
        A.viterbi_decode(x.to(DEV), tr.to(DEV), il.int().to(DEV))
