"""GPU tests (-m gpu) of the exact graph decoder (csrc/asg_decode_graph.hip) and the exact graph loss
(csrc/asg_graph_loss.hip, 5h) at the sizes where their kernels change shape, against the numpy restatements
tests/graph_decode_ref.py (every output bit-identical) and tests/graph_loss_ref.py (the parity rule of
tests/test_hip_graph_loss.py: rtol = atol = 1e-9 in float64, util.assert_close -- scaled 1e-4 -- in float32, the same finiteness
pattern, no NaN):

  * more than 64 utterances on the streaming routes (2 and 3 blocks of 64 lanes, a partial last one);
  * scores without stored alpha (no_grad, or inputs that need no gradient): the two ping-pong rows of the streaming forward;
  * more than 1024 product states on the resident loss route, more than 64 KiB of LDS on both resident routes, the fit limits
    2*Q*e <= 128 KiB and 2*(Q+N)*e <= 128 KiB from both sides, N = 1024 | 1025 on the resident decoder;
  * the default route's edge threshold of the loss from both sides;
  * more labels than product states, automata without any path, no input_lengths, utterance groups inside a wide batch,
    the target walk over more than one block with strided targets, capture and replay with 65 utterances.

The route a call took cannot be seen from Python, so every case runs under the default route and both forcing flags, and first
asserts from the compiled graph's Q and E and the routing rules restated in tests/graph_regime_cases.py that it is in the regime it
names (tests/test_graph_regimes_cpu.py asserts the same without a GPU).  Every loss case passes a non-uniform grad_scores."""
import numpy as np
import pytest
import torch

import graph_regime_cases as C
from graph_loss_ref import target_scores_ref
from util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = C.F32, C.F64
DTYPES = [F32, F64]
LOSS_FLAGS = [0, C.LOSS_STREAM, C.LOSS_RESIDENT]
DEC_FLAGS = [0, C.DEC_STREAM, C.DEC_RESIDENT]
DEC_NAMES = ("scores", "path", "tokens", "token_lengths", "states")


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _native():
    from torch_asg_amd.asg import native
    return native()


def _sizes(name, dtype):
    """Q and E of the compiled graph, which must be those the case table states."""
    c = C.graph(name).compile(DEV, dtype)
    assert (c["Q"], c["E"]) == C.expected(name), name
    return c["Q"], c["E"]


def _loss(x, tr, graph, il, flags, gs, max_work_bytes=1 << 30):
    xd = x.to(DEV).requires_grad_(True)
    td = tr.to(DEV).requires_grad_(True)
    Z = _asg().GraphFullScore.apply(xd, td, graph, None if il is None else il.to(DEV), 1.0, 0.0, max_work_bytes, flags)
    Z.backward(gs.to(DEV, Z.dtype))
    torch.cuda.synchronize()
    return Z.detach().cpu(), xd.grad.cpu(), td.grad.cpu()


def _scaled_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        return float(np.abs(a[fin] - ref[fin]).max() / max(1.0, np.abs(ref[fin]).max()))


def _cmp_loss(got, want, dtype, il, T, what):
    """The rules of tests/test_hip_graph_loss.py::_compare (figures printed first), then the structure: exact zeros behind an
    utterance's length and in the whole column of an utterance without a score."""
    Z, gx, gtr = got
    Zr, gxr, gtrr = want
    fin = np.isfinite(Zr)
    print("%s: scaled max err Z %.3e grad_inputs %.3e grad_transition %.3e" %
          (what, _scaled_err(Z.numpy(), Zr), _scaled_err(gx.numpy(), gxr), _scaled_err(gtr.numpy(), gtrr)))
    assert (np.isfinite(Z.numpy()) == fin).all(), what
    assert (Z.numpy()[~fin] == -np.inf).all(), what
    assert not torch.isnan(gx).any() and not torch.isnan(gtr).any(), what
    if dtype == F64:
        assert np.allclose(Z.numpy()[fin], Zr[fin], rtol=1e-9, atol=1e-9), what
        assert np.allclose(gx.numpy(), gxr, rtol=1e-9, atol=1e-9), what
        assert np.allclose(gtr.numpy(), gtrr, rtol=1e-9, atol=1e-9), what
    else:
        assert_close(Z.numpy()[fin], Zr[fin], what=what + " Z")
        assert_close(gx.numpy(), gxr, what=what + " grad_inputs")
        assert_close(gtr.numpy(), gtrr, what=what + " grad_transition")
    for b in range(gx.shape[1]):
        L = T if il is None else min(max(int(il[b]), 0), T)
        assert (gx[L:, b] == 0).all(), what
        if not (fin[b] and L):
            assert (gx[:, b] == 0).all(), what


def _loss_case(name, T, B, seed, dtype, flags, what, with_lengths=True):
    """Run inputs(T, B, N, seed) through the loss under `flags` and compare with the cached reference -> the GPU result."""
    g = C.graph(name)
    x, tr, il, gs = C.inputs(T, B, g.N, seed, dtype == F64)
    if not with_lengths:
        il = None
    got = _loss(x, tr, g, il, flags, gs)
    _cmp_loss(got, C.loss_reference(name, T, B, seed, dtype == F64, with_lengths), dtype, il, T,
              "%s %s B=%d flags=%d" % (what, str(dtype)[6:], B, flags))
    return got


def _decode(x, tr, graph, il, flags, max_work_bytes=1 << 30):
    out = _native().viterbi_decode_graph(x.to(DEV), tr.to(DEV), graph, None if il is None else il.to(DEV), 1.0, 0.0,
                                         max_work_bytes, flags)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _cmp_decode(got, want, dtype, what):
    assert got[0].dtype == dtype and all(o.dtype == torch.int64 for o in got[1:])
    for name, g, w in zip(DEC_NAMES, got, want):
        assert np.array_equal(g.numpy(), w), "%s %s" % (name, what)


def _decode_case(name, T, B, seed, dtype, flags, what, with_lengths=True):
    g = C.graph(name)
    x, tr, il, _ = C.inputs(T, B, g.N, seed, dtype == F64)
    got = _decode(x, tr, g, il if with_lengths else None, flags)
    _cmp_decode(got, C.decode_reference(name, T, B, seed, dtype == F64, with_lengths), dtype,
                "%s %s B=%d flags=%d" % (what, str(dtype)[6:], B, flags))
    return got


# ---- a, b: more than 64 utterances; the edge threshold of the loss ------------------------------------------------------------

@pytest.mark.parametrize("flags", LOSS_FLAGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [65, 130])
def test_loss_with_more_than_64_utterances(B, dtype, flags):
    """Bigram over 65 tokens, E = 4160 > 4096: the default route streams.  2 and 3 blocks of 64 lanes with a partial last one in
    graph_loss_fwd_frame / _bwd_frame, two and three strides of graph_loss_tr_reduce; lengths 0, 1 and T in the second block."""
    T = 7
    Q, E = _sizes("bigram65", dtype)
    e = C.esize(dtype)
    assert not C.loss_resident(0, e, Q, E) and C.loss_resident(C.LOSS_RESIDENT, e, Q, E)
    il = C.inputs(T, B, 65, 1, dtype == F64)[2]
    assert (B + 63) // 64 >= 2 and B % 64 and C.mixed_parity(il)
    assert {int(il[64])} <= {0, 1, T} and (B < 67 or {0, 1, T} <= set(il[64:128].tolist()))
    _loss_case("bigram65", T, B, 1, dtype, flags, "bigram65")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [65, 130])
def test_decoder_with_more_than_64_utterances(B, dtype):
    """The same inputs through the decoder: graph_frame_kernel's lane mapping and its back-pointers [(t * Q + q) * B + b] under
    the streaming flag (the default here is the resident route, E <= 32768)."""
    T = 7
    Q, E = _sizes("bigram65", dtype)
    assert C.dec_resident(0, C.esize(dtype), 65, Q, E) and not C.dec_resident(C.DEC_STREAM, C.esize(dtype), 65, Q, E)
    outs = [_decode_case("bigram65", T, B, 1, dtype, flags, "bigram65") for flags in DEC_FLAGS]
    for u, v, w in zip(*outs):
        assert torch.equal(u, v) and torch.equal(u, w)


@pytest.mark.parametrize("flags", LOSS_FLAGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["bigram64", "bigram65"])
def test_loss_on_either_side_of_the_edge_threshold(name, dtype, flags):
    """E = 4032 <= 4096: the default route is the resident one; E = 4160: it streams."""
    Q, E = _sizes(name, dtype)
    e = C.esize(dtype)
    assert C.loss_fits(e, Q)
    assert C.loss_resident(0, e, Q, E) == (name == "bigram64") and (E <= C.LOSS_EDGES) == (name == "bigram64")
    _loss_case(name, 7, 5, 3, dtype, flags, name)


# ---- c: scores without stored alpha ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", LOSS_FLAGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [8, 9])
@pytest.mark.parametrize("name", ["bigram65", "trigram40_holes"])
def test_scores_without_stored_alpha(name, T, dtype, flags):
    """Under no_grad, or with inputs that need no gradient, the forward keeps two rows of alpha: the streaming route ping-pongs
    them (frames t >= len must leave an utterance's column alone, graph_loss_fwd_finish reads row (len - 1) & 1), the resident
    route passes no alpha pointer.  B = 70: two blocks of lanes."""
    B = 70
    g = C.graph(name)
    Q, E = _sizes(name, dtype)
    x, tr, il, _ = C.inputs(T, B, g.N, 7, dtype == F64)
    assert C.mixed_parity(il) and int(il.max()) == T and {0, 1, T} <= set(il[64:].tolist())
    Zr = C.loss_reference(name, T, B, 7, dtype == F64)[0]
    fin = np.isfinite(Zr)
    assert fin.sum() * 2 > B
    xd, td, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    GF = _asg().GraphFullScore
    with torch.no_grad():
        z1 = GF.apply(xd.clone().requires_grad_(True), td, g, ild, 1.0, 0.0, 1 << 30, flags)
    z2 = GF.apply(xd, td, g, ild, 1.0, 0.0, 1 << 30, flags)
    z3, saved = _native().graph_full_forward(xd, td, g, ild, 1.0, 0.0, False, 1 << 30, flags)
    torch.cuda.synchronize()
    assert saved is None and not z1.requires_grad and not z2.requires_grad
    for how, z in (("no_grad", z1), ("no gradient needed", z2), ("store=False", z3)):
        what = "%s T=%d %s flags=%d %s" % (name, T, str(dtype)[6:], flags, how)
        z = z.cpu().numpy()
        print("%s: scaled max err Z %.3e" % (what, _scaled_err(z, Zr)))
        assert (np.isfinite(z) == fin).all() and (z[~fin] == -np.inf).all(), what
        if dtype == F64:
            assert np.allclose(z[fin], Zr[fin], rtol=1e-9, atol=1e-9), what
        else:
            assert_close(z[fin], Zr[fin], what=what)
    # the stored-alpha forward computes the same recursion: the same bits
    zs = _loss(x, tr, g, il, flags, torch.ones(B, dtype=F64))[0]
    assert torch.equal(zs, z1.cpu()) and torch.equal(z1, z2) and torch.equal(z1, z3)


# ---- d: more than 1024 product states on the resident loss route ---------------------------------------------------------------

@pytest.mark.parametrize("flags", LOSS_FLAGS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_loss_with_more_than_1024_product_states(dtype, flags):
    """Trigram over 40 tokens with holes, Q = 1633: under the resident flag the q += 1024 loops of graph_loss_fwd_resident /
    _bwd_resident take a second pass and a thread owns the accumulators of two product states.  Twice per route: the same bits
    (the determinism of 5h where one thread owns several accumulators)."""
    Q, E = _sizes("trigram40_holes", dtype)
    e = C.esize(dtype)
    assert C.WG < Q <= 2 * C.WG and C.loss_lds(e, Q) <= C.LDS_PLAIN
    assert C.loss_resident(C.LOSS_RESIDENT, e, Q, E) and not C.loss_resident(0, e, Q, E)
    a = _loss_case("trigram40_holes", 6, 3, 11, dtype, flags, "trigram40_holes")
    b = _loss_case("trigram40_holes", 6, 3, 11, dtype, flags, "trigram40_holes again")
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("flags", [0, C.LOSS_STREAM])
def test_trigram_streams_with_70_utterances(flags):
    """The same graph at B = 70 on the streaming route (which the default takes, E > 4096): two blocks of lanes, a backward grid
    of ceil(1633 / 4) x 2 workgroups."""
    Q, E = _sizes("trigram40_holes", F64)
    assert not C.loss_resident(flags, 8, Q, E)
    il = C.inputs(6, 70, 40, 12, True)[2]
    assert C.mixed_parity(il)
    _loss_case("trigram40_holes", 6, 70, 12, F64, flags, "trigram40_holes")


# ---- e, f: resident launches with more than 64 KiB of LDS ----------------------------------------------------------------------

BIG_LDS = [("enterable600", F64, 5, 3, 4), ("enterable1000", F32, 5, 2, 5)]


@pytest.mark.parametrize("flags", LOSS_FLAGS)
@pytest.mark.parametrize("name,dtype,T,B,seed", BIG_LDS, ids=["f64", "f32"])
def test_loss_with_more_than_64_kib_of_lds(name, dtype, T, B, seed, flags):
    """Random automata with Q = 6059 (float64) and Q = 10093 (float32): the resident kernels have to ask for their dynamic LDS
    (set_lds), 64 KiB < 256 + 2*Q*e <= 128 KiB + 256."""
    Q, E = _sizes(name, dtype)
    e = C.esize(dtype)
    assert C.LDS_PLAIN < C.loss_lds(e, Q) <= 256 + C.VEC_BYTES
    assert C.loss_resident(C.LOSS_RESIDENT, e, Q, E) and not C.loss_resident(0, e, Q, E)
    _loss_case(name, T, B, seed, dtype, flags, name)


@pytest.mark.parametrize("name,dtype,T,B,seed", BIG_LDS, ids=["f64", "f32"])
def test_decoder_with_more_than_64_kib_of_lds(name, dtype, T, B, seed):
    """The same graphs through the decoder: more than 64 KiB of dynamic LDS, and the backtrace stages 4 (float64) or 2 (float32)
    frames of back-pointer rows at a time, so T = 5 takes two or three stages."""
    Q, E = _sizes(name, dtype)
    e, N = C.esize(dtype), C.graph(name).N
    assert C.LDS_PLAIN < C.dec_lds(e, N, Q) <= 160 * 1024
    assert C.dec_resident(C.DEC_RESIDENT, e, N, Q, E) and not C.dec_resident(0, e, N, Q, E)
    assert C.dec_stage_frames(e, N, Q) == (4 if dtype == F64 else 2) and T > C.dec_stage_frames(e, N, Q)
    outs = [_decode_case(name, T, B, seed, dtype, flags, name) for flags in DEC_FLAGS]
    assert np.isfinite(outs[0][0].numpy()[0])
    for u, v, w in zip(*outs):
        assert torch.equal(u, v) and torch.equal(u, w)


# ---- g: the fit limits ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", LOSS_FLAGS)
@pytest.mark.parametrize("name,dtype", [("shift16384", F32), ("shift16385", F32), ("shift8192", F64), ("shift8193", F64)])
def test_loss_at_the_fit_limit(name, dtype, flags):
    """2*Q*e == 128 KiB is the last graph the resident flag keeps resident; with one more product state the flag must fall back
    to the streaming route and still give the reference's result."""
    Q, E = _sizes(name, dtype)
    e = C.esize(dtype)
    fits = name in ("shift16384", "shift8192")
    assert (2 * Q * e == C.VEC_BYTES) if fits else (2 * (Q - 1) * e == C.VEC_BYTES)
    assert C.loss_resident(C.LOSS_RESIDENT, e, Q, E) == fits and not C.loss_resident(0, e, Q, E)
    _loss_case(name, 6, 2, 6, dtype, flags, name)


@pytest.mark.parametrize("name,dtype", [("shift16380", F32), ("shift16381", F32), ("shift8188", F64), ("shift8189", F64)])
def test_decoder_at_the_fit_limit(name, dtype):
    """2*(Q+N)*e == 128 KiB, then one more product state (the resident flag streams)."""
    Q, E = _sizes(name, dtype)
    e = C.esize(dtype)
    fits = name in ("shift16380", "shift8188")
    assert (2 * (Q + 4) * e == C.VEC_BYTES) if fits else (2 * (Q + 3) * e == C.VEC_BYTES)
    assert C.dec_resident(C.DEC_RESIDENT, e, 4, Q, E) == fits
    assert C.dec_resident(0, e, 4, Q, E) == (fits and E <= C.DEC_EDGES)     # (float64: E = 24564, the default stays resident)
    outs = [_decode_case(name, 6, 2, 6, dtype, flags, name) for flags in DEC_FLAGS]
    assert np.isfinite(outs[0][0].numpy()).all()
    for u, v, w in zip(*outs):
        assert torch.equal(u, v) and torch.equal(u, w)


# ---- h: N = 1024 and 1025 on the decoder -------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1024, 1025])
def test_decoder_at_the_alphabet_limit_of_the_resident_route(N):
    """One state, zero weights.  N = 1024 = the resident workgroup: every thread loads an emission and the transition matrix
    (4 MiB) is read from global memory; N = 1025: even the resident flag streams.  Both equal `viterbi_decode`."""
    name = "one_state%d" % N
    Q, E = _sizes(name, F32)
    assert C.dec_resident(C.DEC_RESIDENT, 4, N, Q, E) == (N == 1024) and not C.dec_resident(0, 4, N, Q, E)
    assert C.dec_lds(4, N, Q) == 512 + 4 * N * 4                 # no room for the matrix
    T, B = 4, 2
    outs = [_decode_case(name, T, B, 8, F32, flags, name) for flags in DEC_FLAGS]
    for u, v, w in zip(*outs):
        assert torch.equal(u, v) and torch.equal(u, w)
    x, tr, il, _ = C.inputs(T, B, N, 8, False)
    want = _asg().viterbi_decode(x.to(DEV), tr.to(DEV), il.to(DEV))
    for g, w in zip(outs[2][:4], want):
        assert torch.equal(g, w.cpu())
    assert torch.equal(outs[2][4], torch.where(outs[2][1] >= 0, 0, -1))


# ---- i: more labels than product states ------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", LOSS_FLAGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["cycle3", "cycle3_n14"])
def test_loss_with_more_labels_than_product_states(name, dtype, flags):
    """A 3-state cycle over three tokens of N: Q = 9 < N, so the streaming backward grid is sized by N.  The gradient rows of the
    labels without a product state and every grad_transition entry that is neither a stay nor an edge's label pair are exactly
    0.0.  With N = 12 (tokens 0..2) a grid sized by Q alone (3 workgroups of 4 wavefronts) would still reach every label; with
    N = 14 the cycle moves on the tokens 0, 1 and 13, so label 13 needs a fourth workgroup and its gradient is not zero: a grid
    sized by Q leaves that column unwritten, which no content of the buffer can make right (and the buffers the allocator is
    about to hand out are filled with NaN first)."""
    Q, E = _sizes(name, dtype)
    N = C.graph(name).N
    tokens = list(C.CYCLE_TOKENS[name])
    rest = [i for i in range(N) if i not in tokens]
    assert N > Q and (max(tokens) >= (Q + 3) // 4 * 4) == (name == "cycle3_n14")
    T, B = 6, 66
    il = C.inputs(T, B, N, 9, dtype == F64)[2]
    assert C.mixed_parity(il) and {1, T} <= set(il[64:].tolist())
    gxr = C.loss_reference(name, T, B, 9, dtype == F64)[1]
    assert all((gxr[:, :, i] != 0).any() for i in tokens)
    poison = [torch.full((T, B, N), float("nan"), dtype=dtype, device=DEV) for _ in range(4)]
    torch.cuda.synchronize()
    del poison
    Z, gx, gtr = _loss_case(name, T, B, 9, dtype, flags, name)
    assert np.isfinite(Z.numpy()).sum() * 2 > B
    assert (gx[:, :, rest] == 0).all() and all((gx[:, :, i] != 0).any() for i in tokens)
    used = torch.zeros(N, N, dtype=torch.bool)
    used[np.ix_(tokens, tokens)] = True
    assert (gtr[~used] == 0).all() and (gtr[used] != 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_decoder_with_more_labels_than_product_states(dtype):
    _sizes("cycle3", dtype)
    outs = [_decode_case("cycle3", 6, 66, 9, dtype, flags, "cycle3") for flags in DEC_FLAGS]
    assert (outs[0][1] < 3).all()
    for u, v, w in zip(*outs):
        assert torch.equal(u, v) and torch.equal(u, w)


# ---- j: automata without any accepted path ---------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, C.LOSS_STREAM])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["dead_final", "dead_start", "dead_empty"])
def test_loss_of_automata_without_a_path(name, dtype, flags):
    """No accepting state, no arc at the start state, no arc at all (Q = 0): Z is -inf, the gradients are exact zeros, nothing
    is NaN, and graph_asg_loss is +inf."""
    _sizes(name, dtype)
    g = C.graph(name)
    T, B = 9, 3
    Z, gx, gtr = _loss_case(name, T, B, 10, dtype, flags, name)
    assert (Z == -np.inf).all() and (gx == 0).all() and (gtr == 0).all()
    if flags == 0:
        x, tr, il, _ = C.inputs(T, B, 6, 10, dtype == F64)
        xd, td = x.to(DEV).requires_grad_(True), tr.to(DEV).requires_grad_(True)
        tg = torch.tensor([[1, 2, 3], [0, 0, 4], [5, 1, 1]]).to(DEV)
        loss = _asg().graph_asg_loss(xd, tg, td, g, il.to(DEV), torch.tensor([3, 1, 2]).to(DEV))
        loss.sum().backward()
        torch.cuda.synchronize()
        assert (loss.detach().cpu() == np.inf).all()
        assert not torch.isnan(xd.grad).any() and not torch.isnan(td.grad).any()


# ---- k: no input_lengths ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", LOSS_FLAGS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_loss_without_input_lengths(dtype, flags):
    _sizes("bigram10", dtype)
    _loss_case("bigram10", 6, 65, 13, dtype, flags, "bigram10 no lengths", with_lengths=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_decoder_without_input_lengths(dtype):
    _sizes("bigram10", dtype)
    for flags in DEC_FLAGS:
        _decode_case("bigram10", 6, 65, 13, dtype, flags, "bigram10 no lengths", with_lengths=False)


# ---- l: utterance groups inside a wide batch -------------------------------------------------------------------------------

def _group_sizes(work_bytes, B, budget):
    """The utterance groups of torch_asg_amd/asg.py (_decode_graph, graph_full_forward) for the library's own work_bytes(nb)."""
    gsz = max(1, min(B, budget // max(work_bytes(1), 1)))
    while gsz > 1 and work_bytes(gsz) > budget:
        gsz -= 1
    return [min(B, b0 + gsz) - b0 for b0 in range(0, B, gsz)]


def _library_work_bytes(kind, x, tr, il, g, dtype):
    """nb -> asg_graph_full_work_bytes (stored alpha) or asg_viterbi_decode_graph_work_bytes of nb utterances, asked of the
    library the way torch_asg_amd/asg.py asks."""
    import ctypes
    from torch_asg_amd import _lib, graph as _graph
    L = _lib.lib()
    p, keep = _native()._problem(x.to(DEV), tr.to(DEV), None, il.to(DEV), None)
    if kind == "loss":
        view = _graph.abi_graph_loss(g.compile_loss(DEV, dtype, 1.0, 0.0))
    else:
        view = _graph.abi_graph(g.compile(DEV, dtype, 1.0, 0.0))

    def work_bytes(nb):
        p.B = nb
        if kind == "loss":
            return int(L.asg_graph_full_work_bytes(ctypes.byref(p), ctypes.byref(view), 1))
        return int(L.asg_viterbi_decode_graph_work_bytes(ctypes.byref(p), ctypes.byref(view)))
    work_bytes.keep = (keep, view)
    return work_bytes


def test_loss_groups_of_a_wide_batch():
    """130 utterances in groups of 50, 50 and 30 (from the library's asg_graph_full_work_bytes): Z and grad_inputs equal one
    call bit for bit, grad_transition (a sum over the groups) within 1e-12 as
    tests/test_hip_graph_loss.py::test_small_work_budget_groups_utterances."""
    T, B, Q = 7, 130, 65
    _sizes("bigram65", F64)
    g = C.graph("bigram65")
    x, tr, il, gs = C.inputs(T, B, 65, 1, True)
    work = _library_work_bytes("loss", x, tr, il, g, F64)
    assert work(50) == 50 * T * Q * 8                                   # stored alpha: T * Q * B * e
    budget = work(50)
    groups = _group_sizes(work, B, budget)
    assert groups == [50, 50, 30] and len(groups) >= 3 and all(n % 64 for n in groups)
    one = _loss(x, tr, g, il, 0, gs)
    grouped = _loss(x, tr, g, il, 0, gs, max_work_bytes=budget)
    assert torch.equal(one[0], grouped[0]) and torch.equal(one[1], grouped[1])
    assert torch.allclose(one[2], grouped[2], rtol=1e-12, atol=1e-12)
    _cmp_loss(grouped, C.loss_reference("bigram65", T, B, 1, True), F64, il, T, "bigram65 grouped")


def test_decoder_groups_of_a_wide_batch():
    """The decoder's groups likewise, 46, 46 and 38 from the library's asg_viterbi_decode_graph_work_bytes (the group size is
    the budget over the rounded-up workspace of one utterance): every output equals one call, on every route."""
    T, B, Q = 7, 130, 65
    _sizes("bigram65", F64)
    g = C.graph("bigram65")
    x, tr, il, _ = C.inputs(T, B, 65, 1, True)
    work = _library_work_bytes("decoder", x, tr, il, g, F64)
    assert work(50) == (T * 50 * Q * 4 + 255) // 256 * 256 + 2 * Q * 50 * 8      # back-pointers and two vectors
    budget = work(50)
    groups = _group_sizes(work, B, budget)
    assert groups == [46, 46, 38] and len(groups) >= 3 and all(n % 64 for n in groups)
    for flags in DEC_FLAGS:
        one = _decode(x, tr, g, il, flags)
        grouped = _decode(x, tr, g, il, flags, max_work_bytes=budget)
        for u, v in zip(one, grouped):
            assert torch.equal(u, v)
        _cmp_decode(grouped, C.decode_reference("bigram65", T, B, 1, True), F64, "bigram65 grouped flags=%d" % flags)


# ---- m: the target walk ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_lengths", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_target_walk_over_two_blocks_with_strided_targets(dtype, with_lengths):
    """graph_target_walk with B = 300 (a second block of 256 threads), targets every other column of a wider tensor, with and
    without target_lengths; repeats, sequences the automaton rejects (the cycle moves on tokens 0..2 only) and labels outside
    [0, N)."""
    g = C.graph("cycle3")
    B, S, N = 300, 6, 12
    gen = torch.Generator().manual_seed(14)
    wide = torch.randint(0, 3, (B, 2 * S), generator=gen)
    bad = torch.randint(-2, N + 3, (B, 2 * S), generator=gen)
    rows = torch.rand(B, generator=gen) < 0.4
    cell = torch.rand(B, 2 * S, generator=gen) < 0.2
    wide = torch.where(rows[:, None] & cell, bad, wide)
    wide[5, 2] = wide[5, 0]                                              # a repeat
    wide[299, 0], wide[298, 10] = -1, N                                  # outside [0, N), in the second block
    tg = wide[:, ::2]
    assert tg.shape == (B, S) and tg.stride() == (2 * S, 2)
    tl = torch.randint(0, S + 1, (B,), generator=gen) if with_lengths else None
    want = target_scores_ref(tg.numpy(), None if tl is None else tl.numpy(), g.next, g.weight, g.final, g.start,
                             fold_dt=np.float64 if dtype == F64 else np.float32)
    fin = np.isfinite(want)
    assert 0 < fin[:256].sum() < 256 and 0 < fin[256:].sum() < B - 256   # accepted and rejected ones in both blocks
    x = torch.zeros(1, B, N, dtype=dtype, device=DEV)
    tr = torch.zeros(N, N, dtype=dtype, device=DEV)
    tgd = wide.to(DEV)[:, ::2]
    assert tgd.stride() == (2 * S, 2)
    got = _native().graph_target_scores(x, tr, g, tgd, None if tl is None else tl.to(DEV)).cpu().numpy()
    assert np.array_equal(np.isfinite(got), fin) and (got[~fin] == -np.inf).all()
    if dtype == F64:
        assert np.allclose(got[fin], want[fin], rtol=1e-9, atol=1e-9)
    else:
        assert_close(got[fin], want[fin], what="target walk")


# ---- capture and replay with 65 utterances ---------------------------------------------------------------------------------

def test_capture_and_replay_of_the_streaming_loss_with_65_utterances():
    g = C.graph("bigram65")
    T, B, N = 7, 65, 65
    x, tr, il, gs = C.inputs(T, B, N, 1, False)
    xs = x.to(DEV).requires_grad_(True)
    trd = tr.to(DEV).requires_grad_(True)
    ils, gsd = il.to(DEV), gs.to(DEV, F32)
    GF = _asg().GraphFullScore

    def step():
        xs.grad = None
        trd.grad = None
        Z = GF.apply(xs, trd, g, ils, 1.0, 0.0, 1 << 30, C.LOSS_STREAM)
        Z.backward(gsd)
        return Z
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                           # warm
    torch.cuda.current_stream().wait_stream(s)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        Zc = step()
    x2, tr2, il2, _ = C.inputs(T, B, N, 2, False)
    assert not torch.equal(il, il2)
    with torch.no_grad():
        xs.copy_(x2.to(DEV))
        trd.copy_(tr2.to(DEV))
        ils.copy_(il2.to(DEV))
    cg.replay()
    torch.cuda.synchronize()
    got = (Zc.detach().cpu().clone(), xs.grad.cpu().clone(), trd.grad.cpu().clone())
    want = _loss(x2, tr2, g, il2, C.LOSS_STREAM, gs)
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    _cmp_loss(got, C.loss_reference("bigram65", T, B, 2, False), F32, il2, T, "bigram65 replayed")


def test_capture_and_replay_of_the_streaming_decoder_with_65_utterances():
    g = C.graph("bigram65")
    T, B, N = 7, 65, 65
    x, tr, il, _ = C.inputs(T, B, N, 1, False)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    nat = _native()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nat.viterbi_decode_graph(xd, trd, g, ild, 1.0, 0.0, 1 << 30, C.DEC_STREAM)      # warm: compiles and caches the graph
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        out = nat.viterbi_decode_graph(xd, trd, g, ild, 1.0, 0.0, 1 << 30, C.DEC_STREAM)
    x2, tr2, il2, _ = C.inputs(T, B, N, 2, False)
    xd.copy_(x2.to(DEV))
    trd.copy_(tr2.to(DEV))
    ild.copy_(il2.to(DEV))
    cg.replay()
    torch.cuda.synchronize()
    got = [o.cpu().clone() for o in out]
    for u, v in zip(got, _decode(x2, tr2, g, il2, C.DEC_STREAM)):
        assert torch.equal(u, v)
    _cmp_decode(got, C.decode_reference("bigram65", T, B, 2, False), F32, "bigram65 replayed")
