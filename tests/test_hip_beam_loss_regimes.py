"""GPU tests (-m gpu) of the beam-pruned ASG loss (csrc/asg_beam_loss.hip) at the sizes where its kernels
change shape, against the numpy restatement tests/beam_loss_ref.py with the parity rule of tests/test_hip_beam_loss.py
(util.assert_close, scaled 1e-4 in float32; rtol = atol = 1e-9 in float64):

  * wide lattices: one lane per state above 512 states, several passes over a frame above 1024, also while the kernel walks
    U_{t-1} instead of a long CSR row (the root of a lexicon trie);
  * more than 64 KiB of LDS in the set / forward / backward kernels;
  * alphabets whose (i, j) count tile passes 64 KiB of LDS, leaves LDS for the utterance's scratch, and N = 1024;
  * the fixed-point scale of the tile across the steps of ceil(log2(len)) and at 3000 frames;
  * 2048 forced positions, odd targets, and the refusals at the limits.

A test cannot see which kernel instantiation ran, so every case first asserts FROM THE REFERENCE'S OWN OUTPUT (the U_t it
returns, the set sizes of its search) and from the restated launch arithmetic below that its inputs are in the regime it is
meant for.  Every case passes a non-uniform grad_scores."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from beam_loss_cases import DEV, INF, _asg, _case, _compare, _full, _lexicon, _ngram, _one_state
from beam_loss_ref import beam_loss_ref
from util import assert_close

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
DTYPES = [F32, F64]

# ---- the launch arithmetic of csrc/asg_beam_loss.hip, restated for the preconditions ------------------------------------
WG = 1024                     # kBL: lanes of a forward / backward workgroup
LDS_MAX = 160 * 1024          # kBLLds
LDS_PLAIN = 64 * 1024         # above this a launch has to ask for its dynamic LDS
HEAD = 256                    # kBLHead


def _subgroup(m):
    """Lanes per state of a frame with m states (subgroup())."""
    G = 1
    while G < 64 and G * 2 * m <= WG:
        G *= 2
    return G


def _bwd_lds(e, M, N, tile):
    """bwd_lds(): reduction slots, beta and U_t of a frame, a frame's label posteriors and -- `tile` -- the [N][N] counts."""
    return HEAD + ((M * (e + 4) + 15) & ~15) + N * 8 + (N * N * 8 if tile else 0)


def _esize(dtype):
    return 8 if dtype == F64 else 4


# ---- helpers ---------------------------------------------------------------------------------------------------------

def _reference(x, tr, graph, il, K, th=INF, gs=None, tg=None, tl=None):
    """-> ((Z, grad_inputs, grad_transition), U, info) of tests/beam_loss_ref.py."""
    np_ = lambda t: None if t is None else t.numpy()
    info = {}
    Z, gx, gtr, U = beam_loss_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start, np_(il), K, th, 1.0,
                                  0.0, np_(tg), np_(tl), np_(gs), info)
    return (Z, gx, gtr), U, info


def _widest(U):
    return max([int(a.size) for u in U for a in u] + [0])


def _check(got, want, dtype, il, what):
    """The parity rule plus the structural checks of tests/test_hip_beam_loss.py: -inf where the reference has it, no NaN
    (both in _compare), exact zeros behind an utterance's length and in the whole row of an utterance without a score."""
    _compare(got, want, dtype, what)
    Z, gx, _ = got
    for b in range(gx.shape[1]):
        L = min(max(int(il[b]), 0), gx.shape[0])
        assert (gx[L:, b] == 0).all(), what
        if not (np.isfinite(float(Z[b])) and L):
            assert (gx[:, b] == 0).all(), what


def _weights(B):
    return torch.linspace(-1.0, 2.0, B, dtype=F64) if B > 1 else torch.tensor([1.5], dtype=F64)


def _plain_targets(B, S, N, seed, tl):
    g = torch.Generator().manual_seed(seed)
    tg = torch.randint(0, N, (B, S), generator=g)
    if S >= 2:
        tg[0, 1] = tg[0, 0]                                # a repeat in the target
    return tg, torch.tensor(tl)


@functools.lru_cache(maxsize=None)
def _trigram40():
    return _ngram(40, 3, 11)                               # Q = 40 + 40 * 40 = 1640


@functools.lru_cache(maxsize=None)
def _fourgram40():
    return _ngram(40, 4, 9)                                # Q = 65640


@functools.lru_cache(maxsize=None)
def _wide_trie():
    return _lexicon(40, 4000, 9, maxlen=3)                 # more than 1024 word ends: the in-degree of (root, separator)


# ---- 1: wide lattices ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [600, 1200, 1640])
def test_wide_lattice_against_reference(K, dtype):
    """Dense trigram over 40 tokens.  K = 600: one lane per state (more than 512 states in a frame), one pass; K = 1200 and
    K = Q = 1640: more than 1024 states in a frame, so the k0 loops of beam_loss_fwd / beam_loss_bwd take a second pass."""
    graph = _trigram40()
    assert graph.compile_host(np.float32)["Q"] == 1640
    T, B = 12, 4
    x, tr, il = _case(T, B, 40, 31, dtype)                 # lengths T, 0, 1 and a random one
    assert int(il[0]) == T and int(il[1]) == 0 and int(il[2]) == 1
    gs = _weights(B)
    tg, tl = _plain_targets(B, 6, 40, 3, [6, 0, 1, 3])
    sizes_inf = {}
    for th in (INF, 9.0 if K == 600 else 10.0):           # (thresholds that cut some frames and leave others at K)
        for tgt in (None, (tg, tl)):
            a, b = tgt if tgt else (None, None)
            what = "trigram40 %s K=%d th=%s targets=%s" % (dtype, K, th, tgt is not None)
            want, U, info = _reference(x, tr, graph, il, K, th, gs, a, b)
            widest = _widest(U)
            sizes = [r["sizes"] for r in info["search"]]
            print("%s: max |U_t| = %d, |A_t| = %s" % (what, widest, sizes))
            # the regime, from the reference's own lattice
            assert widest > 512 and _subgroup(widest) == 1, what
            if K == 600:
                assert widest <= WG, what                  # one pass
            else:
                assert widest > WG, what                   # a second pass of k0
            if th == INF:
                sizes_inf[tgt is not None] = sizes
                assert max(sizes[0]) == min(K, 1600), what     # (the 40 states behind the padding context live at t = 0 only)
            else:                                          # the threshold really cut a frame
                assert sizes != sizes_inf[tgt is not None], what
            _check(_full(x, tr, graph, il, K, th, gs=gs, tg=a, tl=b), want, dtype, il, what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_whole_beam_equals_the_exact_route(dtype):
    """K = Q = 1640 without a threshold: scores, losses and both gradients of the GPU's exact route (graph_full_score /
    graph_asg_loss), in frames of 1600 live states (two passes of k0, one lane per state)."""
    A = _asg()
    graph = _trigram40()
    Q = graph.compile_host(np.float32)["Q"]
    assert Q > WG
    T, B = 12, 4
    x, tr, il = _case(T, B, 40, 32, dtype)
    tg, tl = _plain_targets(B, 6, 40, 5, [6, 0, 1, 3])
    _, U, _ = _reference(x, tr, graph, il, Q, INF, None, tg, tl)
    assert _widest(U) > WG                                 # the frames really take a second pass
    w = _weights(B).to(DEV, dtype)
    dv = lambda t: t.to(DEV)
    Za = A.beam_graph_full_score(dv(x), dv(tr), graph, dv(il), beam_size=Q).cpu()
    Zb = A.graph_full_score(dv(x), dv(tr), graph, dv(il)).cpu()
    outs = []
    for fn in (lambda a, b: A.beam_graph_asg_loss(a, dv(tg), b, graph, dv(il), dv(tl), beam_size=Q),
               lambda a, b: A.graph_asg_loss(a, dv(tg), b, graph, dv(il), dv(tl))):
        xd, td = dv(x).requires_grad_(True), dv(tr).requires_grad_(True)
        l = fn(xd, td)
        (torch.where(torch.isfinite(l), l, torch.zeros_like(l)) * w).sum().backward()
        outs.append((l.detach().cpu(), xd.grad.cpu(), td.grad.cpu()))
    (la, ga, ta), (lb, gb, tb) = outs
    assert torch.equal(torch.isinf(Za), torch.isinf(Zb)) and not torch.isnan(Za).any()
    assert torch.equal(torch.isinf(la), torch.isinf(lb)) and not torch.isnan(la).any()
    assert not torch.isnan(ga).any() and not torch.isnan(ta).any()
    fz, fin = torch.isfinite(Zb), torch.isfinite(lb)
    assert fz.any() and fin.any()
    if dtype == F64:
        assert torch.allclose(Za[fz], Zb[fz], rtol=1e-9, atol=1e-9)
        assert torch.allclose(la[fin], lb[fin], rtol=1e-9, atol=1e-9)
        assert torch.allclose(ga, gb, rtol=1e-9, atol=1e-9) and torch.allclose(ta, tb, rtol=1e-9, atol=1e-9)
    else:
        assert_close(Za[fz].numpy(), Zb[fz].numpy(), what="Z")
        assert_close(la[fin].numpy(), lb[fin].numpy(), what="loss")
        assert_close(ga.numpy(), gb.numpy(), what="grad_inputs")
        assert_close(ta.numpy(), tb.numpy(), what="grad_transition")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [600, 1200])
def test_wide_lattice_walks_the_kept_set_at_a_trie_root(K, dtype):
    """A lexicon trie whose (root, separator) state has more than 1024 incoming edges, one per word end.  With K below that
    in-degree the forward kernel walks U_{t-1} and searches the row (by_row == false); K = 600 does so with one lane per state,
    K = 1200 in a frame of more than 1024 states, that is together with a second pass of k0."""
    graph = _wide_trie()
    h = graph.compile_host(np.float64)
    deg = np.diff(h["row"])
    root = int(deg.argmax())
    indeg = int(deg[root])
    assert indeg > WG and K < indeg and h["Q"] > K
    T, B = 12, 3
    x, tr, il = _case(T, B, 40, 7, dtype)
    gs = _weights(B)
    tg, tl = _plain_targets(B, 4, 40, 2, [4, 0, 1])
    for tgt in (None, (tg, tl)):
        a, b = tgt if tgt else (None, None)
        what = "trie %s K=%d targets=%s" % (dtype, K, tgt is not None)
        want, U, info = _reference(x, tr, graph, il, K, INF, gs, a, b)
        # a frame t >= 1 that holds the root while the row is longer than |U_{t-1}|, and how wide such a frame gets
        hit = [len(u[t]) for u in U for t in range(1, len(u)) if root in u[t] and indeg > len(u[t - 1]) > 0]
        print("%s: in-degree %d, frames that walk U_{t-1}: %d, widest of them %d" % (what, indeg, len(hit), max(hit + [0])))
        assert hit and max(hit) > (WG if K > WG else 512), what
        _check(_full(x, tr, graph, il, K, gs=gs, tg=a, tl=b), want, dtype, il, what)


# ---- 2: more than 64 KiB of LDS ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,K", [(F32, 8192), (F32, 8188), (F64, 5600)])
def test_large_lds_against_reference(dtype, K):
    """Dense 4-gram over 40 tokens (Q = 65640), S = 4 forced positions: M = K + 4 states per frame need more than 64 KiB in
    beam_loss_fwd / beam_loss_bwd.  K = 8192 in float32 (M = 8196) also makes beam_loss_sets sort 16384 slots, exactly 64 KiB
    of dynamic LDS beside its static word; K = 8188 (M = 8192) sorts 8192."""
    graph = _fourgram40()
    T, B, S = 5, 2, 4
    e = _esize(dtype)
    M = K + min(S, T)
    assert M * (e + 4) > 65280                             # HEAD + M * (e + 4) > 64 KiB: the forward asks for its LDS
    assert _bwd_lds(e, M, 40, True) > LDS_PLAIN and _bwd_lds(e, M, 40, True) <= LDS_MAX
    P2 = 1 << (M - 1).bit_length()
    if K == 8192:
        assert 8192 < M <= 10240 and P2 * 4 == LDS_PLAIN
    elif K == 8188:
        assert M == 8192 and P2 == 8192
    x, tr, _ = _case(T, B, 40, 17, dtype)
    il = torch.tensor([5, 4])
    gs = torch.tensor([1.5, -0.5], dtype=F64)
    tg = torch.tensor([[3, 17, 17, 30], [8, 1, 25, 12]])
    tl = torch.tensor([4, 3])
    what = "4-gram %s K=%d" % (dtype, K)
    want, U, info = _reference(x, tr, graph, il, K, INF, gs, tg, tl)
    widest = _widest(U)
    print("%s: M = %d, max |U_t| = %d, |A_t| = %s" % (what, M, widest, [r["sizes"] for r in info["search"]]))
    assert widest >= K and widest * (e + 4) > 65280, what   # the frames really are that wide
    _check(_full(x, tr, graph, il, K, gs=gs, tg=tg, tl=tl), want, dtype, il, what)


def test_a_beam_above_8192_is_still_refused():
    A = _asg()
    graph = _fourgram40()
    x, tr, _ = _case(5, 2, 40, 17, F32)
    tg = torch.tensor([[3, 17, 17, 30], [8, 1, 25, 12]])
    with pytest.raises(RuntimeError, match="status 2"):
        A.beam_graph_full_score(x.to(DEV), tr.to(DEV), graph, beam_size=8193, targets=tg.to(DEV))
    with pytest.raises(RuntimeError, match="status 2"):
        A.beam_graph_asg_loss(x.to(DEV), tg.to(DEV), tr.to(DEV), graph, beam_size=8193)


# ---- 3: alphabet size and the (i, j) count tile ------------------------------------------------------------------------

# bwd_lds(e, M, N, true) = 256 + align16(M * (e + 4)) + 8 N + 8 N^2 <= 160 KiB = 163840 keeps the tile in LDS.  With
# M = K + S <= 68 the lattice part is at most 816 bytes, so N = 142 (8 * 142^2 + 8 * 142 = 162448) stays in LDS for both
# dtypes and both K, and N = 143 (8 * 143^2 + 8 * 143 = 164736) does not: beam_loss_bwd<R, false>, integer atomics into the
# utterance's global scratch.  The tile alone passes 64 KiB from N = 91 (8 * 91^2 = 66248): the large-LDS <R, true> launch.
TILE_N = [91, 128, 142, 143, 200, 512]
TILE_LAST_IN_LDS = 142


def _tile_graph(kind, N):
    return _one_state(N) if kind == "one_state" else _ngram(N, 2, N)


def _tile_regime(dtype, K, S, N):
    e, M = _esize(dtype), K + S
    in_lds = _bwd_lds(e, M, N, True) <= LDS_MAX
    assert in_lds == (N <= TILE_LAST_IN_LDS)
    assert N * N * 8 > LDS_PLAIN and _bwd_lds(e, M, N, False) <= LDS_MAX
    return in_lds


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,N", [("bigram", n) for n in TILE_N] + [("one_state", n) for n in TILE_N + [1024]])
def test_count_tile_against_reference(kind, N, dtype):
    graph = _tile_graph(kind, N)
    T, B, S = 10, 4, 4
    x, tr, il = _case(T, B, N, 100 + N, dtype)
    gs = _weights(B)
    tg, tl = _plain_targets(B, S, N, N, [4, 0, 1, 2])
    for K, th in ((16, INF), (64, 4.0)):
        in_lds = _tile_regime(dtype, K, S, N)
        what = "%s N=%d %s K=%d th=%s tile in LDS=%s" % (kind, N, dtype, K, th, in_lds)
        want, U, info = _reference(x, tr, graph, il, K, th, gs, tg, tl)
        assert max(info["search"][0]["sizes"]) > 1 and 1 < _widest(U) <= K + S, what
        assert np.isfinite(want[0][0]) and np.abs(want[2]).max() > 0, what       # the tile is not empty
        _check(_full(x, tr, graph, il, K, th, gs=gs, tg=tg, tl=tl), want, dtype, il, what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", TILE_N + [1024])
def test_one_state_whole_beam_equals_asg_loss(N, dtype):
    """The one-state automaton with zero weights accepts every label path with score 0: with K >= N the loss and both of its
    gradients are those of ASGLoss(reduction='none') on the same inputs."""
    A = _asg()
    graph = _one_state(N)
    T, B, S = 10, 4, 4
    e, M = _esize(dtype), N + S                            # (M = N + 4 here: the tile leaves LDS a little earlier)
    assert (_bwd_lds(e, M, N, True) <= LDS_MAX) == (N <= 128) and _bwd_lds(e, M, N, False) <= LDS_MAX
    x, tr, _ = _case(T, B, N, 200 + N, dtype)
    il = torch.tensor([10, 7, 1, 5])
    tg, tl = _plain_targets(B, S, N, N + 1, [4, 3, 1, 2])
    w = _weights(B).to(DEV, dtype)
    dv = lambda t: t.to(DEV)
    m = A.ASGLoss(N, reduction="none").to(DEV)
    if dtype == F64:
        m = m.double()
    with torch.no_grad():
        m.transition.copy_(tr)
    xa = dv(x).requires_grad_(True)
    la = m(xa, dv(tg), dv(il), dv(tl))
    (la * w).sum().backward()
    xb, tb = dv(x).requires_grad_(True), dv(tr).requires_grad_(True)
    lb = A.beam_graph_asg_loss(xb, dv(tg), tb, graph, dv(il), dv(tl), beam_size=N)
    (lb * w).sum().backward()
    torch.cuda.synchronize()
    la, lb = la.detach().cpu(), lb.detach().cpu()
    ga, gb, ta, tb_ = xa.grad.cpu(), xb.grad.cpu(), m.transition.grad.cpu(), tb.grad.cpu()
    assert torch.isfinite(la).all() and torch.isfinite(lb).all()
    assert not torch.isnan(gb).any() and not torch.isnan(tb_).any()
    for b in range(B):
        assert (gb[int(il[b]):, b] == 0).all()
    if dtype == F64:
        assert torch.allclose(lb, la, rtol=1e-9, atol=1e-9)
        assert torch.allclose(gb, ga, rtol=1e-9, atol=1e-9) and torch.allclose(tb_, ta, rtol=1e-9, atol=1e-9)
    else:
        assert_close(lb.numpy(), la.numpy(), what="loss")
        assert_close(gb.numpy(), ga.numpy(), what="grad_inputs")
        assert_close(tb_.numpy(), ta.numpy(), what="grad_transition")


def test_groups_accumulate_into_a_tile_in_scratch_bit_for_bit(monkeypatch):
    """N = 200 keeps the tile in global scratch.  One utterance per group (max_work_bytes = 1: four groups, so
    ASG_FLAG_BEAM_LOSS_ACCUMULATE is used) gives the bits of the single call, run to run, and captured and replayed with new
    emissions, lengths and targets."""
    N, K, S, T, B = 200, 16, 4, 10, 4
    assert not _tile_regime(F32, K, S, N)
    graph = _ngram(N, 2, N)
    x, tr, il = _case(T, B, N, 8, F32)
    tg, tl = _plain_targets(B, S, N, 1, [4, 0, 1, 2])
    gs = _weights(B).float()
    be = _asg().asg.native()
    forward, groups = be.beam_graph_full_forward, []

    def counted(*a, **k):
        r = forward(*a, **k)
        groups.append(len(r[1]))
        return r
    monkeypatch.setattr(be, "beam_graph_full_forward", counted)
    one = _full(x, tr, graph, il, K, 4.0, gs=gs, tg=tg, tl=tl)
    assert torch.isfinite(one[0][0]) and one[2].abs().max() > 0
    runs = [_full(x, tr, graph, il, K, 4.0, gs=gs, tg=tg, tl=tl, max_work_bytes=1) for _ in range(2)]
    assert groups == [1, B, B]                             # one group, then one utterance per group
    for r in runs:
        for u, v in zip(one, r):
            assert torch.equal(u, v)
    # capture and replay, grouped
    xs = x.to(DEV).requires_grad_(True)
    trd = tr.to(DEV).requires_grad_(True)
    ils, tgs, tls, gsd = il.to(DEV), tg.to(DEV), tl.to(DEV), gs.to(DEV)
    F = _asg().BeamGraphFullScore

    def step():
        xs.grad = None
        trd.grad = None
        Z = F.apply(xs, trd, graph, ils, K, 4.0, 1.0, 0.0, tgs, tls, 1)
        assert groups[-1] == B
        (torch.where(torch.isfinite(Z), Z, torch.zeros_like(Z)) * gsd).sum().backward()
        return Z
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        Zc = step()
    x2, _, il2 = _case(T, B, N, 9, F32)
    tg2, tl2 = _plain_targets(B, S, N, 5, [3, 0, 1, 4])
    with torch.no_grad():
        xs.copy_(x2.to(DEV))
        ils.copy_(il2.to(DEV))
        tgs.copy_(tg2.to(DEV))
        tls.copy_(tl2.to(DEV))
    cg.replay()
    torch.cuda.synchronize()
    got = (Zc.detach().cpu().clone(), xs.grad.cpu().clone(), trd.grad.cpu().clone())
    fin = torch.isfinite(got[0])
    want = _full(x2, tr, graph, il2, K, 4.0, gs=fin.float() * gs, tg=tg2, tl=tl2)
    for u, v in zip(got, want):
        assert torch.equal(u, v)


def test_a_batch_of_65536_utterances_is_one_call():
    """beam_loss_sets has the utterances in grid x and the frames strided over y, so B has no limit of its own (with the frames
    in x and the utterances in y, B > 65535 was a launch error).  Forward only: two different utterances (lengths 2 and 1)
    alternate over B = 65 536, T = 2, N = 2, the one-state automaton, K = 1, float32.  The whole batch's workspace is
    188 743 680 bytes (asg_beam_graph_full_work_bytes for these sizes, Q = 2, num_start = 2, max_out = 1; at T = 2 the same
    with and without the stored alphas), given as max_work_bytes: one group."""
    B, T, N, K, WORK = 65536, 2, 2, 1, 188743680
    graph = _one_state(N)
    x2, tr, _ = _case(T, 2, N, 3, F32)
    il2 = torch.tensor([2, 1])
    be = _asg().asg.native()

    def run(nb, max_work_bytes):
        x = x2.repeat(1, nb // 2, 1).contiguous().to(DEV)
        Z, saved = be.beam_graph_full_forward(x, tr.to(DEV), graph, il2.repeat(nb // 2).to(DEV), K, store=True,
                                              max_work_bytes=max_work_bytes)
        torch.cuda.synchronize()
        return Z.cpu().view(torch.int32), saved                # the bits
    Z, saved = run(B, WORK)
    assert len(saved) == 1 and saved[0][:2] == (0, B) and saved[0][2].numel() == WORK
    small, _ = run(2, 1 << 30)
    assert torch.isfinite(small.view(torch.float32)).all() and small[0] != small[1]
    assert torch.equal(Z[0::2], Z[0].expand(B // 2)) and torch.equal(Z[1::2], Z[1].expand(B // 2))
    assert torch.equal(Z[:2], small)


# ---- 4: length steps and long utterances ------------------------------------------------------------------------------------

LONG_T = 3000
LONG_LENGTHS = [1, 2, 3, 4, 5, 8, 9, 1024, 1025, LONG_T]


def long_case(T, dtype, lengths=None):
    """Bigram over 10 tokens, B = 10, targets of S = 40; `lengths` None: every utterance has all T frames."""
    graph = _ngram(10, 2, 2)
    B, S = 10, 40
    x, tr, _ = _case(T, B, 10, 77, dtype)
    il = torch.tensor(lengths) if lengths is not None else torch.full((B,), T, dtype=torch.int64)
    g = torch.Generator().manual_seed(78)
    tg = torch.randint(0, 10, (B, S), generator=g)
    tl = torch.minimum(il, torch.tensor(S))
    return graph, x, tr, il, tg, tl, _weights(B)


def test_length_steps_and_long_utterances_float64():
    """tile_shift(len) = 62 - ceil(log2 len) is computed in beam_loss_bwd and again in beam_loss_tr_reduce: one batch whose
    lengths sit on both sides of its steps (1, 2 | 3, 4 | 5, 8 | 9 .. and 1024 | 1025) and one utterance of 3000 frames.
    float64 only: alpha is kept in the emissions' dtype and grows with T, and the measured scaled error of the float32
    gradients on this case with equal full lengths is 3.6e-4 at T = 250, the shortest length of the
    ladder 250 .. 3000 -- above the rule's 1e-4, so float32 stays gated at the lengths of tests/test_hip_beam_loss.py."""
    graph, x, tr, il, tg, tl, gs = long_case(LONG_T, F64, LONG_LENGTHS)
    steps = sorted({int(np.ceil(np.log2(l))) for l in LONG_LENGTHS})
    assert steps == [0, 1, 2, 3, 4, 10, 11, 12]
    want, U, info = _reference(x, tr, graph, il, 4, INF, gs, tg, tl)
    assert np.isfinite(want[0]).all() and [len(u) for u in U] == LONG_LENGTHS
    assert all(_widest([u]) > 1 for u in U[1:])
    _check(_full(x, tr, graph, il, 4, gs=gs, tg=tg, tl=tl), want, F64, il, "length steps, float64")


# ---- 5: forced-state limits and odd targets -----------------------------------------------------------------------------

def test_2048_forced_positions_and_a_target_of_one_token():
    """min(S, T) = 2048, the limit: a target of 2048 positions without a repeat (2048 forced states through beam_loss_targets
    and the sort of beam_loss_sets, 4096 slots), and one that merges down to a single token."""
    A = _asg()
    N, T, S, K, B = 10, 2100, 2048, 4, 2
    graph = _ngram(N, 2, 2)
    x, tr, _ = _case(T, B, N, 41, F64)
    il = torch.tensor([T, 2060])
    tg = torch.stack([torch.arange(S) % N, torch.full((S,), 3)])
    tl = torch.tensor([S, S])
    assert min(S, T) == 2048 and (tg[0, 1:] != tg[0, :-1]).all() and int(il.min()) >= S
    gs = torch.tensor([1.5, -0.5], dtype=F64)
    want, U, info = _reference(x, tr, graph, il, K, INF, gs, tg, tl)
    # forced states beyond the beam in some frame of both utterances
    for b in range(B):
        sz = info["search"][b]["sizes"]
        assert any(len(U[b][t]) > sz[t] for t in range(int(il[b]))), b
    _check(_full(x, tr, graph, il, K, gs=gs, tg=tg, tl=tl), want, F64, il, "2048 forced positions")
    dv = lambda t: t.to(DEV)
    loss = A.beam_graph_asg_loss(dv(x), dv(tg), dv(tr), graph, dv(il), dv(tl), beam_size=K).cpu()
    assert torch.isfinite(loss[0]) and float(loss[0]) >= -1e-9 and not torch.isnan(loss).any()
    tg9 = torch.cat([tg, tg[:, :1]], 1)                    # min(S, T) = 2049
    with pytest.raises(RuntimeError, match="status 2"):
        A.beam_graph_full_score(dv(x), dv(tr), graph, dv(il), K, targets=dv(tg9), target_lengths=dv(tl))


def _small_automaton():
    # tests/test_beam_loss_cpu.py::test_target_cases: no arc on 2 from the start; state 0 does not accept
    return _asg().TokenGraph(np.array([[1, 0, -1], [1, 0, 1]]), np.zeros((2, 3)), np.array([-np.inf, 0.0]))


ODD = [("a label of -1", [0, -1, 2], 3, 6),
       ("a label of N", [0, 3, 2], 3, 6),
       ("no arc on 2 from the start", [2, 0, 2], 3, 6),
       ("ends in a state that does not accept", [0, 1, 1], 2, 6),
       ("target length 0", [0, 2, 0], 0, 6),
       ("target longer than the input", [0, 2, 0], 3, 2)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_odd_targets_force_nothing(dtype):
    """As tests/test_beam_loss_cpu.py::test_target_cases, on the GPU: nothing is forced, so the score and the gradients are
    those of the beam's own lattice -- and equal to the run without targets bit for bit."""
    graph = _small_automaton()
    B, T, N = len(ODD), 6, 3
    x, tr, _ = _case(T, B, N, 5, dtype)
    il = torch.tensor([c[3] for c in ODD])
    tg = torch.tensor([c[1] for c in ODD])
    tl = torch.tensor([c[2] for c in ODD])
    gs = _weights(B)
    for K in (1, 2):
        want, U, info = _reference(x, tr, graph, il, K, INF, gs, tg, tl)
        for b in range(B):                                 # nothing was forced
            assert [len(a) for a in U[b]] == info["search"][b]["sizes"], ODD[b][0]
        assert np.isfinite(want[0]).any()
        got = _full(x, tr, graph, il, K, gs=gs, tg=tg, tl=tl)
        _check(got, want, dtype, il, "odd targets K=%d" % K)
        for u, v in zip(got, _full(x, tr, graph, il, K, gs=gs)):
            assert torch.equal(u, v)


@pytest.mark.parametrize("dtype", DTYPES)
def test_odd_targets_give_an_infinite_loss_and_the_normaliser_gradient(dtype):
    """Every target of ODD through beam_graph_asg_loss (and graph_asg_loss, which must be +inf in the same places): +inf, no
    NaN, and only the normaliser's posterior in the gradients.  The force-aligned kernels never see a label outside the
    alphabet: the loss replaces it and makes the aligned score -inf (torch_asg_amd.asg._guarded_targets).  A seventh utterance
    with a good target, next to them in the batch, keeps a finite loss (its grad_scores is 0, so that the gradients stay the
    reference's)."""
    A = _asg()
    graph = _small_automaton()
    odd = ODD + [("a good target", [0, 2, -1], 2, 6)]          # (-1 behind the target's length: padding, not an error)
    B, T, N = len(odd), 6, 3
    x, tr, _ = _case(T, B, N, 6, dtype)
    il = torch.tensor([c[3] for c in odd])
    tg = torch.tensor([c[1] for c in odd])
    tl = torch.tensor([c[2] for c in odd])
    gs = _weights(B)
    gs[-1] = 0.0
    bad = torch.tensor([True] * len(ODD) + [False])
    dv = lambda t: t.to(DEV)
    exact = A.graph_asg_loss(dv(x), dv(tg), dv(tr), graph, dv(il), dv(tl)).cpu()
    assert (exact[bad] == INF).all() and torch.isfinite(exact[~bad]).all(), exact
    for K in (1, 2):
        want, _, _ = _reference(x, tr, graph, il, K, INF, gs, tg, tl)
        xd, td = dv(x).requires_grad_(True), dv(tr).requires_grad_(True)
        loss = A.beam_graph_asg_loss(xd, dv(tg), td, graph, dv(il), dv(tl), beam_size=K)
        lc = loss.detach().cpu()
        assert (lc[bad] == INF).all(), (K, lc)
        assert torch.isfinite(lc[~bad]).all() and (lc[~bad] >= -1e-4).all(), (K, lc)
        loss.backward(gs.to(DEV, dtype))
        gx, gtr = xd.grad.cpu(), td.grad.cpu()
        assert not torch.isnan(gx).any() and not torch.isnan(gtr).any()
        if dtype == F64:
            assert np.allclose(gx.numpy(), want[1], rtol=1e-9, atol=1e-9) and np.allclose(gtr.numpy(), want[2], rtol=1e-9, atol=1e-9)
        else:
            assert_close(gx.numpy(), want[1], what="grad_inputs")
            assert_close(gtr.numpy(), want[2], what="grad_transition")


def test_more_than_2_to_the_20_frames_is_refused_by_the_workspace_query():
    """A pure host check, no allocation: T = 2^20 is sized, T = 2^20 + 1 is not."""
    from torch_asg_amd import _lib
    L = _lib.lib()
    Q, E, N, B, K = 65640, 2559960, 40, 1, 256
    g = _lib.AsgTokenGraph()
    g.Q, g.E, g.N, g.dtype = Q, E, N, _lib.ASG_DTYPE_F32
    for n in ("label", "state", "row", "src", "src_label", "start_w", "final_w", "edge_w"):
        setattr(g, n, 8)
    gb = _lib.AsgTokenGraphBeam()
    gb.graph = ctypes.pointer(g)
    gb.num_start, gb.max_out = 40, 39
    for n in ("orow", "oarc", "ow", "start_q"):
        setattr(gb, n, 8)
    gl = _lib.AsgTokenGraphBeamLoss()
    gl.beam, gl.S, gl.start, gl.next = ctypes.pointer(gb), 1641, 0, 8
    p = _lib.AsgProblem()
    p.inputs = p.transition = p.targets = 8
    p.B, p.N, p.S, p.dtype = B, N, 60, _lib.ASG_DTYPE_F32
    for T, ok in (((1 << 20), True), ((1 << 20) + 1, False)):
        p.T = T
        for store in (0, 1):
            assert (L.asg_beam_graph_full_work_bytes(ctypes.byref(p), ctypes.byref(gl), K, store) > 0) == ok
        assert (L.asg_beam_graph_full_scratch_bytes(ctypes.byref(p), ctypes.byref(gl), K) > 0) == ok
