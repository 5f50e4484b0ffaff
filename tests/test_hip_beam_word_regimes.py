"""GPU tests (-m gpu) of the lexicon + word-LM beam family -- the one-shot decoder, LM look-ahead, n-best, the two streams and the
two beam-pruned losses, which all compile csrc/asg_beam_word_frame.h -- at the sizes where that frame changes shape:

  1. pairs h << qbits | q of 8 | 9, 16 | 17, 32 | 33 and 35 bits: the tie select's second and later 8-bit digits, its narrow
     last digit, and pairs at and above 2^32 under the 64-bit atomicMin of `arg`, the n-best sort and the losses' sorted sets;
  2. LM walks of 63 and 64 backoff steps in `step` and `look` (kMaxBackoff = 64);
  3. the transitions inside LDS and in global memory, on both sides of 4096 + K (e + 8) + N N e <= 160 KiB, where N pushes the
     step (K = 8) and where K does (K = 8192).  Above 64 KiB -- every K = 8192 row, and the K = 8 rows on their LDS side -- the
     launch also asks the runtime for its dynamic LDS;
  4. beams around every halving of the lanes per kept pair (64 -> 1), bit for bit, with rows longer than the lanes.

The inputs are those of tests/beam_word_regime_cases.py.  Every case first repeats its precondition from the restatement's own
`info` and the restated launch arithmetic (tests/test_beam_word_regimes_cpu.py holds the same assertions, and that a wrong rank
of the pairs or a walk one step short changes the outputs), then compares the device with the restatement by the family's own
rules: the decoders, n-best lists and streams bit for bit, the losses to rtol = atol = 1e-9 in float64 and tests/util.py's
assert_close in float32 with the infinity pattern exact.

Out of scope: pairs wider than 37 bits (they need a lexicon or an LM too large for a test), chains deeper than 64 passed
through the C API, the separate LDS layout of the n-best kernel, and the losses at K = 8192 (their own bound on the lattice set,
tests/test_hip_beam_word_loss.py::test_both_sides_of_the_bound_on_the_lattice_set, is below it).

The two confidence entry points, `beam_decode_words_confidence` and `beam_decode_words_nbest_confidence`, have these sizes in
tests/test_hip_beam_word_conf_regimes.py."""
import numpy as np
import pytest
import torch

import beam_word_la_ref
import beam_word_regime_cases as C
import test_hip_beam_word as one_shot
import test_hip_beam_word_la as la_one_shot
import test_hip_beam_word_la_loss as la_loss
import test_hip_beam_word_la_nbest as la_nbest
import test_hip_beam_word_la_stream as la_stream
import test_hip_beam_word_la_window as la_window
import test_hip_beam_word_loss as loss
import test_hip_beam_word_nbest as nbest
import test_hip_beam_word_stream as stream
import test_hip_beam_word_window as window
from test_beam_word_regimes_cpu import assert_width_regime, lanes_regime, width_regime

pytestmark = pytest.mark.gpu
INF = float("inf")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
NP = {torch.float32: np.float32, torch.float64: np.float64}
W1 = (1.0, 1.0, 0.0)               # lm_weight, word_score, token_score of case 1: integers stay integers
W = (0.7, -0.4, 0.3)
WW = (0.5, -0.2, 0.1)


@pytest.fixture(autouse=True, scope="module")
def one_look_ahead_memo_per_case():
    """The look-ahead restatements of this module run over one 2500-word lexicon and LMs of up to 2^22 + 1 states: while the
    module runs they share the memos of E and L (tests/beam_word_la_ref.py::shared_memos), which die with it."""
    beam_word_la_ref.shared_memos = {}
    yield
    beam_word_la_ref.shared_memos = None


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _t(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def _streams(x, tr, lex, lm, la, il, K, theta, w, one, what):
    """The plain or look-ahead stream, fed one frame at a time and in uneven chunks: the restatement's bytes after every chunk,
    and the one-shot call's bits at the end.  -> the restatement's (tie cuts, source ties)."""
    T, B = x.shape[0], x.shape[1]
    seen = [0, 0]
    for cuts in (list(range(T + 1)), [0, 1, 1, T - 3, T]):
        s = stream.Both(tr, lex, lm, B, T, K, theta, *w) if la is None else la_stream.Both(tr, lex, lm, la, B, T, K, theta, *w)
        s.feed(x, il, cuts, check="%s chunks %s" % (what, cuts))
        end = s.check("%s chunks %s" % (what, cuts))[True]
        stream._same_as_one_shot(end, one, T, what)
        seen = [seen[0] + s.ref.tie_cuts, seen[1] + s.ref.src_ties]
    return seen


def _windows(x, tr, lex, lm, la, il, K, theta, w, one, what):
    T, B = x.shape[0], x.shape[1]
    for Wn, P, cuts in ((4, 2, list(range(T + 1))), (8, 3, [0, 1, 1, T - 3, T])):
        s = window.Both(tr, lex, lm, B, Wn, P, K, theta, *w) if la is None else la_window.Both(tr, lex, lm, la, B, Wn, P, K, theta, *w)
        res = s.feed(x, il, cuts, "%s W=%d P=%d" % (what, Wn, P), results=True)
        assert res[True]["scores"].tobytes() == one["scores"].tobytes(), what          # the search is the one-shot search


# ---------------------------------------------------------------------------------------------------------------- case 1
@DTYPES
@pytest.mark.parametrize("pbits", sorted(C.WIDTHS))
def test_pair_widths_in_the_decoder_and_the_loss(pbits, dtype):
    """The one-shot decoder over every beam and threshold of the width, the plain loss with targets that force pairs whose
    history is the largest state.  The precondition is the CPU test's: cuts in the top digit and in a lower one, source ties
    between histories and, from 33 bits on, a cut and a source tie decided at or above bit 32."""
    lex, lm = C.width_case(pbits)
    x, tr, il = _t(*C.width_inputs(pbits, NP[dtype]))
    tg, tl = _t(*C.last_word_target(lex))
    gs = torch.tensor([1.0, -0.5])
    total = {}
    for K in C.width_beams(pbits):
        for theta in C.WIDTH_THETAS:
            info = {}
            one_shot._check(x, tr, lex, lm, il, K, theta, *W1, info=info, what="pbits %d" % pbits)
            for k, v in width_regime(pbits, info).items():
                total[k] = sorted(set(total.get(k, [])) | set(v)) if k == "digits" else total.get(k, 0) + v
    print("pbits %d %s: Q %d qbits %d H %d; %s" % (pbits, dtype, info["Q"], info["qbits"], lm.H, total))
    graph = lex.compile_words(one_shot.DEV, dtype)
    assert graph["Q"] == graph["label"].numel() == info["Q"]                                   # the bit counts of the compiled graph
    assert C.bits_of(graph["Q"]) + C.bits_of(lm.H) == pbits == info["pbits"]
    assert_width_regime(pbits, total)
    for K in C.width_beams(pbits)[:2]:
        _, (Z, _, _, U) = loss._check(x, tr, lex, lm, il, K, INF, W1, tg, tl, gs, what="pbits %d" % pbits)
        assert np.isfinite(Z).all() and max(h for Ub in U for u in Ub for h, _ in u) == lm.H - 1


@DTYPES
@pytest.mark.parametrize("pbits", [8, 9, 33])
def test_every_entry_point_on_both_sides_of_a_digit_and_above_32_bits(pbits, dtype):
    """Every entry point at 8 | 9 and 33 bits, each against its own restatement, the streams also against the one-shot call.  The
    precondition is the width's, asserted from the plain restatement's `info` over the beams and thresholds THIS test runs: a
    cut in the top digit and (from 9 bits) one in a lower digit, a source tie between histories and, at 33 bits, a cut and a
    source tie decided at or above bit 32 (at K = 8 and K = 64)."""
    A = _asg()
    lex, lm = C.width_case(pbits)
    x, tr, il = _t(*C.width_inputs(pbits, NP[dtype]))
    tg, tl = _t(*C.last_word_target(lex))
    gs = torch.tensor([1.0, -0.5])
    beams = (3, 5) if pbits < 32 else (8, 64)
    total = {}
    cuts = ties = lists = 0
    for K in beams:
        for theta in C.WIDTH_THETAS:
            what = "pbits %d K=%d theta=%s" % (pbits, K, theta)
            info = {}
            one = one_shot._check(x, tr, lex, lm, il, K, theta, *W1, info=info, what=what)
            for k, v in width_regime(pbits, info).items():
                total[k] = sorted(set(total.get(k, [])) | set(v)) if k == "digits" else total.get(k, 0) + v
            _, want = nbest._check(x, tr, lex, lm, il, K, K, theta, *W1, what=what)
            lists += int((want["num_hyps"] > 1).sum())
            c, s = _streams(x, tr, lex, lm, None, il, K, theta, W1, one, what)
            assert c == 2 * info["tie_cuts"] and s == 2 * info["src_ties"]       # the streams made the plain search's cuts, twice
            _windows(x, tr, lex, lm, None, il, K, theta, W1, one, what)
            for order in (1, 2):
                la = A.WordLookahead(lex, lm, order)
                info = {}
                one = la_one_shot._check(x, tr, lex, lm, la, il, K, theta, *W1, info=info, what=what)
                cuts, ties = cuts + info["tie_cuts"], ties + info["src_ties"]
                if order == 2:
                    assert (la.la_state == np.arange(lm.H)).all()      # look() reads its state at the pair's own, wide h
                    la_nbest._check(x, tr, lex, lm, la, il, K, K, theta, *W1, what=what)
                    _streams(x, tr, lex, lm, la, il, K, theta, W1, one, what)
                    _windows(x, tr, lex, lm, la, il, K, theta, W1, one, what)
        la = A.WordLookahead(lex, lm, 2)
        _, (Z, _, _, U) = la_loss._check(x, tr, lex, lm, la, il, K, INF, W1, tg, tl, gs, what="pbits %d" % pbits)
        assert np.isfinite(Z).all() and max(h for Ub in U for u in Ub for h, _ in u) == lm.H - 1
    print("pbits %d %s beams %s: %s" % (pbits, dtype, beams, total))
    assert_width_regime(pbits, total)
    assert cuts > 0 and ties > 0 and lists > 0             # the look-ahead searches cut ties and tie sources too


# ---------------------------------------------------------------------------------------------------------------- case 2
@DTYPES
@pytest.mark.parametrize("form", ["uniform", "mixed"])
@pytest.mark.parametrize("depth", [63, 64])
def test_walks_of_63_and_64_backoff_steps(depth, form, dtype):
    """`step` on the separator edges and at the end, `look` of order 65 from the deepest state: kMaxBackoff = 64 steps are
    walked, not 63 (the CPU test shows that one step short gives -inf or other words on this input)."""
    A = _asg()
    lex, lm = C.small_lexicon(), C.chain_lm(depth, form)
    x, tr, il = _t(*C.chain_inputs(NP[dtype]))
    tg = torch.tensor([[0, 1, 4, 2, 4, 0, 1, 4], [2, 4, 0, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0, 0, 0]])
    tl = torch.tensor([8, 2, 1])
    gs = torch.tensor([1.0, -0.5, 2.0])
    deep = A.WordLookahead(lex, lm, 65)
    assert deep.depth[deep.la_state].max() == depth and lm.start == depth
    for K in (1, 8):
        what = "depth %d %s K=%d" % (depth, form, K)
        got = one_shot._check(x, tr, lex, lm, il, K, INF, *W, what=what)
        assert got["word_lengths"][0] >= 2 and np.isfinite(got["scores"][:2]).all()
        one = stream._gpu_one_shot(x, tr, lex, lm, il, K, INF, *W)
        _streams(x, tr, lex, lm, None, il, K, INF, W, one, what)
        for order in (1, 2, 65):
            la_one_shot._check(x, tr, lex, lm, deep if order == 65 else A.WordLookahead(lex, lm, order), il, K, INF, *W, what=what)
        _, (Z, _, _, _) = loss._check(x, tr, lex, lm, il, K, INF, W, tg, tl, gs, what=what)
        assert np.isfinite(Z).all()
        la_loss._check(x, tr, lex, lm, deep, il, K, INF, W, tg, tl, gs, what=what)
    print("depth %d %s %s: walks of up to %d steps, look-ahead depth %d" % (depth, form, dtype, depth, deep.depth[deep.la_state].max()))


# ---------------------------------------------------------------------------------------------------------------- case 3
@pytest.mark.parametrize("side", ["transitions-in-lds", "transitions-in-global-memory"])
@pytest.mark.parametrize("elem,K,N0", C.LDS_STEPS, ids=["f32-K8", "f64-K8", "f32-K8192", "f64-K8192"])
def test_both_transition_layouts_of_every_step(elem, K, N0, side):
    """4096 + K (e + 8) + N N e against 160 KiB: N = 199 | 200 (float32) and 141 | 142 (float64) at K = 8; 123 | 124 and 59 | 60 at
    K = 8192, where the set takes 96 or 128 KiB.  Every K = 8192 launch and every launch with the matrix inside asks for more
    than 64 KiB, so it also sets the kernel's dynamic LDS limit.  The one-shot decoder plain and with look-ahead, the plain
    n-best, and at K = 8 the plain loss (K = 8192 is beyond the loss's own bound)."""
    A = _asg()
    dtype = torch.float32 if elem == 4 else torch.float64
    N = N0 + (side != "transitions-in-lds")
    assert C.transitions_in_lds(K, N, elem) == (N == N0) and C.transitions_in_lds(K, N0, elem) and not C.transitions_in_lds(K, N0 + 1, elem)
    assert C.dynamic_lds(K, N, elem) > 64 * 1024 or (K == 8 and N == N0 + 1)
    print("elem %d K %d N %d: %d bytes with the matrix, the launch asks for %d" % (elem, K, N, C.beam_lds(K, N, elem), C.dynamic_lds(K, N, elem)))
    lex, lm = C.layout_case(N)
    x, tr, il = _t(*C.layout_inputs(N, NP[dtype]))
    info = {}
    got = one_shot._check(x, tr, lex, lm, il, K, INF, *W, info=info, what="N=%d" % N)
    assert got["word_lengths"][0] >= 2 and max(max(z) for z in info["sizes"]) > 1
    la_one_shot._check(x, tr, lex, lm, A.WordLookahead(lex, lm, 2), il, K, INF, *W, what="N=%d" % N)
    nbest._check(x, tr, lex, lm, il, K, 3, INF, *W, what="N=%d" % N)
    if K == 8:
        mid = 100 if N > 101 else 40
        tg = torch.tensor([[3, 7, N - 1, N - 2, N - 1], [3, mid, 5, N - 1, 0]])
        loss._check(x, tr, lex, lm, il, K, INF, W, tg, torch.tensor([5, 4]), torch.tensor([1.0, -2.0]), what="N=%d" % N)


@pytest.mark.parametrize("N", [199, 200], ids=["transitions-in-lds", "transitions-in-global-memory"])
def test_both_transition_layouts_of_the_streams_in_float32(N):
    """The float32 step of the four streams (tests/test_hip_beam_word_stream.py and its kin hold the float64 one)."""
    A = _asg()
    K = 8
    assert C.transitions_in_lds(K, N, 4) == (N == 199)
    lex, lm = C.layout_case(N)
    x, tr, il = _t(*C.layout_inputs(N, np.float32))
    one = stream._gpu_one_shot(x, tr, lex, lm, il, K, INF, *W)
    assert one["word_lengths"][0] >= 2
    _streams(x, tr, lex, lm, None, il, K, INF, W, one, "N=%d" % N)
    _windows(x, tr, lex, lm, None, il, K, INF, W, one, "N=%d" % N)
    la = A.WordLookahead(lex, lm, 2)
    one = la_stream._gpu_one_shot(x, tr, lex, lm, la, il, K, INF, *W)
    _streams(x, tr, lex, lm, la, il, K, INF, W, one, "N=%d look-ahead" % N)
    _windows(x, tr, lex, lm, la, il, K, INF, W, one, "N=%d look-ahead" % N)


# ---------------------------------------------------------------------------------------------------------------- case 4
@pytest.mark.parametrize("K", C.LANE_BEAMS)
def test_lanes_per_pair_bit_for_bit(K):
    """A frame with a successor keeps exactly K pairs, and from K = 17 on (G = beam_lanes_per_state(K) < 64) one of them -- the
    separator state, whose row is the trie root's 39 edges -- has a row longer than G: its lanes stride the row more than once."""
    A = _asg()
    lex, lm = C.wide_case()
    x, tr, il = _t(*C.wide_inputs())
    info = {}
    one_shot._check(x, tr, lex, lm, il, K, INF, *WW, info=info, what="lanes")
    G, row = lanes_regime(K, info)
    print("K %d: G %d, longest row %d" % (K, G, row))
    assert (row > G) == (K > 16) and max(max(z) for z in info["sizes"]) == K
    la_one_shot._check(x, tr, lex, lm, A.WordLookahead(lex, lm, 2), il, K, INF, *WW, what="lanes")
    _streams(x, tr, lex, lm, None, il, K, INF, WW, stream._gpu_one_shot(x, tr, lex, lm, il, K, INF, *WW), "lanes")
