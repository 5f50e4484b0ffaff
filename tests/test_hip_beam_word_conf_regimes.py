"""GPU tests (-m gpu) of the two confidence entry points of the lexicon + word-LM beam family --
`beam_decode_words_confidence` (csrc/asg_beam_word_conf.hip) and `beam_decode_words_nbest_confidence`
(csrc/asg_beam_word_nbest_conf.hip) -- at the sizes of tests/test_hip_beam_word_regimes.py, which was written before they
existed.  They bring device text that no other call compiles: the search with the decoder's end
(`beam_word_conf_search<R, TRL, LA, FIN>`), the beta pull over 64-bit pair keys with a word-event sink
(csrc/asg_beam_word_conf_pull.h) and the two sinks.

  1. pairs h << qbits | q of 9, 17, 33 and 35 bits: in the pull `find_sorted`, `pp & qmask`, `label`, `end` and the copy of
     U into LDS all take the full key;
  2. LM walks of 63 and 64 backoff steps on the separator edges of the pull (`for_each_out`) and at its end;
  3. the transitions of the search inside LDS and in global memory, float32 at N = 199 | 200 and float64 at N = 141 | 142,
     plain and with look-ahead, one-best and n-best: all 16 instantiations of the search;
  4. a lattice set at the documented bound M = K = 8179 (float32) / 6816 (float64): more than 64 KiB of dynamic LDS in
     `beam_word_conf_bwd` and `nbest_conf_bwd`, several passes of the pull's k0 loop at one lane per pair, and the refusal at
     K + 1;
  5. source sets around every halving of the lanes per source pair (64 -> 1), with a row of 39 edges longer than the lanes.

The inputs are those of tests/beam_word_regime_cases.py.  Every case first repeats its precondition from the restatement's own
output and the restated launch arithmetic (tests/test_beam_word_conf_regimes_cpu.py holds the same assertions and each case's
bite), then compares through the `_check` of tests/test_hip_beam_word_conf.py and tests/test_hip_beam_word_nbest_conf.py: the
decoder and n-best fields byte for byte with the device's own decoders, the normalisers bit for bit with
`beam_words_full_score`, row 0 bit for bit with the one-best call, frames exactly, confidences by the family's rule (float64
rtol = atol = 1e-9, float32 tests/util.py's assert_close, padding exactly 0, never a NaN)."""
import functools

import numpy as np
import pytest
import torch

import beam_word_regime_cases as C
import test_hip_beam_word_conf as one_best
import test_hip_beam_word_nbest_conf as rows
from beam_word_loss_ref import word_model
from beam_word_nbest_conf_ref import beam_word_nbest_conf_ref
from beam_word_ref import beam_word_ref
from test_beam_word_conf_regimes_cpu import (BOUND_ROWS, BOUND_TOL, NO_RING, WIDTH_ROWS, assert_width_conf_regime, bound_lds,
                                             bound_regime, depth_conf_regime, lanes_conf_regime, width_conf_regime)
from test_hip_beam_word_regimes import one_look_ahead_memo_per_case  # noqa: F401  (autouse: the look-ahead restatements share their memos)

pytestmark = pytest.mark.gpu
INF = float("inf")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
NP = {torch.float32: np.float32, torch.float64: np.float64}
W1 = (1.0, 1.0, 0.0)               # lm_weight, word_score, token_score of case 1: integers stay integers
W = (0.7, -0.4, 0.3)
WW = (0.5, -0.2, 0.1)


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _t(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


@functools.lru_cache(maxsize=None)
def _qbits(lex, lm):
    """The bits of a pair's product state, from the restatement's model."""
    return C.bits_of(word_model(lex, lm, np.float64).Q)


# ---------------------------------------------------------------------------------------------------------------- case 1
@DTYPES
@pytest.mark.parametrize("theta", C.WIDTH_THETAS)
@pytest.mark.parametrize("pbits,K", [(9, 3), (9, 5), (17, 3), (17, 5), (33, 8), (33, 64), (35, 8), (35, 64)])
def test_wide_pairs_in_the_pull_and_the_sinks(pbits, K, theta, dtype):
    """One-best at tolerance 0 and 2, one-best with look-ahead of order 2 at tolerance 1, 8 rows at tolerance 1, 8 rows with
    look-ahead at tolerance 0.  From 33 bits on (CONF_WIDTH_SEEDS) the plain sets hold pairs >= 2^32 and, over the width's
    beams and thresholds, a reported value changes by more than 1e-2, or loses its lattice, when those pairs are taken out;
    the look-ahead sets hold such pairs too.  (A library whose pull cuts an edge's target pair to 32 bits before `find_sorted`
    fails all 16 cases of 33 and 35 bits, with errors of 0.4 to 1.0, and none of 9 and 17 bits.)"""
    A = _asg()
    lex, lm = C.width_case(pbits)
    x, tr, il = _t(*C.width_inputs(pbits, NP[dtype], seed=C.CONF_WIDTH_SEEDS.get(pbits)))
    la = A.WordLookahead(lex, lm, 2)
    plain = {}
    if pbits >= 33:
        wide, diff, dead, plain = width_conf_regime(pbits, NP[dtype])
        print("pbits %d %s: %d pairs >= 2^32; without them the largest change is %.3g, %d hypotheses lose their lattice"
              % (pbits, dtype, wide, diff, dead))
        assert_width_conf_regime(wide, diff, dead)
    ahead = beam_word_nbest_conf_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), K, WIDTH_ROWS, theta, *W1, 0, 2)
    if pbits >= 33:
        assert sum(C.wide_pairs(u, _qbits(lex, lm)) for u in ahead["sets"]) > 0, "no pair >= 2^32 in the look-ahead sets"
    what = "pbits %d" % pbits
    info = {}
    for tol in (0, 2):
        one_best._check(x, tr, lex, lm, il, K, theta, W1, tol, info=info, what=what)
        assert info["pbits"] == pbits and info["qbits"] == _qbits(lex, lm)
    rows._check(x, tr, lex, lm, il, K, WIDTH_ROWS, theta, W1, 1, want=plain.get((K, theta)), what=what)
    rows._check(x, tr, lex, lm, il, K, WIDTH_ROWS, theta, W1, 0, la, want=ahead, what=what)
    one_best._check(x, tr, lex, lm, il, K, theta, W1, 1, la, what=what)


# ---------------------------------------------------------------------------------------------------------------- case 2
@DTYPES
@pytest.mark.parametrize("form", ["uniform", "mixed"])
@pytest.mark.parametrize("depth", [63, 64])
def test_walks_of_63_and_64_backoff_steps_inside_the_pull(depth, form, dtype):
    """The LM step of `for_each_out` on every separator edge and of `end`: kMaxBackoff = 64 steps are walked.  At K = 8 a word
    that ends on a separator edge has a confidence inside (0.01, 0.99): the value read rests on the walk."""
    A = _asg()
    lex, lm = C.small_lexicon(), C.chain_lm(depth, form)
    x, tr, il = _t(*C.chain_inputs(NP[dtype]))
    deep = A.WordLookahead(lex, lm, 65)
    assert deep.depth[deep.la_state].max() == depth and lm.start == depth
    want8 = beam_word_nbest_conf_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), 8, 4, INF, *W, 1)
    steps = depth_conf_regime(depth, form, want8["one_best"], il.numpy())
    print("depth %d %s %s: walks of %s steps" % (depth, form, dtype, sorted(steps)))
    for K in (1, 8):
        what = "depth %d %s" % (depth, form)
        one_best._check(x, tr, lex, lm, il, K, INF, W, 1, what=what)
        one_best._check(x, tr, lex, lm, il, K, INF, W, 0, deep, what=what)
        rows._check(x, tr, lex, lm, il, K, 4, INF, W, 1, want=want8 if K == 8 else None, what=what)
        rows._check(x, tr, lex, lm, il, K, 4, INF, W, 1, deep, what=what)


# ---------------------------------------------------------------------------------------------------------------- case 3
@pytest.mark.parametrize("side", ["transitions-in-lds", "transitions-in-global-memory"])
@pytest.mark.parametrize("elem,N0", [(4, 199), (8, 141)], ids=["f32", "f64"])
def test_every_instantiation_of_the_search_with_the_decoders_end(elem, N0, side):
    """4096 + K (e + 8) + N N e against 160 KiB at K = 8: N = 199 | 200 (float32) and 141 | 142 (float64).  Each of the four
    cases runs the one-best call (FIN = false) and the 3-row n-best call (FIN = true), plain (LA = false) and with look-ahead
    of order 2 (LA = true); over the four cases that is every instantiation of beam_word_conf_search<R, TRL, LA, FIN>:

      <float,  true,  *, *>  f32, N = 199      <float,  false, *, *>  f32, N = 200
      <double, true,  *, *>  f64, N = 141      <double, false, *, *>  f64, N = 142

    with <*, *> = <false, false> one-best, <true, false> one-best with look-ahead, <false, true> n-best, <true, true> n-best
    with look-ahead: 16 in all."""
    A = _asg()
    K = 8
    dtype = torch.float32 if elem == 4 else torch.float64
    assert (elem, K, N0) in C.LDS_STEPS
    N = N0 + (side != "transitions-in-lds")
    assert C.transitions_in_lds(K, N, elem) == (N == N0) and C.transitions_in_lds(K, N0, elem) and not C.transitions_in_lds(K, N0 + 1, elem)
    lex, lm = C.layout_case(N)
    x, tr, il = _t(*C.layout_inputs(N, NP[dtype]))
    info = {}
    pre = beam_word_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), K, INF, *W, info=info)
    assert pre["word_lengths"][0] >= 2 and max(max(z) for z in info["sizes"]) > 1
    la = A.WordLookahead(lex, lm, 2)
    what = "N=%d" % N
    _, want = one_best._check(x, tr, lex, lm, il, K, INF, W, 1, what=what)
    assert (want["word_frames"][0, :2] >= 1).all()
    one_best._check(x, tr, lex, lm, il, K, INF, W, 1, la, what=what)
    rows._check(x, tr, lex, lm, il, K, 3, INF, W, 1, what=what)
    rows._check(x, tr, lex, lm, il, K, 3, INF, W, 1, la, what=what)


# ---------------------------------------------------------------------------------------------------------------- case 4
@DTYPES
def test_both_sides_of_the_bound_on_the_lattice_set(dtype):
    """M = K = 8179 (float32) / 6816 (float64) on the 300-word lexicon: frames 3 and 4 keep exactly K pairs, so the pull's k0
    loop takes 8 (7) passes at one lane per pair, `beam_word_conf_bwd` asks for 100208 (111104) bytes of dynamic LDS and
    `nbest_conf_bwd` with 4 rows at tolerance 1 for 99376 (110272).  K + 1 is refused by both calls, and so is, at K, the first
    ring that does not fit beside the set (8192 slots: 64 rows at tolerance 32)."""
    e = 4 if dtype == torch.float32 else 8
    K = C.CONF_BOUND[e]
    lex, lm = C.wide_case()
    x, tr, il = _t(*C.wide_inputs(NP[dtype]))
    one, many, over = bound_lds(e)
    assert rows.fits(e, K, BOUND_ROWS, BOUND_TOL) and not rows.fits(e, K, *NO_RING)
    want = beam_word_nbest_conf_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), K, BOUND_ROWS, INF, *WW, BOUND_TOL)
    sizes = bound_regime(e, want["sets"])
    print("%s K %d: sets of %s, %d and %d bytes of dynamic LDS" % (dtype, K, sizes, one, many))
    rows._check(x, tr, lex, lm, il, K, BOUND_ROWS, INF, WW, BOUND_TOL, want=want, what="M = bound")
    one_best._check(x, tr, lex, lm, il, K, INF, WW, BOUND_TOL, what="M = bound")
    with pytest.raises(RuntimeError, match="asg_beam_words_confidence"):
        one_best._run(x, tr, lex, lm, il, K + 1, INF, WW, BOUND_TOL)
    with pytest.raises(RuntimeError, match="asg_beam_words_nbest_confidence"):
        rows._run(x, tr, lex, lm, il, K + 1, BOUND_ROWS, INF, WW, BOUND_TOL)
    with pytest.raises(RuntimeError, match="asg_beam_words_nbest_confidence"):
        rows._run(x, tr, lex, lm, il, K, NO_RING[0], INF, WW, NO_RING[1])


# ---------------------------------------------------------------------------------------------------------------- case 5
@pytest.mark.parametrize("K", C.LANE_BEAMS)
def test_lanes_per_source_pair_in_the_pull(K):
    """A source set of exactly K pairs, G = subgroup(K) lanes per pair, and from K = 17 on (G < 64) the separator state's row of
    39 edges -- the trie root's -- is longer than G: its lanes stride the row more than once, each LM step taken by the lane
    that owns the edge."""
    lex, lm = C.wide_case()
    x, tr, il = _t(*C.wide_inputs())
    info = {}
    beam_word_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), K, INF, *WW, info=info)
    G, row = lanes_conf_regime(K, info)
    print("K %d: G %d, longest row %d" % (K, G, row))
    assert (row > G) == (K > 16)
    _, want = one_best._check(x, tr, lex, lm, il, K, INF, WW, 1, what="lanes")
    assert any(len(u) == K for Ub in want["sets"] for u in Ub[:-1])
    if K in (16, 17, 128, 129, 512, 513):
        rows._check(x, tr, lex, lm, il, K, 5, INF, WW, 1, what="lanes")
