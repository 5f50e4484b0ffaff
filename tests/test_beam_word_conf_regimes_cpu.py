"""CPU tests of the inputs of tests/test_hip_beam_word_conf_regimes.py: from the numpy restatements (tests/beam_word_conf_ref.py,
tests/beam_word_nbest_conf_ref.py) and the restated launch arithmetic of tests/beam_word_regime_cases.py ALONE, every case of
the two confidence calls is in the regime it names, and every case can tell a subtly wrong kernel from a right one:

  widths   the lattice sets hold pairs h << qbits | q >= 2^32, and a REPORTED confidence changes by more than 1e-2 (or its
           utterance's normaliser becomes -inf) when the lattice loses those pairs -- what a pull that cut a key to 32 bits in
           `find_sorted`, `label`, `end` or the copy of U into LDS would report.  1e-2 is a hundred times the family's float32
           rule (tests/util.py::assert_close, 1e-4 scaled): such a difference cannot hide inside the tolerance;
  depths   a word that ends on a separator edge -- the pull's own LM step -- has a confidence strictly inside (0.01, 0.99),
           and in the 'uniform' chain every LM step of the lattice takes exactly `depth` backoff steps;
  bound    at K = 8179 (float32) / 6816 (float64) a source set has exactly K pairs, the pull asks for more than 64 KiB and at
           most 160 KiB of LDS, and the n-best limit holds with a ring of 16 slots and fails with the first ring that does not
           fit beside that set, 8192 slots;
  lanes    a source set has exactly K pairs, the lattice pass's `subgroup` is the search's lanes per kept pair, and from
           K = 17 on a kept pair's row of 39 edges is longer than its G lanes.

The functions without `test_` are what the GPU module repeats, from the restatement's output, before it compares."""
import functools

import numpy as np
import pytest

import beam_word_regime_cases as C
from beam_word_conf_ref import beam_word_conf_ref, word_events
from beam_word_loss_ref import word_model
from beam_word_nbest_conf_ref import beam_word_nbest_conf_ref
from beam_word_ref import beam_word_ref
from graph_decode_ref import _clamped_lengths
from test_beam_word_regimes_cpu import lanes_regime

INF = float("inf")
W1 = (1.0, 1.0, 0.0)               # lm_weight, word_score, token_score of the width cases: integers stay integers
W = (0.7, -0.4, 0.3)
WW = (0.5, -0.2, 0.1)              # the weights of the 300-word cases
MARGIN = 1e-2                      # what losing the wide pairs has to change in a reported value
CONF_WIDTH_BEAMS = (8, 64)
WIDTH_ROWS = 8
BOUND_ROWS, BOUND_TOL = 4, 1
NO_RING = (64, 32)                 # (nbest, tol) of the first ring that does not fit beside a set at the bound: 8192 slots


# ---------------------------------------------------------------------------------------------------------------- widths
def wide_pair_effect(lex, lm, xs, tr, il, w, want, tol):
    """What the reported confidences of one restatement (one-best, or n-best: `path` has three axes) owe to the pairs >= 2^32
    of its sets -> (the number of such pairs, the largest change of a reported confidence when the lattice loses them and keeps a
    finite normaliser, the number of hypotheses whose utterance's normaliser becomes -inf without them).  On the way:
    `confidences_on_sets` over the full sets is the restatement."""
    xs = np.asarray(xs)
    T, B, _ = xs.shape
    m = word_model(lex, lm, xs.dtype.type, *w)
    qbits = C.bits_of(m.Q)
    x, tr = xs.astype(np.float64), np.asarray(tr, np.float64)
    lens = _clamped_lengths(il, T, B)
    rows = want["path"].ndim == 3
    wide, diff, dead = 0, 0.0, 0
    for b in range(B):
        L, full = int(lens[b]), want["sets"][b]
        cut = C.without_wide_pairs(full, qbits)
        wide += C.wide_pairs(full, qbits)
        if rows:
            hyps = [(want["path"][b, r], want["words"][b, r], int(want["word_lengths"][b, r]), want["word_confidences"][b, r])
                    for r in range(int(want["num_hyps"][b]))]
        else:
            hyps = [(want["path"][b], want["words"][b], int(want["word_lengths"][b]), want["word_confidences"][b])]
        ev_full, ev_cut = word_events(m, x[:, b], tr, L, full), word_events(m, x[:, b], tr, L, cut)
        for path, words, nw, conf in hyps:
            if nw == 0:
                continue
            Z, c = C.confidences_on_sets(m, x[:, b], tr, L, full, path, words, nw, tol, ev_full)
            assert Z == want["normalisers"][b] and np.array_equal(c, conf[:nw]) and not conf[nw:].any()
            Z2, c2 = C.confidences_on_sets(m, x[:, b], tr, L, cut, path, words, nw, tol, ev_cut)
            if Z2 == -np.inf and Z > -np.inf:
                dead += 1
            else:
                diff = max(diff, float(np.abs(np.subtract(c, c2)).max()))
    return wide, diff, dead


@functools.lru_cache(maxsize=None)
def width_conf_regime(pbits, dtype, seed=None):
    """The plain runs of a width from 33 bits on, over CONF_WIDTH_BEAMS and WIDTH_THETAS: the one-best restatement at tolerance 0
    and 2, the 8-row n-best restatement at tolerance 1 -> (pairs >= 2^32 in the sets of the one-best runs at tolerance 0, the
    largest change `without_wide_pairs` makes in a reported value of a lattice that stays alive, the reported hypotheses whose
    lattice dies without those pairs, {(K, theta): the n-best restatement})."""
    lex, lm = C.width_case(pbits)
    x, tr, il = C.width_inputs(pbits, dtype, seed=C.CONF_WIDTH_SEEDS[pbits] if seed is None else seed)
    wide, diff, dead, rows = 0, 0.0, 0, {}
    for K in CONF_WIDTH_BEAMS:
        for theta in C.WIDTH_THETAS:
            for tol in (0, 2):
                n, d, z = wide_pair_effect(lex, lm, x, tr, il, W1, beam_word_conf_ref(x, tr, lex, lm, il, K, theta, *W1, tol), tol)
                wide, diff, dead = wide + (n if tol == 0 else 0), max(diff, d), dead + z
            rows[K, theta] = beam_word_nbest_conf_ref(x, tr, lex, lm, il, K, WIDTH_ROWS, theta, *W1, 1)
            _, d, z = wide_pair_effect(lex, lm, x, tr, il, W1, rows[K, theta], 1)
            diff, dead = max(diff, d), dead + z
    return wide, diff, dead, rows


def assert_width_conf_regime(wide, diff, dead):
    assert wide > 0, "no pair at or above 2^32 in the lattice sets"
    assert diff > MARGIN or dead > 0, "no reported confidence depends on a pair at or above 2^32: the case is not in its regime"


@pytest.mark.parametrize("pbits", sorted(C.CONF_WIDTH_SEEDS))
def test_a_reported_confidence_depends_on_a_pair_above_32_bits(pbits):
    lex, lm = C.width_case(pbits)
    x, tr, il = C.width_inputs(pbits, np.float32, seed=C.CONF_WIDTH_SEEDS[pbits])
    assert (x == np.round(x)).all() and not tr.any()
    info = {}
    beam_word_ref(x, tr, lex, lm, il, 8, INF, *W1, info=info)
    assert info["pbits"] == pbits and info["qbits"] == C.bits_of(word_model(lex, lm, np.float32, *W1).Q)
    wide, diff, dead, _ = width_conf_regime(pbits, np.float32)
    print("pbits %d seed %d: %d pairs >= 2^32 in the sets; without them the largest change of a reported value is %.3g and %d "
          "reported hypotheses lose their lattice" % (pbits, C.CONF_WIDTH_SEEDS[pbits], wide, diff, dead))
    assert_width_conf_regime(wide, diff, dead)


def test_the_33_bit_seed_of_the_search_cases_would_not_bite():
    """Why CONF_WIDTH_SEEDS[33] is not WIDTH_SEEDS[33]: that input keeps pairs >= 2^32 in its sets, and no reported value reads
    them.  The condition of the test above can fail."""
    assert C.CONF_WIDTH_SEEDS[33] != C.WIDTH_SEEDS[33] and C.CONF_WIDTH_SEEDS[35] == C.WIDTH_SEEDS[35]
    wide, diff, dead, _ = width_conf_regime(33, np.float32, seed=C.WIDTH_SEEDS[33])
    print("pbits 33 seed %d: %d pairs >= 2^32 in the sets; without them the largest change of a reported value is %.3g and %d "
          "reported hypotheses lose their lattice" % (C.WIDTH_SEEDS[33], wide, diff, dead))
    assert wide > 0 and not diff > MARGIN and dead == 0
    with pytest.raises(AssertionError, match="not in its regime"):
        assert_width_conf_regime(wide, diff, dead)


# ---------------------------------------------------------------------------------------------------------------- depths
def walk_steps(lm, h, w):
    """The backoff steps of the LM step (h, w), counted from the LM's arrays."""
    n = 0
    while lm.find(h, w) < 0:
        h, n = int(lm.backoff[h]), n + 1
    return n


def depth_conf_regime(depth, form, want, il):
    """From the one-best restatement at K = 8: utterance 0 has two words or more, and a word that ends on a separator edge has
    a confidence inside (0.01, 0.99) -> the set of backoff depths of the LM steps out of the histories of the lattice."""
    lm = C.chain_lm(depth, form)
    nw = int(want["word_lengths"][0])
    assert nw >= 2
    f, c = want["word_frames"][0, :nw], want["word_confidences"][0, :nw]
    assert ((f < int(il[0])) & (c > 0.01) & (c < 0.99)).any(), (f, c)
    hist = {h for Ub in want["sets"] for u in Ub for h, _ in u}
    assert hist and 0 not in hist
    steps = {walk_steps(lm, h, w) for h in hist for w in range(lm.V)}
    if form == "uniform":                                  # every arc leads to the deepest state, and only state 0 holds arcs
        assert lm.start == depth and set(np.asarray(lm.next).tolist()) == {depth} and int(lm.row[1]) == lm.A
        assert all(walk_steps(lm, h, w) == h for h in range(lm.H) for w in range(lm.V))     # h steps down to state 0
        assert hist == {depth} and steps == {depth}        # and the one history a step leaves from is the deepest
    else:
        assert max(steps) == depth and len(steps) > 2
    return steps


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("form", ["uniform", "mixed"])
@pytest.mark.parametrize("depth", [63, 64])
def test_a_confidence_behind_a_walk_of_63_and_64_steps(depth, form, dtype):
    lex, lm = C.small_lexicon(), C.chain_lm(depth, form)
    x, tr, il = C.chain_inputs(dtype)
    want = beam_word_conf_ref(x, tr, lex, lm, il, 8, INF, *W, 1)
    steps = depth_conf_regime(depth, form, want, il)
    nw = int(want["word_lengths"][0])
    print("depth %d %s: walks of %s steps; frames %s confidences %s"
          % (depth, form, sorted(steps), want["word_frames"][0, :nw], np.round(want["word_confidences"][0, :nw], 4)))
    # the bite: a pull whose walk stops one step short loses every word end of the 'uniform' chain -- no event is left
    if form == "uniform":
        m = word_model(lex, lm, dtype, *W)
        m.step = lambda h, w: None if walk_steps(lm, h, w) > depth - 1 else type(m).step(m, h, w)
        Z, P = word_events(m, x[:, 0].astype(np.float64), tr.astype(np.float64), int(il[0]), want["sets"][0])
        assert Z == -np.inf and not P and want["normalisers"][0] > -np.inf


# ---------------------------------------------------------------------------------------------------------------- bound
def bound_lds(elem):
    """The dynamic LDS at K = CONF_BOUND[elem] -> (bytes of the one-best pull, bytes of the n-best pull at BOUND_ROWS rows and
    tolerance BOUND_TOL, bytes the first ring that does not fit would take)."""
    K = C.CONF_BOUND[elem]
    assert K == (160 * 1024 - 256) // (16 + elem)
    one = C.conf_pull_lds(elem, K)
    rows = C.nbest_conf_pull_lds(elem, K, BOUND_ROWS, BOUND_TOL)
    assert 64 * 1024 < one <= C.LDS_MAX and 64 * 1024 < rows <= C.LDS_MAX
    assert C.nbest_conf_ring(K, BOUND_ROWS, BOUND_TOL) == 16
    # the largest ring beside a set at the bound has 4096 slots; 8192 is the first power of two that does not fit
    nb, tol = NO_RING
    assert C.nbest_conf_ring(K, nb, tol - 1) == 4096 and C.nbest_conf_pull_lds(elem, K, nb, tol - 1) <= C.LDS_MAX
    assert C.nbest_conf_ring(K, nb, tol) == 8192
    over = C.nbest_conf_pull_lds(elem, K, nb, tol)
    assert over > C.LDS_MAX
    return one, rows, over


def bound_regime(elem, sets):
    """A source set -- a frame with a successor -- of exactly K = CONF_BOUND[elem] pairs: at G = subgroup(K) = 1 lane per pair
    the k0 loop of the pull takes ceil(K / 1024) > 1 passes."""
    K = C.CONF_BOUND[elem]
    assert C.subgroup(K) == 1 and -(-K // C.THREADS) > 1
    sizes = [[len(u) for u in Ub] for Ub in sets]
    assert any(n == K for z in sizes for n in z[:-1]) and max(max(z) for z in sizes) == K, sizes
    return sizes


@pytest.mark.parametrize("elem", [4, 8], ids=["f32", "f64"])
def test_a_source_set_at_the_lattice_bound(elem):
    K = C.CONF_BOUND[elem]
    lex, lm = C.wide_case()
    x, tr, il = C.wide_inputs(np.float32 if elem == 4 else np.float64)
    info = {}
    beam_word_ref(x, tr, lex, lm, il, K, INF, *WW, info=info)
    sizes = bound_regime(elem, info["kept"])
    one, rows, over = bound_lds(elem)
    print("elem %d K %d: sets of %s; LDS of the one-best pull %d bytes, of the n-best pull %d bytes (nbest %d tol %d), "
          "%d bytes with a ring of 8192 slots (nbest %d tol %d)" % ((elem, K, sizes, one, rows, BOUND_ROWS, BOUND_TOL, over) + NO_RING))
    assert sizes[0][:3] == [39, 319, 2101]                 # the beam fills from the fourth frame on


# ---------------------------------------------------------------------------------------------------------------- lanes
def lanes_conf_regime(K, info):
    """From the search's `info`: a source set of exactly K pairs, the lattice pass's lanes per source pair, and the longest row
    among those pairs -> (G, row)."""
    G, row = lanes_regime(K, info)
    assert C.subgroup(K) == G == C.beam_lanes_per_state(K)
    assert row == 39 and (row > G) == (K > 16)
    return G, row


@pytest.mark.parametrize("K", C.LANE_BEAMS)
def test_lanes_per_source_pair(K):
    lex, lm = C.wide_case()
    x, tr, il = C.wide_inputs()
    info = {}
    beam_word_ref(x, tr, lex, lm, il, K, INF, *WW, info=info)
    G, row = lanes_conf_regime(K, info)
    print("K %d: G %d, longest row %d" % (K, G, row))
    assert [C.subgroup(m) for m in (16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513)] == [64, 32, 32, 16, 16, 8, 8, 4, 4, 2, 2, 1]
