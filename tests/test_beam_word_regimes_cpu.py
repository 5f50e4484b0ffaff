"""CPU tests of the inputs of tests/test_hip_beam_word_regimes.py (tests/beam_word_regime_cases.py): from the numpy restatements
and the restated launch arithmetic ALONE, every case is in the regime it names -- the pair widths and the digit of the tie
select in which every cut falls, the depth of the LM walks, the side of the LDS bound, the lanes per kept pair against the
longest outgoing row -- and every case can tell a subtly wrong kernel from a right one: the restatement run with a wrong rank
of the pairs (the low 32 bits; the second digit of the tie select cleared) or with the walk bounded one step short gives other
outputs.  A case whose wrong variant gave the same outputs would not be in its regime."""
import numpy as np
import pytest

import beam_word_regime_cases as C
from beam_word_la_ref import beam_word_la_ref, truncated_state
from beam_word_ref import beam_word_ref

INF = float("inf")
NAMES = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths")
W1 = (1.0, 1.0, 0.0)               # lm_weight, word_score, token_score of case 1: integers stay integers
W = (0.7, -0.4, 0.3)


def _same(a, b):
    return all(a[n].tobytes() == b[n].tobytes() for n in NAMES)


def width_regime(pbits, info):
    """What the restatement's `info` of one run shows of a width's regime -> a dict of counts."""
    qb = info["qbits"]
    assert info["pbits"] == pbits and qb == C.bits_of(info["Q"])
    digits = [C.deciding_digit(a, b, qb, pbits) for _, _, a, b in info["cuts"]]
    tied = [s for _, _, _, s in info["tied"] if len({h for h, _ in s}) > 1]
    return dict(top=sum(d == 0 for d in digits), lower=sum(d > 0 for d in digits), digits=sorted(set(digits)),
                cut32=sum(C.deciding_bit(a, b, qb) >= 32 for _, _, a, b in info["cuts"]), other_h=len(tied),
                tie32=sum(C.deciding_bit(s[0], s[1], qb) >= 32 for s in tied))


def assert_width_regime(pbits, total):
    assert total["top"] > 0, "no cut whose two pairs first differ in the top digit"
    assert total["lower"] > 0 or pbits <= 8, "no cut decided in a lower digit"
    assert total["other_h"] > 0, "no source tie between different histories"
    if pbits >= 33:
        assert total["cut32"] > 0 and total["tie32"] > 0, "no cut / no source tie decided at or above bit 32"


# ---------------------------------------------------------------------------------------------------------------- arithmetic
def test_the_restated_launch_arithmetic():
    assert [C.bits_of(n) for n in (1, 2, 3, 7, 8, 9, 32, 33, 2830, 1 << 20, (1 << 20) + 1, (1 << 22) + 1)] == \
        [1, 1, 2, 3, 3, 4, 5, 6, 12, 20, 21, 23]
    assert [C.beam_lanes_per_state(K) for K in C.LANE_BEAMS] == [64, 64, 64, 32, 32, 16, 16, 8, 8, 4, 4, 2, 2, 1]
    assert [C.beam_lanes_per_state(K) for K in (1, 1024, 8192)] == [64, 1, 1]
    assert C.digit_shifts(6) == [(0, 6)] and C.digit_shifts(9) == [(1, 8), (0, 1)] and C.digit_shifts(16) == [(8, 8), (0, 8)]
    assert C.digit_shifts(33) == [(25, 8), (17, 8), (9, 8), (1, 8), (0, 1)] and C.digit_shifts(35)[-1] == (0, 3)
    for elem, K, N in C.LDS_STEPS:
        assert C.transitions_in_lds(K, N, elem) and not C.transitions_in_lds(K, N + 1, elem), (elem, K, N)
        print("elem %d K %d: N = %d takes %d bytes of LDS, N = %d would take %d; the launch asks for %d and %d"
              % (elem, K, N, C.beam_lds(K, N, elem), N + 1, C.beam_lds(K, N + 1, elem), C.dynamic_lds(K, N, elem),
                 C.dynamic_lds(K, N + 1, elem)))
    assert C.LDS_STEPS == [(4, 8, 199), (8, 8, 141), (4, 8192, 123), (8, 8192, 59)]
    assert all(C.dynamic_lds(8192, N, elem) > 64 * 1024 for elem, K, N0 in C.LDS_STEPS if K == 8192 for N in (N0, N0 + 1))


# ---------------------------------------------------------------------------------------------------------------- case 1
@pytest.mark.parametrize("pbits", sorted(C.WIDTHS))
def test_pair_width_regimes_and_their_bite(pbits):
    lex, lm = C.width_case(pbits)
    x, tr, il = C.width_inputs(pbits, np.float32)
    assert (x == np.round(x)).all() and not tr.any()
    total, bites = {}, {"cut": 0, "source": 0}
    wrong = C.low32 if pbits >= 33 else C.without_second_digit(pbits) if pbits in (9, 17) else None
    for K in C.width_beams(pbits):
        for theta in C.WIDTH_THETAS:
            info = {}
            want = beam_word_ref(x, tr, lex, lm, il, K, theta, *W1, info=info)
            assert np.isfinite(want["scores"]).all()
            for k, v in width_regime(pbits, info).items():
                total[k] = sorted(set(total.get(k, [])) | set(v)) if k == "digits" else total.get(k, 0) + v
            for where in bites if wrong is not None else ():
                bites[where] += not _same(want, beam_word_ref(x, tr, lex, lm, il, K, theta, *W1, rank=wrong, rank_where=(where,)))
    print("pbits %d: Q %d qbits %d H %d; %s; runs whose outputs a wrong rank changes: %s"
          % (pbits, info["Q"], info["qbits"], lm.H, total, bites))
    assert info["pbits"] == C.bits_of(lm.H) + C.bits_of(info["Q"]) == pbits
    assert_width_regime(pbits, total)
    if wrong is not None:                                  # the wrong rank at the cut alone, and between the sources of a target alone
        assert bites["cut"] > 0 and bites["source"] > 0, "the wrong rank gives the same eight outputs: the case is not in its regime"
    # the forced pairs of the loss cases: the history behind the last word is the largest state
    tg, tl = C.last_word_target(lex)
    assert int(lm.next[lm.find(0, lex.num_words - 1)]) == lm.H - 1 and tg[0, tl[0] - 1] != lex.separator


def test_the_whole_array_form_of_the_truncated_states_is_the_loop():
    for lm in (C.spread_lm(5, 8193), C.chain_lm(64, "mixed"), C.chain_lm(63, "uniform"), C.array_bigram(300, 72, 0.03)):
        for order in (1, 2, 3, 30, 65):
            loop = truncated_state(lm, order, whole_arrays=False)
            assert truncated_state(lm, order, whole_arrays=True) == loop
            assert all(type(h) is int for h in loop[:4])
    lm = C.spread_lm(5, 8193)                               # (above the size at which the default changes form)
    assert truncated_state(lm, 1) == [0] * lm.H and truncated_state(lm, 2) == list(range(lm.H))
    assert truncated_state(C.chain_lm(64, "mixed"), 30) == [min(h, 29) for h in range(65)]


# ---------------------------------------------------------------------------------------------------------------- case 2
def test_a_chain_of_65_backoff_steps_is_refused():
    for form in ("uniform", "mixed"):
        assert C.chain_lm(C.MAX_BACKOFF - 1, form).H == 64 and C.chain_lm(C.MAX_BACKOFF, form).H == 65
        with pytest.raises(ValueError, match="64 steps"):
            C.chain_lm(C.MAX_BACKOFF + 1, form)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("form", ["uniform", "mixed"])
@pytest.mark.parametrize("depth", [63, 64])
def test_backoff_depth_regimes_and_their_bite(depth, form, dtype):
    from torch_asg_amd import WordLookahead
    lex, lm = C.small_lexicon(), C.chain_lm(depth, form)
    assert lm.start == depth and (lm.backoff == np.arange(-1, depth)).all()
    assert (lm.bow[1:] != np.round(lm.bow[1:])).all() and (lm.logp != np.round(lm.logp)).all()
    la = WordLookahead(lex, lm, 65)
    assert la.depth[la.la_state].max() == depth            # look() takes `depth` steps from the deepest state
    x, tr, il = C.chain_inputs(dtype)
    steps = set()
    for h in range(lm.H):
        for w in range(lm.V):
            n, s = 0, h
            while lm.find(s, w) < 0:
                s, n = int(lm.backoff[s]), n + 1
            steps.add(n)
    assert max(steps) == depth and (steps == set(range(depth + 1)) if form == "uniform" else len(steps) > 2)
    bites = 0
    for K in (1, 8):
        want = beam_word_ref(x, tr, lex, lm, il, K, INF, *W)
        assert want["word_lengths"][0] >= 2 and np.isfinite(want["scores"][:2]).all()     # a walk on a separator edge and at the end
        short = beam_word_ref(x, tr, lex, lm, il, K, INF, *W, max_backoff=depth - 1)
        if form == "uniform":                              # every walk takes the full depth: one step short rejects every word
            assert (short["scores"] == -np.inf).all() and (short["words"] == -1).all()
        bites += not _same(want, short)
        assert _same(want, beam_word_ref(x, tr, lex, lm, il, K, INF, *W, max_backoff=depth))
        for order in (1, 2, 65):                           # (the restatement's own assertions hold: every kept pair's look-ahead is finite)
            ahead = beam_word_la_ref(x, tr, lex, lm, order, il, K, INF, *W)
            assert np.isfinite(ahead["scores"][0]) and ahead["word_lengths"][0] >= 2       # look() on a separator edge and at the end
            assert (ahead["scores"] <= beam_word_ref(x, tr, lex, lm, il, 1024, INF, *W)["scores"] + 1e-4).all()
    assert bites > 0
    print("depth %d %s: walks of %s steps" % (depth, form, sorted(steps) if len(steps) < 8 else "0 .. %d" % max(steps)))


# ---------------------------------------------------------------------------------------------------------------- case 3
@pytest.mark.parametrize("elem,K,N0", C.LDS_STEPS)
def test_both_sides_of_every_lds_step(elem, K, N0):
    dt = np.float32 if elem == 4 else np.float64
    for N in (N0, N0 + 1):
        lex, lm = C.layout_case(N)
        assert lex.graph.N == N and lex.separator == N - 1
        x, tr, il = C.layout_inputs(N, dt)
        info = {}
        want = beam_word_ref(x, tr, lex, lm, il, min(K, 8), INF, *W, info=info)
        assert want["word_lengths"][0] >= 2 and max(max(z) for z in info["sizes"]) > 1
        assert C.transitions_in_lds(K, N, elem) == (N == N0)


# ---------------------------------------------------------------------------------------------------------------- case 4
def lanes_regime(K, info):
    """-> (G, the longest outgoing row among the kept pairs of a frame that has a successor and keeps exactly K pairs)."""
    G = C.beam_lanes_per_state(K)
    deg = info["out_degree"]
    rows = [max(deg[q] for _, q in kept) for kl in info["kept"] for kept in kl[:-1] if len(kept) == K]
    assert rows, "no frame with a successor keeps exactly K pairs"
    return G, max(rows)


@pytest.mark.parametrize("K", C.LANE_BEAMS)
def test_lanes_per_pair_regimes(K):
    lex, lm = C.wide_case()
    x, tr, il = C.wide_inputs()
    info = {}
    beam_word_ref(x, tr, lex, lm, il, K, INF, 0.5, -0.2, 0.1, info=info)
    G, row = lanes_regime(K, info)
    print("K %d: G %d, longest row %d (the separator state's: %d)" % (K, G, row, info["out_degree"][info["sep_q"][0]]))
    # a row of 39 edges -- the trie root's, behind the separator state -- takes more than one stride of G lanes wherever
    # G < 64; at K <= 16 a pair has the whole wavefront and no row over 40 tokens can be longer
    assert row == 39 and (row > G) == (K > 16)
