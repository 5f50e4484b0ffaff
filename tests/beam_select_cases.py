"""Inputs shared by the CPU and GPU tests of the per-frame select of the beam search (the end of `beam_frame` in
csrc/asg_beam_frame.h and its copy in csrc/asg_beam_word_frame.h) at the sizes where it changes shape
(tests/test_beam_select_regimes_cpu.py, tests/test_hip_beam_select_regimes.py).  Every input is built for ONE regime:

  key widths   a one-state automaton over N = 200 labels with all weights 0.  Label 199 is a witness (below); the other 199 are
               the candidates of a frame, and a frame is a list of 199 values handed to the labels in a random order.  The
               values are V - k ulp with V = 1 + (2^m - 1) ulp (all the low mantissa bits of V set: m = 20 in float32, 44 in
               float64), so that enc(V) ^ enc(V - k ulp) = k and the width `rem` of the key select is the bit length of the
               largest k: the list chooses it.  The largest candidate is V itself, so the next frame starts from V again, and a
               frame's emissions are value - V (value itself in a first frame): exact, and the same lists serve both dtypes.
  the witness  With zero transitions every label's best source is the best kept state, so the five outputs would not depend on
               what else a select keeps.  Row 199 of the transitions therefore holds g[j] = 4 * (rank of label j in the frame
               under test, value descending, label ascending), label 199 emits -inf (it is no candidate) except in a last
               frame where it alone emits 0: the score is then (v + g) of the LOWEST-ranked state the select kept, and the path
               names it.  A select that keeps another set changes score and path.
  state widths random deterministic automata with zero weights, zero transitions and emissions in {-1, 0, 1}, their number of
               product states Q just below and above 2^8 and 2^16, and above 2^17: the tie select over q walks 1, 2 (8 | 1),
               2 (8 | 8), 3 (8 | 8 | 1) and 3 (8 | 8 | 2) digits.  Half of the automaton's states send two labels to one state, which makes neighbouring product
               states that tie whenever the two labels emit the same: cuts decided in the narrow last digit.
  lanes, LDS   one automaton with rows of 69 arcs and beams around every halving of the lanes per state; K = 8192 with the
               transitions on either side of the LDS bound.

Q of 25 bits and more (a fourth digit of the tie select) needs 2^24 product states and is out of scope; 19 to 24 bits add no
digit to the 18 bits here and only cost time.  The launch arithmetic of csrc/asg_beam_graph.hip is restated below;
the tests assert their regimes from it and from the restatement's `info`, never from the device."""
import functools

import numpy as np

from beam_decode_ref import digit_shifts, q_bits

INF = float("inf")
FIXED_LDS = 4096                   # kFixedLds
LDS_MAX = 160 * 1024               # kLdsMax
THREADS = 1024                     # kBT
MAX_K = 8192                       # kBeamMaxK


def beam_lanes_per_state(K):
    G = 1
    while G < 64 and G * 2 * K <= THREADS:
        G *= 2
    return G


def graph_lds(K, N, elem):
    """launch_beam_graph: control block, the kept set (value, q), 8 bytes, and [N][N] transitions when they fit."""
    return FIXED_LDS + K * (elem + 4) + 8 + N * N * elem


def transitions_in_lds(K, N, elem):
    return graph_lds(K, N, elem) <= LDS_MAX


def deciding_digit(a, b, Q):
    """The first digit of the tie select over q, from the top, in which the states a and b differ."""
    for d, (shift, w) in enumerate(digit_shifts(q_bits(Q))):
        if (a >> shift) != (b >> shift):
            return d
    raise AssertionError("equal states")


def _graph(nxt, final=None):
    from torch_asg_amd import TokenGraph
    nxt = np.asarray(nxt, np.int64)
    return TokenGraph(nxt, np.zeros(nxt.shape), np.zeros(nxt.shape[0]) if final is None else final)


# ------------------------------------------------------------------------------------------------------------ key widths
N_KEY = 200
WITNESS = N_KEY - 1
K_KEY = 7
ONES = {np.float32: 20, np.float64: 44}
ULP = {np.float32: 2.0 ** -23, np.float64: 2.0 ** -52}


def base_value(dtype):
    return dtype(1.0) + dtype((2 ** ONES[dtype] - 1) * ULP[dtype])


def _ks(bits, seed, kind="distinct-cut"):
    """199 offsets k in ascending order (the best candidate first), the largest 2^bits - 1.  Positions K_KEY - 1 and K_KEY,
    the two sides of the cut at K = 7, hold a and a + 1 with a even: they differ in bit 0 alone, so a select that ignores
    its last digit ties them.  'ties-taken': positions 4..6 hold a (the K-th key's ties end at the cut); 'ties-cut':
    positions 5..8 hold a (the cut falls among four equal keys)."""
    rng = np.random.default_rng(seed)
    top = 2 ** bits - 1
    n = N_KEY - 1
    a = 2 * int(rng.integers(1, max(2, min(2 ** (bits - 1), 2 ** 40) - 1)))
    assert a + 1 <= top
    head = sorted(int(v) for v in rng.integers(0, a + 1, K_KEY - 2))
    tail = sorted(int(v) for v in rng.integers(a + 1, top + 1, n - K_KEY - 2))
    ks = [0] + head + [a, a + 1] + tail + [top]
    if kind == "ties-taken":
        ks[4:7] = [a] * 3
    elif kind == "ties-cut":
        ks[5:9] = [a] * 4
    else:
        assert kind == "distinct-cut"
    ks = sorted(ks)
    assert len(ks) == n and ks[0] == 0 and ks[-1] == top and ks == sorted(ks)
    return ks


# name -> (the width `rem` at an infinite threshold, the exit at K = 7 and an infinite threshold, the wrong select that has to
# change the outputs there, how the frame is built).  'equal': ten candidates at V, the others -inf.  'zero': 0.25 .. 0.125
# and 196 negative values: candidates on both sides of zero, the full width of the key.
KEY_FRAMES = {
    "rem0-equal": (0, "equal-cut", "ties_from_top", ("equal", 10)),
    "rem3": (3, "kth-ties-taken", "low_bits", ("ulp", 3, "distinct-cut")),
    "rem8": (8, "kth-ties-taken", "last_digit", ("ulp", 8, "distinct-cut")),
    "rem9": (9, "kth-ties-taken", "low_bits", ("ulp", 9, "distinct-cut")),
    "rem16": (16, "kth-ties-taken", "last_digit", ("ulp", 16, "distinct-cut")),
    "rem17": (17, "kth-ties-taken", "low_bits", ("ulp", 17, "distinct-cut")),
    "rem20": (20, "kth-ties-taken", "low_bits", ("ulp", 20, "distinct-cut")),
    "rem12-ties-taken": (12, "kth-ties-taken", "low_bits", ("ulp", 12, "ties-taken")),
    "rem12-ties-cut": (12, "tie-select", "ties_from_top", ("ulp", 12, "ties-cut")),
    "rem40": (40, "kth-ties-taken", "last_digit", ("ulp", 40, "distinct-cut")),          # float64 alone
    "full-width": (None, "kth-ties-taken", "raw_bits", ("zero",)),                       # rem = kBits
}


def key_frame_names(dtype):
    return [n for n in KEY_FRAMES if n != "rem40" or dtype == np.float64]


@functools.lru_cache(maxsize=None)
def key_frame(name, dtype):
    """-> (values [199] by label, -inf where the label is no candidate; the finite threshold of the case, which cuts inside
    the band of the values)."""
    how = KEY_FRAMES[name][3]
    seed = sorted(KEY_FRAMES).index(name)
    rng = np.random.default_rng(100 + seed)
    n = N_KEY - 1
    V, ulp = base_value(dtype), ULP[dtype]
    if how[0] == "equal":
        by_rank = np.full(n, -np.inf, dtype)
        by_rank[:how[1]] = V
        theta = 1.0
    elif how[0] == "ulp":
        ks = _ks(how[1], seed, how[2])
        by_rank = np.array([dtype(1.0) + dtype((2 ** ONES[dtype] - 1 - k) * ulp) for k in ks], dtype)
        theta = ks[11] * ulp
    else:
        by_rank = np.concatenate([[0.25, 0.1875, 0.125], -1.75 - np.arange(n - 3) / 256.0]).astype(dtype)
        theta = 2.1
    order = rng.permutation(n)                             # order[p]: the label of the p-th value
    lo = K_KEY - 3 + int(np.argmin(order[K_KEY - 3:K_KEY + 1]))
    order[[lo, K_KEY]] = order[[K_KEY, lo]]                # the first value dropped sits at the smallest label around the cut
    vals = np.empty(n, dtype)
    vals[order] = by_rank
    return vals, theta


@functools.lru_cache(maxsize=None)
def key_case(name, dtype):
    """The frame `name` under test in three utterances: behind another frame, as the first frame, and behind a second other
    frame; the witness frame behind each.  -> x [3][3][200], tr [200][200], lengths, threshold; x and tr read-only."""
    names = [n for n in key_frame_names(dtype) if n not in (name, "full-width")]
    at = key_frame_names(dtype).index(name)
    before = [names[at % len(names)], None, names[(at + 3) % len(names)]]
    V = base_value(dtype)
    vals, theta = key_frame(name, dtype)
    x = np.zeros((3, 3, N_KEY), dtype)
    lengths = np.array([3, 2, 3])
    cands = []
    with np.errstate(invalid="ignore"):
        for b, prev in enumerate(before):
            frames = [vals] if prev is None else [key_frame(prev, dtype)[0], vals]
            for t, f in enumerate(frames):
                x[t, b, :WITNESS] = f - (V if t else dtype(0))
                x[t, b, WITNESS] = -np.inf
            x[len(frames), b, :WITNESS] = -np.inf
            cands.append((V if prev is not None else dtype(0)) + x[len(frames) - 1, b, :WITNESS])
    ranks = [np.lexsort((np.arange(WITNESS), -c)) for c in cands]
    assert all((r == ranks[0]).all() for r in ranks), "the frame ranks its labels alike wherever it stands"
    tr = np.zeros((N_KEY, N_KEY), dtype)
    tr[WITNESS, ranks[0]] = 4.0 * np.arange(WITNESS)
    x.setflags(write=False), tr.setflags(write=False)
    return x, tr, lengths, theta


@functools.lru_cache(maxsize=None)
def one_state():
    return _graph(np.zeros((1, N_KEY)))


def key_rem(name, dtype):
    rem = KEY_FRAMES[name][0]
    return 8 * np.dtype(dtype).itemsize if rem is None else rem


def key_thresholds(name, dtype):
    """infinity, 0 (only the ties of the maximum pass: rem = 0) and the case's finite threshold."""
    return (INF, 0.0, key_case(name, dtype)[3])


def key_beams(passing):
    """Below, at and above the count that passes the threshold."""
    return sorted({min(K_KEY, max(1, passing - 1)), passing, passing + 1})


# ----------------------------------------------------------------------------------------------------------- the word copy
@functools.lru_cache(maxsize=None)
def word_case():
    """199 words of one token each and a unigram LM of one state: with lm_weight = word_score = 0 a frame behind a separator
    has the candidates of the one-state automaton, and the separator (label 199) is the witness."""
    from torch_asg_amd import Lexicon, WordLM
    V = N_KEY - 1
    lex = Lexicon([[i] for i in range(V)], N_KEY, WITNESS)
    lm = WordLM(V, np.array([0, V]), np.arange(V), np.zeros(V), np.zeros(V, np.int64), np.array([-1]), np.zeros(1), 0, np.zeros(1))
    return lex, lm


@functools.lru_cache(maxsize=None)
def word_key_case(name, dtype):
    """Utterance 0: the best label alone at V, the separator, the frame under test, the separator; utterance 1: the frame
    under test, the separator.  -> x [4][2][200], tr, lengths, threshold."""
    xk, tr, _, theta = key_case(name, dtype)
    V = base_value(dtype)
    best = int(np.argmin(tr[WITNESS, :WITNESS]))
    x = np.full((4, 2, N_KEY), -np.inf, dtype)
    x[0, 0, best] = V
    x[1, 0, WITNESS] = 0
    x[2, 0] = xk[1, 0]
    x[3, 0, WITNESS] = 0
    x[0, 1] = xk[0, 1]
    x[1, 1, WITNESS] = 0
    x[2:, 1] = 0
    x.setflags(write=False)
    return x, tr, np.array([4, 2]), theta


# ---------------------------------------------------------------------------------------------------------- state widths
# bits of q -> (automaton states S, seed of the automaton, seed of the emissions): Q is asserted by the CPU test
WIDTHS = {8: (70, 1, 0), 9: (100, 1, 0), 16: (14000, 1, 2), 17: (22000, 1, 12), 18: (45000, 1, 1)}
WIDTH_N = 6
WIDTH_THETAS = (INF, 1.0)


def width_beams(bits):
    """K = 200 touches more than 1024 states in a frame; K = 2000 is a beam above 1024."""
    return (3, 8, 33, 200) if bits < 16 else (3, 8, 33, 200, 2000)


@functools.lru_cache(maxsize=None)
def width_graph(bits):
    S, seed, _ = WIDTHS[bits]
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, S, (S, WIDTH_N))
    twin = rng.random(S) < 0.5
    nxt[twin, 1] = nxt[twin, 0]                            # labels 0 and 1 enter one state: product states that are neighbours
    nxt[twin, 3] = nxt[twin, 2]
    nxt[rng.random((S, WIDTH_N)) < 0.3] = -1
    nxt[0] = rng.integers(0, S, WIDTH_N)                   # the start state has every arc
    return _graph(nxt, np.where(rng.random(S) < 0.5, 0.0, -np.inf))


@functools.lru_cache(maxsize=None)
def width_inputs(bits, dtype):
    """Emissions [10][2][6] in {-1, 0, 1}; in half of the frames labels 0 | 1 and 2 | 3 emit alike, so the twins tie."""
    rng = np.random.default_rng(WIDTHS[bits][2])
    x = rng.integers(-1, 2, (10, 2, WIDTH_N))
    same = rng.random((10, 2)) < 0.5
    x[..., 1] = np.where(same, x[..., 0], x[..., 1])
    x[..., 3] = np.where(same, x[..., 2], x[..., 3])
    x = x.astype(dtype)
    tr = np.zeros((WIDTH_N, WIDTH_N), dtype)
    x.setflags(write=False), tr.setflags(write=False)
    return x, tr, np.array([10, 9])


# ----------------------------------------------------------------------------------------------------------------- lanes
LANE_BEAMS = (8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513)
LANE_N = 70


@functools.lru_cache(maxsize=None)
def lane_graph():
    """20 states, every arc present: each product state has a row of 69 arcs, more than the 64 lanes of a wavefront."""
    rng = np.random.default_rng(41)
    return _graph(rng.integers(0, 20, (20, LANE_N)))


@functools.lru_cache(maxsize=None)
def lane_inputs(dtype=np.float32):
    """Flat emissions [4][2][70]: every frame behind the first fills the beam."""
    rng = np.random.default_rng(43)
    x = (0.25 * rng.standard_normal((4, 2, LANE_N))).astype(dtype)
    tr = (0.25 * rng.standard_normal((LANE_N, LANE_N))).astype(dtype)
    x.setflags(write=False), tr.setflags(write=False)
    return x, tr, np.array([4, 3])


# ------------------------------------------------------------------------------------------------------------------- LDS
# (elem, K, the last N with the transitions in LDS): the first N in global memory is the next one
LDS_STEPS = [(4, MAX_K, 153), (8, MAX_K, 87)]


@functools.lru_cache(maxsize=None)
def lds_graph(N):
    """200 states over N labels: more than 8192 product states, so that K = 8192 is not clamped."""
    rng = np.random.default_rng(47)
    return _graph(rng.integers(0, 200, (200, N)))


@functools.lru_cache(maxsize=None)
def lds_inputs(N, dtype):
    rng = np.random.default_rng(53)
    x = rng.standard_normal((3, 2, N)).astype(dtype)
    tr = rng.standard_normal((N, N)).astype(dtype)
    x.setflags(write=False), tr.setflags(write=False)
    return x, tr, np.array([3, 2])
