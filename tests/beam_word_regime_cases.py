"""Inputs shared by the CPU and GPU tests of the lexicon + word-LM beam family at the sizes where the frame they all compile
(csrc/asg_beam_word_frame.h) changes shape (tests/test_beam_word_regimes_cpu.py, tests/test_hip_beam_word_regimes.py): pairs
h << qbits | q wider than one 8-bit digit of the tie select and wider than 32 bits, LM walks of 63 and 64 backoff steps,
transitions on both sides of the LDS bound, and beams at which the lanes per kept pair halve.

Every language model here is built from arrays (no ARPA text: its Python loops are quadratic in the vocabulary) and every
builder is memoised, so that a module builds the large lexicon and the large LM once.  The launch arithmetic of the frame is
restated in Python below; the tests assert their regimes from it and from the restatements' own `info`, never from the device.
"""
import functools

import numpy as np

FIXED_LDS = 4096                   # kFixedLds: histograms, counters, reduction slots
LDS_MAX = 160 * 1024               # kLdsMax
THREADS = 1024                     # kBT
MAX_BACKOFF = 64                   # kMaxBackoff


def bits_of(n):
    """The frame's bits_of: the bits that hold 0 .. n - 1, at least 1."""
    return max(1, int(n - 1).bit_length())


def beam_lanes_per_state(K):
    G = 1
    while G < 64 and G * 2 * K <= THREADS:
        G *= 2
    return G


def beam_lds(K, N, elem):
    """Bytes of LDS of a search kernel with the transitions inside: control block, the kept set (value, q, h), [N][N]."""
    return FIXED_LDS + K * (elem + 8) + N * N * elem


def transitions_in_lds(K, N, elem):
    return beam_lds(K, N, elem) <= LDS_MAX


def dynamic_lds(K, N, elem):
    """What the launch asks for: without the matrix when it does not fit."""
    return beam_lds(K, N, elem) if transitions_in_lds(K, N, elem) else FIXED_LDS + K * (elem + 8)


def digit_shifts(pbits):
    """The tie select walks a pair's pbits bits from the top in digits of 8 bits, the last one narrower: [(shift, width)]."""
    out, prem = [], pbits
    while prem > 0:
        w = min(prem, 8)
        out.append((prem - w, w))
        prem -= w
    return out


def pair_int(p, qbits):
    return int(p[0]) << qbits | int(p[1])


def deciding_digit(a, b, qbits, pbits):
    """The first digit, from the top, in which the pairs a and b differ."""
    a, b = pair_int(a, qbits), pair_int(b, qbits)
    for d, (shift, w) in enumerate(digit_shifts(pbits)):
        if (a >> shift) != (b >> shift):
            return d
    raise AssertionError("equal pairs")


def deciding_bit(a, b, qbits):
    return (pair_int(a, qbits) ^ pair_int(b, qbits)).bit_length() - 1


def low32(p):
    """A wrong rank: the pair cut to its low 32 bits."""
    return p & 0xFFFFFFFF


def without_second_digit(pbits):
    """A wrong rank: the pair with the bits of the tie select's second digit cleared."""
    shift, w = digit_shifts(pbits)[1]
    mask = ((1 << w) - 1) << shift
    return lambda p: p & ~mask


# ---------------------------------------------------------------------------------------------------------------- case 1
SMALL_WORDS = [[0], [0, 1], [1, 0], [2], [0, 1, 2]]      # N = 5: tokens 0..3, separator 4 (tests/beam_word_cases.py)


@functools.lru_cache(maxsize=None)
def small_lexicon():
    from torch_asg_amd import Lexicon
    return Lexicon(SMALL_WORDS, 5, 4)


@functools.lru_cache(maxsize=None)
def big_lexicon():
    """2500 random words of 1 to 3 tokens over the tokens 0 .. 38, separator 39; the last word is a one-token word, so that
    the history it leads to (the largest of `spread_lm`) is cheap to reach."""
    from torch_asg_amd import Lexicon
    rng = np.random.default_rng(11)
    words, seen = [], set()
    while len(words) < 2500:
        n = int(rng.integers(1, 4))
        w = tuple(int(t) for t in rng.integers(0, 39, n))
        if w in seen or any(a == b for a, b in zip(w, w[1:])):
            continue
        seen.add(w)
        words.append(list(w))
    one = max(i for i, w in enumerate(words) if len(w) == 1)
    words.append(words.pop(one))
    return Lexicon(words, 40, 39)


@functools.lru_cache(maxsize=None)
def spread_lm(V, H, seed=3):
    """Row 0 holds every unigram, its next states spread evenly over [1, H) (word V - 1 leads to H - 1); every other state has
    no arc and backs off to state 0.  Small integer weights.  The LM moves to a state that depends on the word alone, so word
    ends fan in from different histories."""
    from torch_asg_amd import WordLM
    rng = np.random.default_rng(seed)
    row = np.full(H + 1, V, np.int64)
    row[0] = 0
    nxt = 1 + (np.arange(V, dtype=np.int64) * (H - 2)) // max(V - 1, 1)
    backoff = np.zeros(H, np.int64)
    backoff[0] = -1
    bow = rng.integers(-1, 1, H).astype(np.float64)
    bow[0] = 0.0
    return WordLM(V, row, np.arange(V), rng.integers(-2, 1, V).astype(np.float64), nxt, backoff, bow, 0,
                  rng.integers(-1, 1, H).astype(np.float64))


# pbits -> (lexicon, H): qbits is 3 for the small lexicon and 12 for the big one (asserted from the compiled graph)
WIDTHS = {8: ("small", 32), 9: ("small", 33), 16: ("small", 8192), 17: ("small", 8193),
          32: ("big", 1 << 20), 33: ("big", (1 << 20) + 1), 35: ("big", (1 << 22) + 1)}


# the seeds of `width_inputs`, chosen so that the restatement ALONE shows each width's regime over WIDTH_BEAMS and WIDTH_THETAS
# (tests/test_beam_word_regimes_cpu.py asserts it)
WIDTH_SEEDS = {8: 0, 9: 40, 16: 0, 17: 2, 32: 0, 33: 20, 35: 11}
WIDTH_THETAS = (float("inf"), 1.0)


def width_beams(pbits):
    return (2, 3, 5, 8) if pbits < 32 else (8, 64, 300)


def width_case(pbits):
    kind, H = WIDTHS[pbits]
    lex = small_lexicon() if kind == "small" else big_lexicon()
    return lex, spread_lm(lex.num_words, H)


def width_inputs(pbits, dtype, seed=None):
    """Integer emissions [8][2][N] and a zero transition matrix: ties abound.  Utterance 0 leans towards the last word and a
    separator at its start, which puts the largest history into the beam beside the others."""
    lex, lm = width_case(pbits)
    N = lex.graph.N
    rng = np.random.default_rng(WIDTH_SEEDS[pbits] if seed is None else seed)
    x = rng.integers(-2, 3, (8, 2, N))
    last = _spellings(lex)[lex.num_words - 1]
    for b, t0 in ((0, 0), (1, 2)):
        for t, lab in enumerate(last + [lex.separator]):
            x[t0 + t, b, lab] += 1
    x = x.astype(dtype)
    return x, np.zeros((N, N), dtype), np.array([8, 7])


def last_word_target(lex, S=6):
    """[2][S] targets and their lengths: the last word, a separator, the first word -- the pairs behind that separator have the
    largest spread state as their history."""
    spell = _spellings(lex)
    sep = lex.separator
    a = spell[lex.num_words - 1] + [sep] + spell[0]
    b = spell[lex.num_words - 1] + [sep]
    tg = np.zeros((2, S), np.int64)
    tg[0, :len(a)], tg[1, :len(b)] = a, b
    return tg, np.array([len(a), len(b)])


def _spellings(lex):
    """word id -> tokens, read back from the trie."""
    nxt, wos, sep = np.asarray(lex.graph.next), lex.word_of_state, lex.separator
    out = {}
    stack = [(0, [])]
    while stack:
        n, toks = stack.pop()
        if wos[n] >= 0:
            out[int(wos[n])] = toks
        for x in np.flatnonzero(nxt[n] >= 0):
            if x != sep:
                stack.append((int(nxt[n, x]), toks + [int(x)]))
    return out


# ---------------------------------------------------------------------------------------------------------------- case 2
@functools.lru_cache(maxsize=None)
def chain_lm(depth, form, V=5, seed=7):
    """States 0 .. depth, state d backing off to d - 1, start = depth; bow, logp and eos random and not integer, so that the order
    of the adds shows in float32.  'uniform': arcs only in state 0, all leading to the deepest state -- every walk takes `depth`
    steps.  'mixed': every word in state 0 (next: the deepest state), and word w >= 1 also in state 8 w (next: depth - w) --
    walks of several lengths."""
    from torch_asg_amd import WordLM
    rng = np.random.default_rng(seed)
    H = depth + 1
    arcs = [(0, w, depth) for w in range(V)]
    if form == "mixed":
        arcs += [(8 * w, w, depth - w) for w in range(1, V) if 8 * w <= depth]
    arcs.sort()
    state = np.array([a[0] for a in arcs])
    row = np.concatenate([[0], np.cumsum(np.bincount(state, minlength=H))])
    backoff = np.arange(-1, depth)
    bow = -rng.uniform(0.01, 0.06, H)
    bow[0] = 0.0
    return WordLM(V, row, [a[1] for a in arcs], -rng.uniform(0.1, 2.0, len(arcs)), [a[2] for a in arcs], backoff, bow, depth,
                  -rng.uniform(0.1, 2.0, H))


def chain_inputs(dtype, seed=21):
    """[9][3][5] emissions and transitions for the small lexicon; utterance 0 spells "0 1 | 2 | 0": three words."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((9, 3, 5))
    for t, lab in enumerate([0, 1, 4, 2, 4, 0, 0, 1, 4]):
        x[t, 0, lab] += 4.0
    return x.astype(dtype), (0.5 * rng.standard_normal((5, 5))).astype(dtype), np.array([9, 6, 1])


# ---------------------------------------------------------------------------------------------------------------- case 3
@functools.lru_cache(maxsize=None)
def array_bigram(V, seed, keep=0.3):
    """Every unigram in state 0; state 1 + w is the history of word w, holds a random part of the bigrams and backs off to 0."""
    from torch_asg_amd import WordLM
    rng = np.random.default_rng(seed)
    has = rng.random((V, V)) < keep
    src, wd = np.nonzero(has)
    row = np.concatenate([[0, V], V + np.cumsum(np.bincount(src, minlength=V))])
    word = np.concatenate([np.arange(V), wd])
    backoff = np.zeros(V + 1, np.int64)
    backoff[0] = -1
    bow = np.concatenate([[0.0], -rng.uniform(0.05, 1.0, V)])
    return WordLM(V, row, word, -rng.uniform(0.1, 2.0, word.size), 1 + word, backoff, bow, 0, -rng.uniform(0.1, 2.0, V + 1))


# (elem, K, the last N with the transitions in LDS): the first N in global memory is the next one
LDS_STEPS = [(4, 8, 199), (8, 8, 141), (4, 8192, 123), (8, 8192, 59)]


@functools.lru_cache(maxsize=None)
def layout_case(N):
    """The three-word lexicon of the family's N = 141 | 142 tests (token 100 replaced below N = 101) and a small bigram."""
    from torch_asg_amd import Lexicon
    mid = 100 if N > 101 else 40
    return Lexicon([[3, 7], [3, mid, 5], [N - 2]], N, N - 1), array_bigram(3, 73, 0.5)


def layout_inputs(N, dtype, seed=37):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((6, 2, N))
    for t, lab in enumerate([3, 7, N - 1, N - 2, N - 1, 3]):
        x[t, 0, lab] += 6.0
    return x.astype(dtype), rng.standard_normal((N, N)).astype(dtype), np.array([6, 4])


# ---------------------------------------------------------------------------------------------------------------- case 4
LANE_BEAMS = (8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513)


@functools.lru_cache(maxsize=None)
def wide_case():
    """The 300-word lexicon of tests/test_hip_beam_word.py::wide_lexicon_and_lm (the same generator and seed) with a sparse
    bigram from arrays."""
    from torch_asg_amd import Lexicon
    rng = np.random.default_rng(5)
    words, seen = [], set()
    while len(words) < 300:
        n = int(rng.integers(1, 4))
        w = tuple(int(t) for t in rng.integers(0, 39, n))
        if w in seen or any(a == b for a, b in zip(w, w[1:])):
            continue
        seen.add(w)
        words.append(list(w))
    return Lexicon(words, 40, 39), array_bigram(300, 72, 0.03)


def wide_inputs(dtype=np.float32, seed=33):
    """Flat emissions: many pairs stay close, every frame fills the beam."""
    rng = np.random.default_rng(seed)
    return ((0.25 * rng.standard_normal((5, 2, 40))).astype(dtype), (0.25 * rng.standard_normal((40, 40))).astype(dtype),
            np.array([5, 4]))


# ---------------------------------------------------------------------------------------------------- the confidence calls
# (tests/test_beam_word_conf_regimes_cpu.py, tests/test_hip_beam_word_conf_regimes.py)
# the seeds of `width_inputs` at which a REPORTED confidence depends on a pair at or above 2^32 (the CPU module asserts it).  At 33
# bits WIDTH_SEEDS' own seed keeps such pairs in its sets, yet no reported value reads them: the confidence cases take another.
CONF_WIDTH_SEEDS = {33: 19, 35: 11}

# the largest lattice set of a confidence call, M = K: (160 KiB - 256) / (16 + e), as include/asg_hip.h states it
CONF_BOUND = {4: 8179, 8: 6816}
assert all(CONF_BOUND[e] == (160 * 1024 - 256) // (16 + e) for e in (4, 8))

CONF_RING = 256                    # kConfRing: the accumulators of the one-best sink
SINK_FIXED = 1024                  # kSinkFixed: the window offsets and the word filter of the n-best sink


def subgroup(m):
    """The lattice pass's lanes per member of a source set of m: the largest power of two <= 64 with G m <= 1024 (kBL)."""
    G = 1
    while G < 64 and G * 2 * m <= 1024:
        G *= 2
    return G


def bwd_front(elem, key, M):
    """The dynamic LDS in front of a sink's own: the pairs (key bytes each) and their beta of one lattice set, padded to 16."""
    return (M * (elem + key) + 15) & ~15


def conf_pull_lds(elem, M):
    """The dynamic LDS of beam_word_conf_bwd: the front and the ring of u64 accumulators."""
    return bwd_front(elem, 8, M) + CONF_RING * 8


def nbest_conf_ring(K, nbest, tol):
    """The ring of the row sink: the power of two >= min(nbest, K) (2 tol + 2)."""
    r = 1
    while r < min(nbest, K) * (2 * tol + 2):
        r *= 2
    return r


def nbest_conf_pull_lds(elem, K, nbest, tol):
    """The dynamic LDS of nbest_conf_bwd: the front, the sink's fixed part, a u64 and an int32 per ring slot."""
    return bwd_front(elem, 8, K) + SINK_FIXED + 12 * nbest_conf_ring(K, nbest, tol)


def wide_pairs(sets, qbits):
    """How many pairs of an utterance's sets are h << qbits | q >= 2^32."""
    return sum(pair_int(p, qbits) >= 1 << 32 for u in sets for p in u)


def without_wide_pairs(sets, qbits):
    """An utterance's sets with every pair h << qbits | q >= 2^32 removed: the lattice of a kernel that loses them."""
    return [[p for p in u if pair_int(p, qbits) < 1 << 32] for u in sets]


def confidences_on_sets(m, x, tr, L, sets, path, words, n_words, tol, events=None):
    """One hypothesis of one utterance over a GIVEN lattice: m the word model, x [T,N] and tr [N,N] float64, `sets` the L
    lattice sets, `path` / `words` / `n_words` what the decoder returned -> (Z, the confidences of its n_words words), by
    tests/beam_word_conf_ref.py's `word_events` and `hypothesis_frames` and the window sum of the specification.  `events`:
    that `word_events(m, x, tr, L, sets)` where the caller has it already (several rows over one lattice)."""
    from beam_word_conf_ref import hypothesis_frames, word_events
    Z, P = word_events(m, x, tr, L, sets) if events is None else events
    frames = hypothesis_frames(path, n_words, L, m.sep) if n_words else []
    return Z, [sum(P.get((int(words[k]), t), 0.0) for t in range(max(1, tk - tol), min(L, tk + tol) + 1))
               for k, tk in enumerate(frames)]
