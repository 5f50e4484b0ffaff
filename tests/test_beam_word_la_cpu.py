"""CPU tests of LM look-ahead in the lexicon + word-LM beam decoder (`torch_asg_amd.WordLookahead`,
`beam_decode_words(..., lookahead=)`, include/asg_hip.h::asg_beam_decode_words_la): the host tables against the definition by
plain loops; the numpy restatement (tests/beam_word_la_ref.py) against the restatement without look-ahead where the two must
agree -- unpruned, and pruned for order 1 through a host fold of the look-ahead into the lexicon's weights; the case the feature
is for; the C entry point's argument checks.  No kernel is launched here."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, eighths, small_lexicon, without_unigrams
from beam_word_la_ref import Look, beam_word_la_ref, truncated_state, words_below
from beam_word_ref import beam_word_ref, fold_lm
from test_beam_word_stream_abi import LM_ARRAYS, _graph, _lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAMES = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths")
ALL = 1024

HAND_ARPA = """\\data\\
ngram 1=8
ngram 2=7
ngram 3=4

\\1-grams:
-99 <s> -0.5
-1.0 a -0.25
-1.5 ab -0.5
-0.75 b -0.125
-2.0 c
-1.25 d
-0.5 x -0.25
-1.0 </s>

\\2-grams:
-0.5 <s> a -0.25
-0.25 a b -0.5
-0.75 a x
-1.0 b ab -0.125
-0.5 b </s>
-0.375 x c
-0.625 ab a

\\3-grams:
-0.125 <s> a b
-0.25 a b ab
-0.5 b ab a
-0.75 a b </s>

\\end\\
"""
HAND_VOCAB = ["a", "ab", "b", "c", "d", "x"]


def hand_case():
    """A trigram with missing pairs and histories that back off twice; the prefix pair "a" / "ab"; word d = [3, 0] has no arc in
    the LM (its unigram is taken out), so the nodes [3] and [3, 0] have nothing below them that the LM knows; the LM word x is
    not in the lexicon."""
    from torch_asg_amd import Lexicon, WordLM
    lex = Lexicon([[0], [0, 1], [1], [2], [3, 0]], 5, 4)
    lm = without_unigrams(WordLM.from_arpa(HAND_ARPA, HAND_VOCAB), {4})
    return lex, lm


def table_LA(la, tab, bw, backoff, s, n):
    """LA(s, n) of the header with E from the package's table."""
    dt = tab.dtype.type
    r, a = dt(-np.inf), dt(0)
    while True:
        x = dt(a + la.range_max(tab, s, n))
        if x > r:
            r = x
        if backoff[s] < 0:
            return r
        a, s = dt(a + bw[s]), int(backoff[s])


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def check_tables(lex, lm, order, dt, lm_weight=0.7, word_score=-0.4):
    from torch_asg_amd import WordLookahead
    la = WordLookahead(lex, lm, order)
    lw, bw, _ = fold_lm(lm, dt, lm_weight, word_score)
    look = Look(lex, lm, order, np.dtype(dt).type, lw, bw)
    below = words_below(lex)
    S, H = lex.graph.S, lm.H
    assert la.rlo.dtype == np.int32 and la.rhi.dtype == np.int32 and la.la_state.dtype == np.int32
    assert la.rlo.shape == (S,) and la.rhi.shape == (S,) and la.la_state.shape == (H,) and la.krow.shape == (H + 1,)
    for n in range(S):                                     # the ranks of a node are the words below it
        assert {w for w in range(lm.V) if la.rlo[n] <= la.word_rank[w] < la.rhi[n] and la.word_rank[w] >= 0} == below[n]
        if lex.word_of_state[n] >= 0:                      # a node's own word comes before its descendants'
            assert la.word_rank[lex.word_of_state[n]] == la.rlo[n]
    assert la.la_state.tolist() == truncated_state(lm, order)
    for s in range(H):
        kr = la.krank[la.krow[s]:la.krow[s + 1]]
        assert (np.diff(kr) > 0).all()
        assert sorted(kr.tolist()) == sorted(int(la.word_rank[w]) for w in lm.word[lm.row[s]:lm.row[s + 1]] if la.word_rank[w] >= 0)
    tab = la.compile_host(dt, lm_weight, word_score)
    assert tab.dtype == np.dtype(dt) and tab.shape == (la.levels, la.A)
    assert same_bits(la.dense_host(tab), np.array([look.E(0, n) for n in range(S)], dt))
    for s in range(H):
        for n in range(S):
            assert same_bits(la.range_max(tab, s, n), look.E(s, n)), (s, n)
            assert same_bits(table_LA(la, tab, bw, lm.backoff, s, n), look.LA(s, n)), (s, n)
    return la, look, tab


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_tables_equal_the_definition_on_a_hand_built_trigram(order, dt):
    lex, lm = hand_case()
    depth = lambda h: 0 if lm.backoff[h] < 0 else 1 + depth(int(lm.backoff[h]))     # noqa: E731
    assert max(depth(h) for h in range(lm.H)) == 2                                  # a backoff of depth 2
    assert lm.find(lm.start, 2) < 0 and lm.find(lm.start, 0) >= 0                   # missing pairs
    la, look, tab = check_tables(lex, lm, order, dt)
    assert la.word_rank[5] == -1 and la.word_rank[4] >= 0                           # x has no rank; d has one and no arcs
    assert la.A == lm.A - sum(1 for w in lm.word if w == 5)
    dead = [n for n in range(lex.graph.S) if not (words_below(lex)[n] - {4})]       # the nodes [3] and [3, 0]
    assert len(dead) == 2
    for n in dead:
        for h in range(lm.H):
            assert look.L(h, n) == -np.inf and la.range_max(tab, int(la.la_state[h]), n) == -np.inf
    if order == 1:
        assert set(la.la_state.tolist()) == {0}
    if order >= 3:                                         # full look-ahead: an upper bound of every word's own LM score
        assert la.la_state.tolist() == list(range(lm.H))
        lw, bw, _ = fold_lm(lm, dt, 0.7, -0.4)
        for h in range(lm.H):
            for n in range(1, lex.graph.S):
                for w in words_below(lex)[n]:
                    a, s = dt(0), h
                    while lm.find(s, w) < 0 and lm.backoff[s] >= 0:
                        a, s = dt(a + bw[s]), int(lm.backoff[s])
                    if lm.find(s, w) >= 0:
                        assert look.L(h, n) >= dt(a + lw[lm.find(s, w)])


def test_a_long_row_needs_every_level_and_short_ranges_read_one_entry_twice():
    from torch_asg_amd import Lexicon, WordLM
    words = [[0, 1 + i] for i in range(70)] + [[1], [1, 2], [1, 3], [2], [2, 3], [3]] + [[4, 5 + i] for i in range(5)]
    V = len(words)
    lex = Lexicon(words, 80, 79)
    rng = np.random.default_rng(11)
    sub = np.sort(rng.choice(V, 75, replace=False))        # state 1: 75 of the 81 words, backing off to state 0
    lm = WordLM(V, [0, V, V + 75], np.concatenate([np.arange(V), sub]), -rng.uniform(0.1, 5.0, V + 75), np.zeros(V + 75, np.int64),
                [-1, 0], [0.0, -0.3], 1, [-1.0, -2.0])
    for dt in (np.float32, np.float64):
        la, _, _ = check_tables(lex, lm, 2, dt)
        assert np.diff(la.krow).max() > 64 and la.levels == 7
        assert {1, 2, 3, 5, 70} <= set((la.rhi - la.rlo).tolist())


def test_constructor_errors():
    from torch_asg_amd import Lexicon, WordLM, WordLookahead
    lex, lm = hand_case()
    for order in (0, -1):
        with pytest.raises(ValueError, match="order"):
            WordLookahead(lex, lm, order)
    # word 1 has an arc after word 0 and none in the empty history
    lex2 = Lexicon([[0], [1]], 3, 2)
    bad = WordLM(2, [0, 1, 2], [0, 1], [-1.0, -0.5], [1, 0], [-1, 0], [0.0, -0.25], 0, [-1.0, -1.0])
    with pytest.raises(ValueError, match="no backoff"):
        WordLookahead(lex2, bad, 2)
    with pytest.raises(TypeError):
        WordLookahead(lex2.graph, bad, 2)
    with pytest.raises(RuntimeError, match="knows"):
        WordLookahead(lex, WordLM.null(2), 2)              # check_words' own check
    import torch_asg_amd as A
    assert "WordLookahead" in A.__all__


def _emissions(T, B, N, seed, dt):
    rng = np.random.default_rng(seed)
    return (rng.integers(-32, 32, (T, B, N)) / 8.0).astype(dt), (rng.integers(-16, 16, (N, N)) / 8.0).astype(dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_unpruned_the_look_ahead_cancels_bit_for_bit(order, dt):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = eighths(arpa_lm(5, 3, 43))
    x, tr = _emissions(8, 4, 5, 35, dt)
    il = np.array([8, 5, 1, 0])
    want = beam_word_ref(x, tr, lex, lm, il, ALL, INF, 1.0, 0.25, 0.125)
    info = {}
    got = beam_word_la_ref(x, tr, lex, lm, order, il, ALL, INF, 1.0, 0.25, 0.125, info=info)
    assert max(max(s) for s in info["sizes"] if s) < ALL
    assert (want["scores"][:3] > -np.inf).all()
    for n in NAMES:
        assert same_bits(got[n], want[n]), n


def folded_lexicon(lex, look):
    """The lexicon with an order-1 look-ahead L(n) folded into its weights: L(child) - L(parent) into the trie arcs (L into
    those out of the root), -L(node) into separator arcs and finals."""
    g = lex.graph
    nxt = np.asarray(g.next, np.int64)
    weight, final = np.array(g.weight, np.float64), np.array(g.final, np.float64)
    sep = lex.separator
    Ln = [float(look.L(0, n)) for n in range(g.S)]
    for s in range(g.S):
        for i in range(nxt.shape[1]):
            if nxt[s, i] < 0:
                continue
            weight[s, i] += -Ln[s] if i == sep else Ln[nxt[s, i]] - Ln[s]
        if s and final[s] > -np.inf:
            final[s] -= Ln[s]
    return types.SimpleNamespace(graph=types.SimpleNamespace(next=nxt, weight=weight, final=final, S=g.S, N=g.N),
                                 word_of_state=lex.word_of_state, separator=sep)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_order_one_equals_a_host_fold_into_the_lexicon_pruned(dt):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = eighths(arpa_lm(5, 3, 44, keep=(1.0, 0.5, 0.5)))
    WS, TS = 0.25, 0.125
    lw, bw, _ = fold_lm(lm, np.float64, 1.0, WS)
    look = Look(lex, lm, 1, np.float64, lw, bw)
    assert all(look.L(0, n) > -np.inf for n in range(lex.graph.S))                 # no dead end: the fold keeps every arc
    assert len({look.L(0, n) for n in range(lex.graph.S)}) > 2
    folded = folded_lexicon(lex, look)
    x, tr = _emissions(7, 4, 5, 36, dt)
    il = np.array([7, 4, 1, 0])
    pruned = 0
    for K in (1, 2, 3, 8, 64, ALL):
        for theta in (INF, 2.0, 0.0):
            wi, gi = {}, {}
            want = beam_word_ref(x, tr, folded, lm, il, K, theta, 1.0, WS, TS, info=wi)
            got = beam_word_la_ref(x, tr, lex, lm, 1, il, K, theta, 1.0, WS, TS, info=gi)
            for n in NAMES:
                assert same_bits(got[n], want[n]), (n, K, theta)
            assert gi["kept"] == wi["kept"] and gi["sizes"] == wi["sizes"], (K, theta)
            plain = {}
            beam_word_ref(x, tr, lex, lm, il, K, theta, 1.0, WS, TS, info=plain)
            pruned += plain["kept"] != gi["kept"]
    assert pruned > 0                                      # the look-ahead changed what a narrow beam keeps


def rescue_case(dt):
    """Two words share their first letter; the second letter's acoustics slightly prefer the word the LM dislikes."""
    from torch_asg_amd import Lexicon, WordLM
    lex = Lexicon([[0, 1], [0, 2]], 4, 3)
    lm = WordLM(2, [0, 2], [0, 1], [-5.0, -1.0], [0, 0], [-1], [0.0], 0, [0.0])
    x = np.full((3, 1, 4), -9.0, dt)
    x[0, 0, 0] = 0.0
    x[1, 0, 1], x[1, 0, 2] = 0.0, -0.5
    x[2, 0, 3] = 0.0
    return lex, lm, x, np.zeros((4, 4), dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_look_ahead_rescues_the_word_a_beam_of_one_prunes(dt):
    lex, lm, x, tr = rescue_case(dt)
    best = beam_word_ref(x, tr, lex, lm, None, ALL)
    assert best["words"][0, 0] == 1
    plain = beam_word_ref(x, tr, lex, lm, None, 1)
    assert plain["words"][0, 0] == 0 and plain["scores"][0] < best["scores"][0]     # K = 1 without look-ahead: the poor word
    for order in (1, 2):
        got = beam_word_la_ref(x, tr, lex, lm, order, None, 1)
        for n in NAMES:
            assert same_bits(got[n], best[n]), n


# ---------------------------------------------------------------------------------------------------------------- the C ABI
LA_ARRAYS = ("rlo", "rhi", "la_state", "krow", "krank", "tab", "dense0")


def _la(_lib, S=60000, H=20001, A=300000, levels=15, dtype=None):
    s = _lib.AsgWordLookahead()
    s.S, s.H, s.A, s.levels = S, H, A, levels
    s.dtype = _lib.ASG_DTYPE_F32 if dtype is None else dtype
    for n in LA_ARRAYS:
        setattr(s, n, 256)                                 # never dereferenced here
    return s


def test_entry_point_is_declared_exported_and_bound():
    from torch_asg_amd import _lib
    src = open(os.path.join(ROOT, "include", "asg_hip.h")).read()
    L = _lib.lib()
    n = "asg_beam_decode_words_la"
    assert re.search(r"\b%s\s*\(" % n, src) and hasattr(L, n) and n in _lib.SYMBOLS
    assert "asg_word_lookahead" in src
    assert int(L.asg_hip_version()) == 230 and "#define ASG_HIP_VERSION 230" in src       # an addition


def test_abi_argument_checks_without_a_device():
    from torch_asg_amd import _lib
    L = _lib.lib()
    F32, F64 = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_F64
    g, gb = _graph(_lib)
    w = _lm(_lib)
    la = _la(_lib)
    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.dtype = 8, 2, 40, F32
    p.inputs = p.transition = 256
    wb = int(L.asg_beam_decode_words_work_bytes(ctypes.byref(p), ctypes.byref(gb), ctypes.byref(w), 8))
    assert wb > 0
    big = 1 << 50
    outs = (256,) * 8
    ref = lambda x: None if x is None else ctypes.byref(x)                          # noqa: E731
    call = lambda K=8, th=1.0, work=256, n=big, o=outs, lm=w, pp=p, gg=gb, ll=la: L.asg_beam_decode_words_la(      # noqa: E731
        None, ref(pp), ref(gg), ref(lm), ref(ll), K, th, work, n, *o, 0, None)
    plain = lambda n: L.asg_beam_decode_words(None, ref(p), ref(gb), ref(w), 8, 1.0, 256, n, *outs, 0, None)       # noqa: E731
    # one workspace function serves both entry points: both refuse one byte less
    assert call(n=wb - 1) == 3 and plain(wb - 1) == 3 and call(n=16) == 3
    # the checks of asg_beam_decode_words
    assert call(K=0) == 1 and call(K=8193) == 2 and call(th=-1.0) == 1 and call(th=float("nan")) == 1 and call(work=None) == 1
    assert call(pp=None) == 1 and call(gg=None) == 1 and call(lm=None) == 1
    assert call(lm=_lm(_lib, H=(1 << 25) + 1), ll=_la(_lib, H=(1 << 25) + 1)) == 2
    for name in LM_ARRAYS:
        m = _lm(_lib)
        setattr(m, name, None)
        assert call(lm=m) == 1, name
    for i in range(8):
        assert call(o=outs[:i] + (None,) + outs[i + 1:]) == 1, i
    # the look-ahead's own
    assert call(ll=None) == 1
    for name in LA_ARRAYS:
        m = _la(_lib)
        setattr(m, name, None)
        assert call(ll=m, n=16) == 1, name
    for kw in (dict(S=59999), dict(H=20000), dict(dtype=F64), dict(A=-1), dict(A=400001), dict(levels=0), dict(levels=32),
               dict(A=100, levels=8)):
        assert call(ll=_la(_lib, **kw), n=16) == 1, kw
    assert call(ll=_la(_lib, A=128, levels=8), n=16) == 3                           # 2^7 arcs fill level 7: on to the workspace
    empty = _la(_lib, A=0, levels=1)
    empty.krank = empty.tab = None
    assert call(ll=empty, n=16) == 3                                                # no ranked arc: nothing to point at
    p.dtype = F64
    assert call() == 1
    p.dtype = F32


def test_python_surface_refuses_a_wrong_look_ahead_before_any_launch():
    import torch_asg_amd as A
    lex, lm = hand_case()
    la = A.WordLookahead(lex, lm, 2)
    x, tr = torch.zeros(5, 2, 5), torch.zeros(5, 5)
    with pytest.raises(TypeError, match="lookahead"):
        A.beam_decode_words(x, tr, lex, lm, beam_size=4, lookahead=lm)
    other = A.Lexicon([[0], [1]], 5, 4)
    with pytest.raises(RuntimeError, match="built for"):
        A.beam_decode_words(x, tr, other, lm, beam_size=4, lookahead=la)
    with pytest.raises(RuntimeError, match="built for"):
        A.ASGLoss(5).beam_decode_words(x, lex, A.WordLM.null(6), beam_size=4, lookahead=la)
    same_shape = A.Lexicon([[0], [0, 1], [1], [2], [3, 0]], 5, 4)                   # equal S, another object: its ranks could differ
    with pytest.raises(RuntimeError, match="built for"):
        A.beam_decode_words(x, tr, same_shape, lm, beam_size=4, lookahead=la)
    with pytest.raises(RuntimeError, match="built for"):
        A.beam_decode_words(x, tr, lex, hand_case()[1], beam_size=4, lookahead=la)  # an equal LM, another object
    with pytest.raises(RuntimeError):
        A.beam_decode_words(x, tr, lex, lm, beam_size=4, lookahead=la)              # CPU tensors: there is no CPU implementation
