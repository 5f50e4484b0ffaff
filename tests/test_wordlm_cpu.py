"""CPU tests of the host objects of word-LM decoding (torch_asg_amd/wordlm.py): an ARPA trigram read into a backoff automaton
and compared with a table built by hand, the walk through two backoff steps, the end of the sentence, n-grams with words outside
the vocabulary, the null LM, the folding, and the lexicon's word of each trie node."""
import numpy as np
import pytest

from torch_asg_amd import Lexicon, TokenGraph, WordLM

L10 = float(np.log(np.float64(10.0)))

ARPA = """
\\data\\
ngram 1=9
ngram 2=7
ngram 3=4

\\1-grams:
-99 <s> -0.5
-1.0 </s>
-0.7 a -0.3
-0.8 b -0.2
-0.9 c -0.4
-1.1 d
-1.2 e -0.1
-1.3 f
-1.4 zzz -0.6

\\2-grams:
-0.2 <s> a -0.25
-0.3 a b -0.15
-0.4 b c -0.35
-0.5 b </s>
-0.6 c a
-0.65 a zzz -0.1
-0.45 e b -0.05

\\3-grams:
-0.11 <s> a b
-0.12 a b c
-0.13 a b </s>
-0.14 zzz a b

\\end\\
"""
VOCAB = ["a", "b", "c", "d", "e", "f"]
# the table by hand.  States: 0 (), 1 (<s>), 2..7 (a)..(f), 8 (<s> a), 9 (a b), 10 (b c), 11 (c a), 12 (e b)
ROW = [0, 6, 7, 8, 9, 10, 10, 11, 11, 12, 13, 13, 13, 13]
WORD = [0, 1, 2, 3, 4, 5, 0, 1, 2, 0, 1, 1, 2]
LOGP = [-0.7, -0.8, -0.9, -1.1, -1.2, -1.3, -0.2, -0.3, -0.4, -0.6, -0.45, -0.11, -0.12]
NEXT = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 9, 10]
BACKOFF = [-1, 0, 0, 0, 0, 0, 0, 0, 2, 3, 4, 2, 3]
BOW = [0.0, -0.5, -0.3, -0.2, -0.4, 0.0, -0.1, 0.0, -0.25, -0.15, -0.35, 0.0, -0.05]


def s(x):
    return x * L10


def _eos_by_hand():
    e = [s(-1.0), 0.0 + s(-0.5) + s(-1.0), 0.0 + s(-0.3) + s(-1.0), s(-0.5), 0.0 + s(-0.4) + s(-1.0), 0.0 + 0.0 + s(-1.0),
         0.0 + s(-0.1) + s(-1.0), 0.0 + 0.0 + s(-1.0), ((0.0 + s(-0.25)) + s(-0.3)) + s(-1.0), s(-0.13),
         ((0.0 + s(-0.35)) + s(-0.4)) + s(-1.0), ((0.0 + 0.0) + s(-0.3)) + s(-1.0), (0.0 + s(-0.05)) + s(-0.5)]
    return np.array(e)


def test_arpa_trigram_against_the_table_by_hand():
    lm = WordLM.from_arpa(ARPA, VOCAB)
    assert (lm.V, lm.H, lm.A, lm.start) == (6, 13, 13, 1)
    assert lm.row.tolist() == ROW and lm.word.tolist() == WORD and lm.next.tolist() == NEXT
    assert lm.backoff.tolist() == BACKOFF
    assert np.array_equal(lm.logp, np.array([s(x) for x in LOGP]))
    assert np.array_equal(lm.bow, np.array([s(x) for x in BOW]))
    assert np.array_equal(lm.eos, _eos_by_hand())


def test_out_of_vocabulary_ngrams_are_dropped_and_a_missing_unigram_raises():
    lm = WordLM.from_arpa(ARPA, VOCAB)
    # "zzz", "a zzz" and "zzz a b" left nothing behind: no state, no arc
    assert lm.H == 13 and lm.A == 13
    more = WordLM.from_arpa(ARPA, VOCAB + ["zzz"])
    assert more.V == 7 and more.H > 13 and more.A == 16
    with pytest.raises(ValueError, match="unigram"):
        WordLM.from_arpa(ARPA, VOCAB + ["g"])
    with pytest.raises(ValueError, match="repeats"):
        WordLM.from_arpa(ARPA, ["a", "a"] + VOCAB[1:])


def test_the_walk_backs_off_twice_and_adds_in_walk_order():
    lm = WordLM.from_arpa(ARPA, VOCAB)
    assert lm.step(8, 1) == (9, 0.0 + s(-0.11))                               # <s> a b: explicit
    assert lm.step(8, 2) == (4, ((0.0 + s(-0.25)) + s(-0.3)) + s(-0.9))       # (<s> a) -> (a) -> (): c
    assert lm.step(9, 0) == (2, ((0.0 + s(-0.15)) + s(-0.2)) + s(-0.7))       # (a b) -> (b) -> (): a
    assert lm.step(10, 0) == (11, (0.0 + s(-0.35)) + s(-0.6))                 # (b c) -> (c): a, one step
    assert lm.step(9, 2) == (10, 0.0 + s(-0.12))                              # a b c: next is the suffix (b c)
    assert lm.step(0, 3) == (5, 0.0 + s(-1.1))
    assert lm.step(1, 5) == (7, (0.0 + s(-0.5)) + s(-1.3))


def test_arpa_from_a_file_and_orders(tmp_path):
    p = tmp_path / "lm.arpa"
    p.write_text(ARPA)
    a, b = WordLM.from_arpa(str(p), VOCAB), WordLM.from_arpa(ARPA, VOCAB)
    for n in ("row", "word", "logp", "next", "backoff", "bow", "eos"):
        assert np.array_equal(getattr(a, n), getattr(b, n))
    uni = WordLM.from_arpa("\\data\\\nngram 1=3\n\n\\1-grams:\n-1 a\n-2 b\n-0.5 </s>\n\\end\\\n", ["a", "b"])
    assert (uni.H, uni.A, uni.start) == (1, 2, 0) and uni.next.tolist() == [0, 0] and uni.eos.tolist() == [s(-0.5)]
    with pytest.raises(ValueError, match="orders"):
        WordLM.from_arpa("\\data\\\nngram 5=1\n\n\\5-grams:\n-1 a a a a a\n\\end\\\n", ["a"])


def test_null_lm_and_rejection():
    lm = WordLM.null(4)
    assert (lm.H, lm.A, lm.V, lm.start) == (1, 4, 4, 0) and lm.backoff.tolist() == [-1] and lm.eos.tolist() == [0.0]
    assert all(lm.step(0, w) == (0, 0.0) for w in range(4))
    # a word the empty history does not know is rejected, from every state whose chain reaches it
    part = WordLM(3, [0, 2, 3], [0, 2, 1], [-1.0, -2.0, -0.5], [1, 1, 0], [-1, 0], [0.0, -0.25], 0, [-1.0, -np.inf])
    assert part.step(0, 1) is None and part.step(1, 1) == (0, -0.5) and part.step(1, 2) == (1, -0.25 + -2.0)
    assert part.step(1, 0) == (1, -0.25 + -1.0)


def test_constructor_validates():
    ok = dict(num_words=2, row=[0, 2], word=[0, 1], logp=[0.0, 0.0], next=[0, 0], backoff=[-1], bow=[0.0], start=0, eos=[0.0])
    WordLM(**ok)
    for bad in (dict(word=[1, 0]), dict(word=[0, 2]), dict(next=[0, 1]), dict(backoff=[0]), dict(start=1), dict(row=[0, 1]),
                dict(logp=[0.0, np.nan]), dict(eos=[np.inf])):
        with pytest.raises(ValueError):
            WordLM(**dict(ok, **bad))
    with pytest.raises(ValueError, match="backoff"):      # a cycle that never reaches the empty history
        WordLM(2, [0, 2, 2, 2], [0, 1], [0.0, 0.0], [0, 0], [-1, 2, 1], [0.0, 0.0, 0.0], 0, [0.0, 0.0, 0.0])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_folding_rounds_twice_in_the_decode_dtype_and_keeps_minus_infinity(dt):
    lm = WordLM.from_arpa(ARPA, VOCAB)
    lm = WordLM(lm.V, lm.row, lm.word, np.where(np.arange(lm.A) == 3, -np.inf, lm.logp), lm.next, lm.backoff, lm.bow, lm.start,
                np.where(np.arange(lm.H) == 5, -np.inf, lm.eos))
    for m, ws in ((1.0, 0.0), (0.7, -1.3), (0.0, 0.25)):
        h = lm.compile_host(dt, m, ws)
        want = (dt(m) * lm.logp.astype(dt)).astype(dt) + dt(ws) if m else np.full(lm.A, dt(ws))
        want = np.where(lm.logp == -np.inf, dt(-np.inf), want).astype(dt)
        assert h["lw"].dtype == dt and np.array_equal(h["lw"], want)
        assert np.array_equal(h["bw"], (dt(m) * lm.bow.astype(dt)).astype(dt))
        ew = np.where(lm.eos == -np.inf, dt(-np.inf), (dt(m) * np.where(lm.eos == -np.inf, 0, lm.eos).astype(dt))).astype(dt)
        assert np.array_equal(h["ew"], ew) and h["ew"][5] == -np.inf and h["lw"][3] == -np.inf
    with pytest.raises(ValueError):
        lm.compile_host(dt, np.inf, 0.0)


def test_lexicon_is_from_lexicon_plus_the_word_of_each_node():
    words = [[0], [0, 1], [1, 0], [2], [0, 1, 2]]
    sc = [0.5, -1.0, 0.0, 2.0, -0.25]
    lex = Lexicon(words, 5, 4, sc)
    g = TokenGraph.from_lexicon(words, 5, 4, sc)
    for n in ("next", "weight", "final"):
        assert np.array_equal(getattr(lex.graph, n), getattr(g, n))
    assert lex.graph.start == g.start == 0
    # nodes in order of first creation: 0 root, 1 [0], 2 [0,1], 3 [1], 4 [1,0], 5 [2], 6 [0,1,2]
    assert lex.word_of_state.dtype == np.int64 and lex.word_of_state.tolist() == [-1, 0, 1, -1, 2, 3, 4]
    assert Lexicon(words, 5, 4, None, [7, 5, 3, 1, 9]).word_of_state.tolist() == [-1, 7, 5, -1, 3, 1, 9]
    with pytest.raises(ValueError, match="share the spelling"):
        Lexicon(words + [[1, 0]], 5, 4)
    with pytest.raises(ValueError):
        Lexicon(words, 5, 4, None, [0, 1, 2])
