"""Inputs shared by the CPU and GPU tests of beam decoding with a lexicon and a word LM (tests/test_beam_word_cpu.py,
tests/test_hip_beam_word.py): the small lexicon, random ARPA texts, the static composition of a lexicon with a word LM as one
token automaton, and an independent scorer of one label path."""
import itertools

import numpy as np

from beam_word_ref import fold_lm
from graph_decode_ref import fold

SMALL_WORDS = [[0], [0, 1], [1, 0], [2], [0, 1, 2]]      # N = 5: tokens 0..3, separator 4


def small_lexicon(word_scores=None):
    from torch_asg_amd import Lexicon
    return Lexicon(SMALL_WORDS, 5, 4, word_scores)


def random_arpa(V, order, seed, keep=(1.0, 0.5, 0.4), bow_prob=0.8):
    """ARPA text over the words w0 .. w{V-1}: every unigram, a random part of the higher n-grams whose prefix is there."""
    rng = np.random.default_rng(seed)
    names = ["w%d" % i for i in range(V)]
    levels = [[("<s>",)] + [(n,) for n in names] + [("</s>",)]]
    for k in range(2, order + 1):
        cur = []
        for g in levels[-1]:
            if g[-1] == "</s>":
                continue
            for w in names + ["</s>"]:
                if rng.random() < keep[k - 1]:
                    cur.append(g + (w,))
        levels.append(cur)
    lines = ["\\data\\"] + ["ngram %d=%d" % (k + 1, len(lv)) for k, lv in enumerate(levels)] + [""]
    for k, lv in enumerate(levels):
        lines.append("\\%d-grams:" % (k + 1))
        for g in lv:
            lp = -99.0 if g == ("<s>",) else -float(rng.uniform(0.1, 2.0))
            s = "%.4f %s" % (lp, " ".join(g))
            if k + 1 < order and g[-1] != "</s>" and rng.random() < bow_prob:
                s += " %.4f" % -float(rng.uniform(0.05, 1.0))
            lines.append(s)
        lines.append("")
    lines.append("\\end\\")
    return "\n".join(lines), names


def arpa_lm(V, order, seed, **kw):
    from torch_asg_amd import WordLM
    text, names = random_arpa(V, order, seed, **kw)
    return WordLM.from_arpa(text, names)


def with_weights(lm, fn):
    """The same automaton with every finite weight passed through fn."""
    from torch_asg_amd import WordLM
    f = lambda a: np.where(np.isfinite(a), fn(np.where(np.isfinite(a), a, 0.0)), a)      # noqa: E731
    return WordLM(lm.V, lm.row, lm.word, f(lm.logp), lm.next, lm.backoff, f(lm.bow), lm.start, f(lm.eos))


def eighths(lm):
    return with_weights(lm, lambda a: np.round(a * 8.0) / 8.0)


def integers(lm):
    return with_weights(lm, np.round)


def without_unigrams(lm, words):
    """The same automaton without the arcs of the empty history on `words`: a step that reaches state 0 on them is rejected."""
    from torch_asg_amd import WordLM
    keep = np.ones(lm.A, bool)
    for k in range(int(lm.row[0]), int(lm.row[1])):
        if lm.word[k] in words:
            keep[k] = False
    rid = np.repeat(np.arange(lm.H), np.diff(lm.row))[keep]
    row = np.zeros(lm.H + 1, np.int64)
    np.cumsum(np.bincount(rid, minlength=lm.H), out=row[1:])
    return WordLM(lm.V, row, lm.word[keep], lm.logp[keep], lm.next[keep], lm.backoff, lm.bow, lm.start, lm.eos)


def compose_static(lexicon, lm):
    """The lexicon composed with the LM (lm_weight 1, word_score 0) as ONE token automaton: state h * S + node, so that its
    product states in their own order are the pairs (h, q) in pair order.  -> (next, weight, final, start).  Exact only when
    every weight is such that sums do not round (the callers use multiples of 1/8)."""
    g = lexicon.graph
    S, N, sep = g.S, g.N, lexicon.separator
    H = lm.H
    nxt = np.full((H * S, N), -1, np.int64)
    wt = np.full((H * S, N), -np.inf)
    fin = np.full(H * S, -np.inf)
    for h in range(H):
        for s in range(S):
            for i in range(N):
                if g.next[s, i] < 0 or g.weight[s, i] == -np.inf:
                    continue
                if i != sep:
                    nxt[h * S + s, i], wt[h * S + s, i] = h * S + g.next[s, i], g.weight[s, i]
                else:
                    st = lm.step(h, int(lexicon.word_of_state[s]))
                    if st is not None and st[1] > -np.inf:
                        nxt[h * S + s, i], wt[h * S + s, i] = st[0] * S + g.next[s, i], g.weight[s, i] + st[1]
            if s == 0:
                fin[h * S] = g.final[0] + lm.eos[h]
            elif lexicon.word_of_state[s] >= 0:
                st = lm.step(h, int(lexicon.word_of_state[s]))
                if st is not None:
                    fin[h * S + s] = g.final[s] + (st[1] + lm.eos[st[0]])
    return nxt, wt, fin, lm.start * S


def path_score_words(xb, tr, lexicon, lm, labels, lm_weight=1.0, word_score=0.0, token_score=0.0):
    """Score of one label sequence under the specification's adds, -inf if the lexicon or the LM rejects it; written apart
    from the search (tests/beam_word_ref.py)."""
    dt = xb.dtype.type
    g = lexicon.graph
    sep, wos = lexicon.separator, lexicon.word_of_state
    present, arcw, finw = fold(g.next, g.weight, g.final, dt, 1.0, token_score)
    lw, bw, ew = fold_lm(lm, dt, lm_weight, word_score)
    ninf = dt(-np.inf)

    def step(h, w):
        a = dt(0)
        while True:
            k = lm.find(h, w)
            if k >= 0:
                return int(lm.next[k]), dt(a + lw[k])
            if lm.backoff[h] < 0:
                return None
            a, h = dt(a + bw[h]), int(lm.backoff[h])
    l0 = int(labels[0])
    if not present[0, l0]:
        return ninf
    s, h = int(g.next[0, l0]), lm.start
    v = dt(arcw[0, l0] + xb[0, l0])
    for t in range(1, len(labels)):
        i, j = int(labels[t]), int(labels[t - 1])
        if i == j:
            v = dt(dt(v + tr[i, i]) + xb[t, i])
            continue
        if not present[s, i]:
            return ninf
        c = dt(dt(v + tr[i, j]) + arcw[s, i])
        if i == sep:
            st = step(h, int(wos[s]))
            if st is None:
                return ninf
            h, c = st[0], dt(c + st[1])
        s = int(g.next[s, i])
        v = dt(c + xb[t, i])
    if s == 0:
        endw = ew[h]
    elif wos[s] >= 0:
        st = step(h, int(wos[s]))
        if st is None:
            return ninf
        endw = dt(st[1] + ew[st[0]])
    else:
        return ninf
    return dt(dt(v + finw[s]) + endw)


def best_by_enumeration(xb, tr, lexicon, lm, **kw):
    """The largest path score over ALL label sequences of xb's length."""
    T, N = xb.shape
    best = xb.dtype.type(-np.inf)
    with np.errstate(invalid="ignore"):
        for labels in itertools.product(range(N), repeat=T):
            s = path_score_words(xb, tr, lexicon, lm, labels, **kw)
            if s > best:
                best = s
    return best
