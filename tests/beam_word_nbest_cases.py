"""What the CPU and GPU tests of the n-best over pairs share (tests/test_beam_word_nbest_cpu.py, tests/test_hip_beam_word_nbest.py):
a scorer of ONE label path that also returns the three parts of its score, its tokens and its words, written apart from the
search (tests/beam_word_nbest_ref.py) beside tests/beam_word_cases.py::path_score_words; the enumeration of all label paths
grouped by token sequence; and the bound that holds the split to the score."""
import itertools

import numpy as np

from beam_word_ref import fold_lm
from graph_decode_ref import fold


def path_parts_words(xb, tr, lexicon, lm, labels, final=True, lm_weight=1.0, word_score=0.0, token_score=0.0):
    """One label sequence under the specification's adds -> (score, emission, graph, lm, tokens, words, pair), or None if the
    lexicon or the LM rejects it (with `final`: also if it ends mid-word).  Without `final`: a prefix, no end terms, no final
    word.  pair: (LM state, lexicon state, last label) before the end, which names the search's pair (h, q)."""
    dt = xb.dtype.type
    g = lexicon.graph
    sep, wos = lexicon.separator, lexicon.word_of_state
    present, arcw, finw = fold(g.next, g.weight, g.final, dt, 1.0, token_score)
    lw, bw, ew = fold_lm(lm, dt, lm_weight, word_score)

    def step(h, w):
        a = dt(0)
        while True:
            k = lm.find(h, w)
            if k >= 0:
                return int(lm.next[k]), dt(a + lw[k])
            if lm.backoff[h] < 0:
                return None
            a, h = dt(a + bw[h]), int(lm.backoff[h])
    labels = [int(i) for i in labels]
    l0 = labels[0]
    if not present[0, l0]:
        return None
    with np.errstate(invalid="ignore", over="ignore"):
        s, h = int(g.next[0, l0]), lm.start
        v = dt(arcw[0, l0] + xb[0, l0])
        em, gr, ls = dt(xb[0, l0]), dt(arcw[0, l0]), dt(0)
        tokens, words = [l0], []
        for t in range(1, len(labels)):
            i, j = labels[t], labels[t - 1]
            em = dt(dt(em + tr[i, j]) + xb[t, i])
            if i == j:
                v = dt(dt(v + tr[i, i]) + xb[t, i])
                continue
            if not present[s, i]:
                return None
            c = dt(dt(v + tr[i, j]) + arcw[s, i])
            gr = dt(gr + arcw[s, i])
            tokens.append(i)
            if i == sep:
                st = step(h, int(wos[s]))
                if st is None:
                    return None
                words.append(int(wos[s]))
                h, c, ls = st[0], dt(c + st[1]), dt(ls + st[1])
            s = int(g.next[s, i])
            v = dt(c + xb[t, i])
        pair = (h, s, labels[-1])
        if final:
            if s == 0:
                endw = ew[h]
            elif wos[s] >= 0:
                st = step(h, int(wos[s]))
                if st is None:
                    return None
                endw = dt(st[1] + ew[st[0]])
                words.append(int(wos[s]))
            else:
                return None
            v = dt(dt(v + finw[s]) + endw)
            gr, ls = dt(gr + finw[s]), dt(ls + endw)
    if not v > -np.inf:
        return None
    return v, em, gr, ls, tokens, words, pair


def enumerate_groups(xb, tr, lexicon, lm, final=True, by="tokens", **kw):
    """All label sequences of xb's length, grouped by collapsed token sequence -- or, by="pair", by the pair they end in: the
    search keeps one path per pair, so token sequences that reach one pair (histories that the LM no longer tells apart) share a
    row -> [(best parts of the group, ties)] sorted by score descending; ties: True if the group's best score is reached by two
    paths."""
    T, N = xb.shape
    groups = {}
    for labels in itertools.product(range(N), repeat=T):
        r = path_parts_words(xb, tr, lexicon, lm, labels, final, **kw)
        if r is None:
            continue
        key = tuple(r[4]) if by == "tokens" else r[6]
        cur = groups.get(key)
        if cur is None or r[0] > cur[0][0]:
            groups[key] = [r, False]
        elif r[0] == cur[0][0]:
            cur[1] = True
    return sorted(groups.values(), key=lambda it: -it[0][0])


def split_bound(res, dt):
    """|scores - (e + g + l)| and its bound 2 * n * eps * sum|terms|, float64, over the finite rows -> (difference, bound, mask)."""
    fin = np.isfinite(res["scores"])
    parts = sum(np.where(fin, res[n], 0).astype(np.float64) for n in ("emission_scores", "graph_scores", "lm_scores"))
    diff = np.abs(np.where(fin, res["scores"], 0).astype(np.float64) - parts)
    return diff, 2.0 * res["nterms"] * float(np.finfo(dt).eps) * res["sumabs"], fin
