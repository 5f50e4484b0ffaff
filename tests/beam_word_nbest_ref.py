"""Test-only numpy restatement of the N BEST hypotheses of beam decoding with a lexicon and a word n-gram LM
(`torch_asg_amd.beam_decode_words_nbest`, `BeamWordStream.result_nbest`), written from the specification
(include/asg_hip.h::asg_beam_decode_words_nbest and asg_beam_decode_words) and not from the package.  The search is restated
here once more, because tests/beam_word_ref.py keeps neither the values of the last set nor its back-pointers outside its loop;
tests/test_beam_word_nbest_cpu.py holds row 0 of this file to that one, and to tests/beam_word_stream_ref.py.  Folding and
product states are those of tests/graph_decode_ref.py (`fold`, `product`, lm_weight 1), the LM's folding that of
tests/beam_word_ref.py (`fold_lm`).

`WordSearch` is the search as a state carried frame by frame (per slot: `pos`, the kept pairs `A` = [((h, q), value)], `back`
per frame {kept pair: source pair}, and the frames and transitions it consumed, which only the emission sum reads);
`nbest(slot, n, final)` ranks the last set and walks the back-pointers.  `beam_word_nbest_ref` is the one-shot call,
`BeamWordNbestStreamRef` the stream.  All arithmetic in the dtype of the emissions, in the order the specification gives.
Besides the twelve outputs a result holds, per row, `nterms` (the number of terms the three sums add, the inner terms of every
LM walk included) and `sumabs` (the sum of their magnitudes, float64): the bound on |scores - (e + g + l)| is
2 * nterms * eps * sumabs and no other.
"""
import numpy as np

from beam_word_ref import fold_lm
from graph_decode_ref import _clamped_lengths, fold, product

SCORES = ("scores", "emission_scores", "graph_scores", "lm_scores")
WIDE = ("tokens", "words", "path", "states", "lm_states")
NARROW = ("token_lengths", "word_lengths")
NAMES = ("scores", "emission_scores", "graph_scores", "lm_scores", "tokens", "token_lengths", "words", "word_lengths", "num_hyps",
         "path", "states", "lm_states")


class _Slot:
    def __init__(self):
        self.pos, self.overflow = 0, 0
        self.A, self.back, self.x, self.tr = [], [], [], []
        self.sizes = []


class WordSearch:
    def __init__(self, lexicon, lm, dtype, beam_size, lm_weight=1.0, word_score=0.0, token_score=0.0):
        self.dt = dt = np.dtype(dtype).type
        self.K = int(beam_size)
        assert self.K >= 1
        g = lexicon.graph
        self.sep = int(lexicon.separator)
        self.wos = np.asarray(lexicon.word_of_state, np.int64)
        nxt = np.asarray(g.next, np.int64)
        present, self.arcw, self.finw = fold(nxt, g.weight, g.final, dt, 1.0, token_score)
        self.label, self.state, src, tgt, self.Q = product(nxt, present)
        self.ninf = dt(-np.inf)
        self.start_w = np.where(present[0, self.label] & (nxt[0, self.label] == self.state), self.arcw[0, self.label],
                                self.ninf).astype(dt)
        self.out = [[] for _ in range(self.Q)]                # per source: targets
        for s_, t_ in zip(src, tgt):
            self.out[s_].append(int(t_))
        self.lw, self.bw, self.ew = fold_lm(lm, dt, lm_weight, word_score)
        self.row, self.word, self.lnext, self.backoff = (np.asarray(a, np.int64) for a in (lm.row, lm.word, lm.next, lm.backoff))
        self.lstart = int(lm.start)

    def ow(self, qp, q):
        """The folded weight of the edge qp -> q of the lexicon automaton."""
        return self.arcw[self.state[qp], self.label[q]]

    def step(self, h, w):
        """The LM walk -> (next state, a, the terms a adds) or None."""
        dt = self.dt
        a, terms = dt(0), []
        if w < 0:
            return None
        while True:
            lo, hi = self.row[h], self.row[h + 1]
            k = lo + np.searchsorted(self.word[lo:hi], w)
            if k < hi and self.word[k] == w:
                return int(self.lnext[k]), dt(a + self.lw[k]), terms + [self.lw[k]]
            if self.backoff[h] < 0:
                return None
            a = dt(a + self.bw[h])
            terms.append(self.bw[h])
            h = int(self.backoff[h])

    def prune(self, cand, theta):
        items = [(p, c) for p, c in cand.items() if c > self.ninf]
        if not items:
            return []
        lo = self.dt(max(c for _, c in items) - theta)
        return [it for it in sorted(items, key=lambda it: (-it[1], it[0])) if it[1] >= lo][:self.K]

    def frame(self, s, xt, tr, theta):
        dt, label, state, ninf = self.dt, self.label, self.state, self.ninf
        with np.errstate(invalid="ignore", over="ignore"):
            if s.pos == 0:
                cand = {(self.lstart, q): dt(self.start_w[q] + xt[label[q]]) for q in range(self.Q) if self.start_w[q] > ninf}
                s.A = self.prune(cand, theta)
                s.back.append({p: None for p, _ in s.A})
            elif not s.A:
                s.back.append({})
            else:
                best = {}                                    # target pair -> (value, source pair)

                def offer(tp, c, sp):
                    if c > ninf and (tp not in best or c > best[tp][0] or (c == best[tp][0] and sp < best[tp][1])):
                        best[tp] = (c, sp)
                for (h, q), v in s.A:
                    j = label[q]
                    offer((h, q), dt(v + tr[j, j]), (h, q))
                    for q2 in self.out[q]:
                        i = label[q2]
                        c = dt(dt(v + tr[i, j]) + self.ow(q, q2))
                        h2 = h
                        if i == self.sep:
                            w = self.step(h, int(self.wos[state[q]]))
                            if w is None:
                                continue
                            h2, c = w[0], dt(c + w[1])
                        offer((h2, q2), c, (h, q))
                s.A = self.prune({tp: dt(v_[0] + xt[label[tp[1]]]) for tp, v_ in best.items()}, theta)
                s.back.append({p: best[p][1] for p, _ in s.A})
        s.x.append(np.array(xt, copy=True))
        s.tr.append(tr)
        s.sizes.append(len(s.A))
        s.pos += 1

    def end(self, h, q, v):
        """-> (end, endw, its terms, final word or -1) or None."""
        dt = self.dt
        st = self.state[q]
        if st == 0:
            endw, terms, fw = self.ew[h], [self.ew[h]], -1
        elif self.wos[st] >= 0:
            w = self.step(h, int(self.wos[st]))
            if w is None:
                return None
            endw, terms, fw = dt(w[1] + self.ew[w[0]]), w[2] + [self.ew[w[0]]], int(self.wos[st])
        else:
            return None
        return dt(dt(v + self.finw[st]) + endw), endw, terms, fw

    def candidates(self, s, final):
        """The candidates of the stored set in order: [(end, pair)]."""
        out = []
        with np.errstate(invalid="ignore", over="ignore"):
            for (h, q), v in s.A:
                e = v
                if final:
                    r = self.end(h, q, v)
                    if r is None:
                        continue
                    e = r[0]
                if e > self.ninf:
                    out.append((e, (h, q)))
        return sorted(out, key=lambda it: (-it[0], it[1]))

    def hyp(self, s, e, pair, final):
        """One hypothesis: the outputs of its row and (nterms, sumabs)."""
        dt, label, state = self.dt, self.label, self.state
        L = s.pos
        pairs = [None] * L
        p = pair
        for t in range(L - 1, -1, -1):
            pairs[t] = p
            p = s.back[t][p]
        path = [int(label[q]) for _, q in pairs]
        terms = []
        with np.errstate(invalid="ignore", over="ignore"):
            a = dt(s.x[0][path[0]])
            terms.append(a)
            g = dt(self.start_w[pairs[0][1]])
            terms.append(g)
            l = dt(0)
            words = []
            for t in range(1, L):
                (hp, qp), (h, q) = pairs[t - 1], pairs[t]
                tr_ = s.tr[t][path[t], path[t - 1]]
                a = dt(dt(a + tr_) + s.x[t][path[t]])
                terms += [tr_, s.x[t][path[t]]]
                if q != qp:
                    g = dt(g + self.ow(qp, q))
                    terms.append(self.ow(qp, q))
                    if path[t] == self.sep:
                        w = self.step(hp, int(self.wos[state[qp]]))
                        assert w is not None and w[0] == h
                        l = dt(l + w[1])
                        terms += w[2]
                        words.append(int(self.wos[state[qp]]))
                else:
                    assert h == hp
            if final:
                h, q = pairs[-1]
                r = self.end(h, q, dict(s.A)[pair])
                g = dt(g + self.finw[state[q]])
                l = dt(l + r[1])
                terms += [self.finw[state[q]]] + r[2]
                if r[3] >= 0:
                    words.append(r[3])
        keep = [t for t in range(L) if t == 0 or path[t] != path[t - 1]]
        return dict(scores=e, emission_scores=a, graph_scores=g, lm_scores=l, path=path, states=[int(state[q]) for _, q in pairs],
                    lm_states=[int(h) for h, _ in pairs], tokens=[path[t] for t in keep], words=words, nterms=len(terms),
                    sumabs=float(np.sum(np.abs(np.asarray(terms, np.float64)))))

    def nbest(self, slots, T, nbest, final):
        """The n-best of every slot -> dict of arrays ([B, nbest, ...]), with num_cands [B] besides."""
        B, dt = len(slots), self.dt
        res = {n: np.full((B, nbest), -np.inf, dt) for n in SCORES}
        res.update({n: np.full((B, nbest, T), -1, np.int64) for n in WIDE})
        res.update({n: np.zeros((B, nbest), np.int64) for n in NARROW})
        res.update(num_hyps=np.zeros(B, np.int64), num_cands=np.zeros(B, np.int64), nterms=np.zeros((B, nbest), np.int64),
                   sumabs=np.zeros((B, nbest)))
        for b, s in enumerate(slots):
            if s.pos == 0:
                continue
            cands = self.candidates(s, final)
            res["num_cands"][b] = len(cands)
            res["num_hyps"][b] = min(nbest, len(cands))
            for r, (e, pair) in enumerate(cands[:nbest]):
                row = self.hyp(s, e, pair, final)
                for n in SCORES:
                    res[n][b, r] = row[n]
                for n in WIDE:
                    res[n][b, r, :len(row[n])] = row[n]
                res["token_lengths"][b, r], res["word_lengths"][b, r] = len(row["tokens"]), len(row["words"])
                res["nterms"][b, r], res["sumabs"][b, r] = row["nterms"], row["sumabs"]
        return res


def beam_word_nbest_ref(inputs, transition, lexicon, lm, input_lengths=None, beam_size=1, nbest=1, beam_threshold=np.inf,
                        lm_weight=1.0, word_score=0.0, token_score=0.0, info=None):
    """inputs [T,B,N], transition [N,N] -> dict of the twelve outputs (NAMES; path, states and lm_states always), nterms, sumabs
    [B,nbest] and num_cands [B].  `info`, if a dict, receives sizes (|A_t| per utterance)."""
    x = np.asarray(inputs)
    T, B, N = x.shape
    dt = x.dtype.type
    search = WordSearch(lexicon, lm, dt, beam_size, lm_weight, word_score, token_score)
    tr = np.asarray(transition).astype(dt)
    theta = dt(beam_threshold)
    assert theta >= 0 and nbest >= 1
    lens = _clamped_lengths(input_lengths, T, B)
    slots = [_Slot() for _ in range(B)]
    for b, s in enumerate(slots):
        for t in range(int(lens[b]) if search.Q else 0):
            search.frame(s, x[t, b], tr, theta)
    if info is not None:
        info["sizes"] = [list(s.sizes) for s in slots]
    return search.nbest(slots, T, int(nbest), True)


class BeamWordNbestStreamRef:
    """The stream: reset / advance as include/asg_hip.h::asg_beam_word_stream_advance, result_nbest(nbest, final)."""

    def __init__(self, transition, lexicon, lm, batch_size=1, max_frames=1, beam_size=1, beam_threshold=np.inf, lm_weight=1.0,
                 word_score=0.0, token_score=0.0, dtype=np.float32):
        self.search = WordSearch(lexicon, lm, dtype, beam_size, lm_weight, word_score, token_score)
        self.B, self.max_frames = int(batch_size), int(max_frames)
        self.transition, self.beam_threshold = transition, beam_threshold
        self.slots = [_Slot() for _ in range(self.B)]

    def reset(self, mask=None):
        for b in range(self.B):
            if mask is None or mask[b]:
                self.slots[b] = _Slot()

    def advance(self, chunk, chunk_lengths=None):
        x = np.asarray(chunk)
        Tc, B, N = x.shape
        dt = self.search.dt
        assert B == self.B and x.dtype.type == dt
        tr = np.ascontiguousarray(np.asarray(self.transition), dtype=dt)
        theta = dt(self.beam_threshold)
        for b, s in enumerate(self.slots):
            want = Tc if chunk_lengths is None else int(min(max(int(chunk_lengths[b]), 0), Tc))
            n = min(want, self.max_frames - s.pos)
            if n < want:
                s.overflow = 1
            for t in range(n):
                self.search.frame(s, x[t, b], tr, theta)

    def result_nbest(self, nbest, final=False):
        res = self.search.nbest(self.slots, self.max_frames, int(nbest), final)
        res["frames"] = np.array([s.pos for s in self.slots], np.int64)
        res["status"] = np.array([s.overflow for s in self.slots], np.int64)
        return res
