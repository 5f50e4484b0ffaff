"""Test-only numpy restatement of the N BEST hypotheses of the lexicon + word-LM beam search WITH LM LOOK-AHEAD
(`torch_asg_amd.beam_decode_words_nbest(..., lookahead=)`, `BeamWordStream._result_nbest` of a look-ahead stream), written from
the specification (include/asg_hip.h::asg_beam_decode_words_nbest_la, asg_beam_decode_words_la and the prefix rule of
asg_beam_word_stream_result_la) and not from the package.

The search is tests/beam_word_la_ref.py's frame -- its `Look` (sets and loops: no ranks, no tables), its terms where the header
adds them -- carried frame by frame as tests/beam_word_nbest_ref.py::WordSearch carries the plain one, because the n-best reads
the values of the last set and every back-pointer.  tests/test_beam_word_la_nbest_cpu.py holds row 0 of this file to
beam_word_la_ref and to tests/beam_word_la_stream_ref.py.  Candidates, order and `scores` are the look-ahead search's own end
(final) or v - L(h, node) (prefix); the three parts are WordSearch.hyp's, untouched: no look-ahead term enters them.

Besides the outputs a result holds, per row, `nterms` and `sumabs` as beam_word_nbest_ref's, EXTENDED: every look-ahead value
the search adds on the path -- L of the start pair, L of the target of every edge into a node -- counts twice, once where it
enters and once where it leaves (the next edge out of the node, the separator edge, the end, or the reported prefix).  The bound
on |scores - (e + g + l)| is 2 * nterms * eps * sumabs and no other.  Every L read here is asserted finite.
"""
import numpy as np

from beam_word_la_ref import Look
from beam_word_nbest_ref import WordSearch, _Slot
from graph_decode_ref import _clamped_lengths


class WordLaSearch(WordSearch):
    def __init__(self, lexicon, lm, order, dtype, beam_size, lm_weight=1.0, word_score=0.0, token_score=0.0):
        super().__init__(lexicon, lm, dtype, beam_size, lm_weight, word_score, token_score)
        self.look = Look(lexicon, lm, int(order), self.dt, self.lw, self.bw)
        self.dead = 0                                        # candidates dropped because the look-ahead of their target is -inf

    def L(self, h, q):
        """L(h, state(q)) of a pair the search holds: finite."""
        v = self.look.L(h, self.state[q])
        assert v > self.ninf
        return v

    def frame(self, s, xt, tr, theta):
        dt, label, state, ninf = self.dt, self.label, self.state, self.ninf
        with np.errstate(invalid="ignore", over="ignore"):
            if s.pos == 0:
                cand = {}
                for q in range(self.Q):
                    if self.start_w[q] > ninf:
                        cand[(self.lstart, q)] = dt(dt(self.start_w[q] + self.look.L(self.lstart, state[q])) + xt[label[q]])
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
                    ls = self.L(h, q)
                    offer((h, q), dt(v + tr[j, j]), (h, q))
                    for q2 in self.out[q]:
                        i = label[q2]
                        c = dt(dt(v + tr[i, j]) + self.ow(q, q2))
                        h2 = h
                        if i == self.sep:
                            w = self.step(h, int(self.wos[state[q]]))
                            if w is None:
                                continue
                            h2, c = w[0], dt(c + dt(w[1] - ls))
                        else:
                            lt = self.look.L(h, state[q2])
                            if not lt > ninf:                 # a dead end is pruned where it would be entered
                                self.dead += 1
                                continue
                            c = dt(c + dt(lt - ls))
                        offer((h2, q2), c, (h, q))
                s.A = self.prune({tp: dt(v_[0] + xt[label[tp[1]]]) for tp, v_ in best.items()}, theta)
                s.back.append({p: best[p][1] for p, _ in s.A})
        s.x.append(np.array(xt, copy=True))
        s.tr.append(tr)
        s.sizes.append(len(s.A))
        s.pos += 1

    def la_end(self, h, q, v):
        """The end of asg_beam_decode_words_la, or None."""
        dt = self.dt
        st = self.state[q]
        if st == 0:
            endw = self.ew[h]
        elif self.wos[st] >= 0:
            w = self.step(h, int(self.wos[st]))
            if w is None:
                return None
            endw = dt(dt(w[1] - self.L(h, q)) + self.ew[w[0]])
        else:
            return None
        return dt(dt(v + self.finw[st]) + endw)

    def candidates(self, s, final):
        out = []
        with np.errstate(invalid="ignore", over="ignore"):
            for (h, q), v in s.A:
                e = self.la_end(h, q, v) if final else self.dt(v - self.L(h, q))
                if e is None:
                    continue
                if not final:
                    assert e > self.ninf                      # finite for every kept pair
                if e > self.ninf:
                    out.append((e, (h, q)))
        return sorted(out, key=lambda it: (-it[0], it[1]))

    def hyp(self, s, e, pair, final):
        """The plain row -- its three sums never see a look-ahead term -- with the bound's n and magnitude sum extended."""
        row = super().hyp(s, e, pair, final)
        L = s.pos
        pairs = [None] * L
        p = pair
        for t in range(L - 1, -1, -1):
            pairs[t] = p
            p = s.back[t][p]
        entered = [self.L(*pairs[0])]
        for t in range(1, L):
            (hp, qp), (h, q) = pairs[t - 1], pairs[t]
            if q != qp and self.label[q] != self.sep:
                entered.append(self.L(hp, q))
        row["nterms"] += 2 * len(entered)
        row["sumabs"] += 2.0 * float(np.sum(np.abs(np.asarray(entered, np.float64))))
        return row

    def sets(self, s):
        """The kept pairs of the slot's last set, sorted."""
        return sorted(p for p, _ in s.A)


def beam_word_la_nbest_ref(inputs, transition, lexicon, lm, order, input_lengths=None, beam_size=1, nbest=1, beam_threshold=np.inf,
                           lm_weight=1.0, word_score=0.0, token_score=0.0, info=None):
    """beam_word_nbest_ref's arguments plus `order` -> its dict.  `info`, if a dict, receives sizes (|A_t| per utterance) and
    last (the pairs of the last set per utterance) and dead (candidates dropped because their target's look-ahead is -inf)."""
    x = np.asarray(inputs)
    T, B, N = x.shape
    dt = x.dtype.type
    search = WordLaSearch(lexicon, lm, order, dt, beam_size, lm_weight, word_score, token_score)
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
        info["last"] = [search.sets(s) for s in slots]
        info["dead"] = search.dead
    return search.nbest(slots, T, int(nbest), True)


class BeamWordLaNbestStreamRef:
    """The stream: reset / advance as include/asg_hip.h::asg_beam_word_stream_advance_la, result_nbest(nbest, final)."""

    def __init__(self, transition, lexicon, lm, order, batch_size=1, max_frames=1, beam_size=1, beam_threshold=np.inf,
                 lm_weight=1.0, word_score=0.0, token_score=0.0, dtype=np.float32):
        self.search = WordLaSearch(lexicon, lm, order, dtype, beam_size, lm_weight, word_score, token_score)
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
