"""Test-only numpy restatement of STREAMING beam decoding with a lexicon and a word n-gram LM (`torch_asg_amd.BeamWordStream`),
written from the specification (include/asg_hip.h::asg_beam_word_stream_advance and asg_beam_decode_words) and not from the
package; it does not call tests/beam_word_ref.py either -- tests/test_beam_word_stream_cpu.py holds the two to each other.
Folding and product states of the lexicon automaton are those of tests/graph_decode_ref.py (`fold`, `product`, with lm_weight
1), the folding of the LM that of tests/beam_word_ref.py (`fold_lm`).

The state that is carried from chunk to chunk is explicit, per slot: `pos` (frames consumed), the kept pairs `A` = [((h, q),
value)], `back` (per consumed frame {kept pair: source pair}), the sticky `overflow` word -- and, for the tests, `sizes` (|A_t|),
`cands` (candidates of frame t, the -inf ones excluded) and `kept` (the pairs of A_t, sorted) of every consumed frame, with the
stream's totals `tie_cuts` (frames whose K-th and (K+1)-th candidate pair had equal values) and `src_ties` (targets whose best
value came from more than one source).  `reset` / `advance` / `result(final)` are the three entry points.  A frame looks at
nothing but the stored set and its own emissions: frame 0 of an utterance takes the pairs (start, q) of the start states, every
other frame -- the first of a chunk included -- its candidates from the stored set.  All arithmetic in the dtype of the stream, in
the order the specification gives: stay v + tr[j][j]; edge (v + tr[i][j]) + ow, on a separator edge + a, a being the LM walk's own
sum; then + emission.  Pairs order by h, then q.
"""
import numpy as np

from beam_word_ref import fold_lm
from graph_decode_ref import fold, product

NAMES = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths", "frames", "status")


class _Slot:
    def __init__(self):
        self.pos, self.overflow = 0, 0
        self.A, self.back = [], []
        self.sizes, self.cands, self.kept = [], [], []


class BeamWordStreamRef:
    def __init__(self, transition, lexicon, lm, batch_size=1, max_frames=1, beam_size=1, beam_threshold=np.inf, lm_weight=1.0,
                 word_score=0.0, token_score=0.0, dtype=np.float32):
        self.dt = dt = np.dtype(dtype).type
        self.B, self.max_frames, self.K = int(batch_size), int(max_frames), int(beam_size)
        assert self.B >= 1 and self.max_frames >= 1 and self.K >= 1
        self.transition, self.beam_threshold = transition, beam_threshold
        g = lexicon.graph
        self.sep = int(lexicon.separator)
        self.wos = np.asarray(lexicon.word_of_state, np.int64)
        nxt = np.asarray(g.next, np.int64)
        present, arcw, self.finw = fold(nxt, g.weight, g.final, dt, 1.0, token_score)
        self.label, self.state, src, tgt, self.Q = product(nxt, present)
        label, state = self.label, self.state
        self.ninf = dt(-np.inf)
        self.start_w = np.where(present[0, label] & (nxt[0, label] == state), arcw[0, label], self.ninf).astype(dt)
        self.out_edges = [[] for _ in range(self.Q)]         # per source: (target, weight)
        for s_, t_ in zip(src, tgt):
            self.out_edges[s_].append((int(t_), arcw[state[s_], label[t_]]))
        self.lw, self.bw, self.ew = fold_lm(lm, dt, lm_weight, word_score)
        self.row, self.word, self.lnext, self.backoff = (np.asarray(a, np.int64) for a in (lm.row, lm.word, lm.next, lm.backoff))
        self.lstart = int(lm.start)
        self.slots = [_Slot() for _ in range(self.B)]
        self.tie_cuts = self.src_ties = 0

    def step(self, h, w):
        """The LM walk: (next state, a) or None."""
        dt = self.dt
        a = dt(0)
        if w < 0:
            return None
        while True:
            lo, hi = self.row[h], self.row[h + 1]
            k = lo + np.searchsorted(self.word[lo:hi], w)
            if k < hi and self.word[k] == w:
                return int(self.lnext[k]), dt(a + self.lw[k])
            if self.backoff[h] < 0:
                return None
            a = dt(a + self.bw[h])
            h = int(self.backoff[h])

    # ---- the three entry points
    def reset(self, mask=None):
        for b in range(self.B):
            if mask is None or mask[b]:
                self.slots[b] = _Slot()

    def advance(self, chunk, chunk_lengths=None, transition=None, beam_threshold=None):
        """chunk [Tc,B,N]; `transition` / `beam_threshold`: the values for the frames of this call (default: the constructor's)."""
        x = np.asarray(chunk)
        Tc, B, N = x.shape
        assert B == self.B and x.dtype.type == self.dt
        tr = np.ascontiguousarray(np.asarray(self.transition if transition is None else transition), dtype=self.dt)
        theta = self.dt(self.beam_threshold if beam_threshold is None else beam_threshold)
        assert theta >= 0
        with np.errstate(invalid="ignore", over="ignore"):
            for b, s in enumerate(self.slots):
                want = Tc if chunk_lengths is None else int(min(max(int(chunk_lengths[b]), 0), Tc))
                n = min(want, self.max_frames - s.pos)
                if n < want:
                    s.overflow = 1
                for t in range(n):
                    self._frame(s, x[t, b], tr, theta)

    def result(self, final=False):
        B, T, dt = self.B, self.max_frames, self.dt
        label, state, wos = self.label, self.state, self.wos
        res = {"scores": np.full(B, -np.inf, dt), "token_lengths": np.zeros(B, np.int64), "word_lengths": np.zeros(B, np.int64),
               "frames": np.array([s.pos for s in self.slots], np.int64),
               "status": np.array([s.overflow for s in self.slots], np.int64)}
        for n in ("path", "tokens", "states", "lm_states", "words"):
            res[n] = np.full((B, T), -1, np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            for b, s in enumerate(self.slots):
                L = s.pos
                if L == 0 or not s.A:
                    continue
                win = None                                   # (end, pair, final word or -1)
                for (h, q), v in s.A:
                    fw = -1
                    if not final:
                        e = v                                # the best prefix: no final weight, no LM end, no final word
                    else:
                        st_ = state[q]
                        if st_ == 0:
                            endw = self.ew[h]
                        elif wos[st_] >= 0:
                            w = self.step(h, int(wos[st_]))
                            if w is None:
                                continue
                            endw = dt(w[1] + self.ew[w[0]])
                            fw = int(wos[st_])
                        else:
                            continue                         # mid-word: no end
                        e = dt(dt(v + self.finw[st_]) + endw)
                    if e > self.ninf and (win is None or e > win[0] or (e == win[0] and (h, q) < win[1])):
                        win = (e, (h, q), fw)
                if win is None:
                    continue
                res["scores"][b] = win[0]
                p = win[1]
                pairs = [None] * L
                for t in range(L - 1, -1, -1):
                    pairs[t] = p
                    p = s.back[t][p]
                wl = []
                for t in range(L):
                    h, q = pairs[t]
                    res["path"][b, t], res["states"][b, t], res["lm_states"][b, t] = label[q], state[q], h
                    if t >= 1 and pairs[t][1] != pairs[t - 1][1] and label[q] == self.sep:      # a separator edge
                        wl.append(int(wos[state[pairs[t - 1][1]]]))
                if win[2] >= 0:
                    wl.append(win[2])
                res["words"][b, :len(wl)] = wl
                res["word_lengths"][b] = len(wl)
                pl = res["path"][b, :L]
                keep = np.ones(L, bool)
                keep[1:] = pl[1:] != pl[:-1]
                tk = pl[keep]
                res["tokens"][b, :len(tk)] = tk
                res["token_lengths"][b] = len(tk)
        return res

    def sizes(self):
        return [list(s.sizes) for s in self.slots]

    def cands(self):
        return [list(s.cands) for s in self.slots]

    def kept(self):
        return [list(s.kept) for s in self.slots]

    # ---- one frame of one slot
    def _prune(self, cand, theta):
        """{pair: c} -> the kept list [(pair, c)]: c descending, pair order; the first K with c >= fl(max - theta)."""
        items = [(p, c) for p, c in cand.items() if c > self.ninf]
        if not items:
            return []
        lo = self.dt(max(c for _, c in items) - theta)
        items = [it for it in sorted(items, key=lambda it: (-it[1], it[0])) if it[1] >= lo]
        if len(items) > self.K and items[self.K - 1][1] == items[self.K][1]:
            self.tie_cuts += 1
        return items[:self.K]

    def _frame(self, s, xt, tr, theta):
        dt, label, state, ninf = self.dt, self.label, self.state, self.ninf
        if s.pos == 0:
            cand = {(self.lstart, q): dt(self.start_w[q] + xt[label[q]]) for q in range(self.Q) if self.start_w[q] > ninf}
            s.A = self._prune(cand, theta)
            s.back.append({p: None for p, _ in s.A})
            nc = len(cand)
        elif not s.A:                                        # an empty set stays empty
            s.back.append({})
            nc = 0
        else:
            best = {}                                        # target pair -> [value, source pair, sources at that value]
            nc = 0

            def offer(tp, c, sp):
                cur = best.get(tp)
                if cur is None or c > cur[0]:
                    best[tp] = [c, sp, 1]
                elif c == cur[0]:
                    cur[2] += 1
                    if sp < cur[1]:
                        cur[1] = sp
            for (h, q), v in s.A:
                j = label[q]
                c = dt(v + tr[j, j])
                if c > ninf:
                    nc += 1
                    offer((h, q), c, (h, q))
                for q2, w_e in self.out_edges[q]:
                    i = label[q2]
                    c = dt(dt(v + tr[i, j]) + w_e)
                    h2 = h
                    if i == self.sep:
                        w = self.step(h, int(self.wos[state[q]]))
                        if w is None:
                            continue
                        h2 = w[0]
                        c = dt(c + w[1])
                    if c > ninf:
                        nc += 1
                        offer((h2, q2), c, (h, q))
            self.src_ties += sum(1 for v_ in best.values() if v_[2] > 1)
            s.A = self._prune({tp: dt(v_[0] + xt[label[tp[1]]]) for tp, v_ in best.items()}, theta)
            s.back.append({p: best[p][1] for p, _ in s.A})
        s.sizes.append(len(s.A))
        s.cands.append(nc)
        s.kept.append(sorted(p for p, _ in s.A))
        s.pos += 1
