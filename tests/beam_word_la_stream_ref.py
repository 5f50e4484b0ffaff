"""Test-only numpy restatements of the two word streams WITH LM LOOK-AHEAD (`torch_asg_amd.BeamWordStream(..., lookahead=)` and
`BeamWordWindowStream(..., lookahead=)`), written from the specification (include/asg_hip.h::asg_beam_word_stream_advance_la) and
not from the package: no ranks, no sorted rows, no table.  The carried state, the prune, the LM walk and the folding are those
of tests/beam_word_stream_ref.py (`BeamWordStreamRef`), the ring and the commit attempt those of tests/beam_word_window_ref.py
(`BeamWordWindowRef`); L(h, n) is tests/beam_word_la_ref.py's `Look`, plain loops over the arcs of a row.  What changes is what
the header changes: the frame adds the look-ahead terms of asg_beam_decode_words_la, the end takes L back, and the best PREFIX
is the largest v - L(h, state(q)).  L of every kept pair is asserted finite wherever it is read (`BeamWordLaStreamRef.L`).

`dead` counts, over the stream, the candidates dropped because the look-ahead of their target is -inf.  The window records per
slot `forced` = [(the pair the forced commit followed, the pair of the largest v)], for the tests that need the two to differ.
"""
import numpy as np

from beam_word_la_ref import Look
from beam_word_stream_ref import BeamWordStreamRef
from beam_word_window_ref import BeamWordWindowRef


class BeamWordLaStreamRef(BeamWordStreamRef):
    def __init__(self, transition, lexicon, lm, order, batch_size=1, max_frames=1, beam_size=1, beam_threshold=np.inf,
                 lm_weight=1.0, word_score=0.0, token_score=0.0, dtype=np.float32):
        super().__init__(transition, lexicon, lm, batch_size, max_frames, beam_size, beam_threshold, lm_weight, word_score,
                         token_score, dtype)
        self.order = int(order)
        self.look = Look(lexicon, lm, self.order, self.dt, self.lw, self.bw)
        self.dead = 0

    def L(self, h, q):
        """L(h, state(q)) of a KEPT pair: finite by construction."""
        ls = self.look.L(h, self.state[q])
        assert ls > self.ninf, (h, q)
        return ls

    def winner(self, A, final):
        """(end, pair, final word or -1) of the best end over the kept list A, or None."""
        dt, state, wos = self.dt, self.state, self.wos
        win = None
        for (h, q), v in A:
            fw = -1
            ls = self.L(h, q)
            if not final:
                e = dt(v - ls)                               # the best prefix: the estimate that has not cancelled is taken back
            else:
                st_ = state[q]
                if st_ == 0:
                    endw = self.ew[h]
                elif wos[st_] >= 0:
                    w = self.step(h, int(wos[st_]))
                    if w is None:
                        continue
                    endw = dt(dt(w[1] - ls) + self.ew[w[0]])
                    fw = int(wos[st_])
                else:
                    continue                                 # mid-word: no end
                e = dt(dt(v + self.finw[st_]) + endw)
            if e > self.ninf and (win is None or e > win[0] or (e == win[0] and (h, q) < win[1])):
                win = (e, (h, q), fw)
        return win

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
                win = self.winner(s.A, final)
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

    def _frame(self, s, xt, tr, theta):
        dt, label, state, ninf = self.dt, self.label, self.state, self.ninf
        if s.pos == 0:
            cand = {(self.lstart, q): dt(dt(self.start_w[q] + self.look.L(self.lstart, state[q])) + xt[label[q]])
                    for q in range(self.Q) if self.start_w[q] > ninf}
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
                ls = self.L(h, q)
                c = dt(v + tr[j, j])                         # the stay: the same node, nothing added
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
                        c = dt(c + dt(w[1] - ls))
                    else:
                        lt = self.look.L(h, state[q2])
                        if not lt > ninf:                    # a dead end is pruned on entry
                            self.dead += 1
                            continue
                        c = dt(c + dt(lt - ls))
                    if c > ninf:
                        nc += 1
                        offer((h2, q2), c, (h, q))
            self.src_ties += sum(1 for v_ in best.values() if v_[2] > 1)
            s.A = self._prune({tp: dt(v_[0] + xt[label[tp[1]]]) for tp, v_ in best.items()}, theta)
            s.back.append({p: best[p][1] for p, _ in s.A})
        for (h, q), _ in s.A:
            self.L(h, q)                                     # every kept pair has a finite look-ahead
        s.sizes.append(len(s.A))
        s.cands.append(nc)
        s.kept.append(sorted(p for p, _ in s.A))
        s.pos += 1


class BeamWordLaWindowRef(BeamWordWindowRef):
    def __init__(self, transition, lexicon, lm, order, batch_size=1, window=1, commit_every=None, beam_size=1,
                 beam_threshold=np.inf, lm_weight=1.0, word_score=0.0, token_score=0.0, dtype=np.float32):
        super().__init__(transition, lexicon, lm, batch_size, window, commit_every, beam_size, beam_threshold, lm_weight,
                         word_score, token_score, dtype)
        self.s = BeamWordLaStreamRef(transition, lexicon, lm, order, batch_size, 1, beam_size, beam_threshold, lm_weight,
                                     word_score, token_score, dtype)

    def result(self, final=False):
        """-> a dict with the keys of beam_word_window_ref.RESULT"""
        B, W, dt, s = self.B, self.W, self.dt, self.s
        res = {"scores": np.full(B, -np.inf, dt), "token_lengths": np.zeros(B, np.int64), "word_lengths": np.zeros(B, np.int64),
               "frames": np.array([v.pos for v in self.slots], np.int64),
               "committed": np.array([v.base for v in self.slots], np.int64),
               "status": np.array([v.status | (2 if v.pos >= 1 and not v.A else 0) for v in self.slots], np.int64)}
        for n in ("path", "tokens", "states", "lm_states", "words"):
            res[n] = np.full((B, W), -1, np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            for b, v in enumerate(self.slots):
                if v.pos == 0 or not v.A:
                    continue
                win = s.winner(v.A, final)
                if win is None:
                    continue
                res["scores"][b] = win[0]
                out = ([], [], [], [], [])
                self._append(v.carry, v.carry_state, self._walk(v, win[1], v.pos - 1, v.base), out)
                if win[2] >= 0:
                    out[4].append(win[2])
                assert all(len(o) <= W for o in out)
                for n, o in zip(("path", "states", "lm_states", "tokens", "words"), out):
                    res[n][b, :len(o)] = o
                res["token_lengths"][b], res["word_lengths"][b] = len(out[3]), len(out[4])
        return res

    def _attempt(self, v, out):
        W, P, pos, base0 = self.W, self.P, v.pos, v.base
        # 1. convergence: slots only, as without look-ahead
        R = set(p for p, _ in v.A)
        c = None
        if len(R) == 1:
            c = pos - 1
        else:
            for u in range(pos - 1, v.base, -1):
                row = self._row(v, u)
                R = set(row[p] for p in R)
                if len(R) == 1:
                    c = u - 1
                    break
        if c is not None:
            self._commit(v, self._walk(v, next(iter(R)), c, v.base), out)
            assert v.base == c + 1
        # 2. forced commit: along the best prefix pair, the largest v - L
        F = 0
        if pos - v.base > W - P:
            F = (pos - v.base) - (W - P)
            with np.errstate(invalid="ignore", over="ignore"):
                best = self.s.winner(v.A, False)[1]
            plain = min(v.A, key=lambda it: (-it[1], it[0]))[0]
            v.__dict__.setdefault("forced", []).append((best, plain))
            self._commit(v, self._walk(v, best, pos - 1, v.base)[:F], out)
            v.status |= 1
        assert pos - v.base <= W - P
        v.attempts.append((pos, base0, c, F))
