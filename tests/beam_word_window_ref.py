"""Test-only numpy restatement of WINDOWED streaming beam decoding with a lexicon and a word n-gram LM
(`torch_asg_amd.BeamWordWindowStream`), written from the specification (include/asg_hip.h::asg_beam_word_window_advance) and
not from the package.  The frame step is that of tests/beam_word_stream_ref.py (`BeamWordStreamRef._frame`), as
tests/beam_window_ref.py builds on tests/beam_stream_ref.py: the window never touches the search.

The carried state is explicit, per slot: `pos`, `base`, the kept pairs `A` = [((h, q), value)], `carry` (label of the last
committed frame), `carry_state` (its automaton state), the sticky `status` and the `ring` of W rows -- row u mod W holds (u,
{kept pair of frame u: its source pair}) and every read checks that the row still belongs to the frame it is read for, so a
commit rule that let a live row be overwritten fails here and not silently.  A row names a source by its pair where the device
names it by its slot: a pair is in a set once, so the two say the same.  `attempts` records, per slot, (pos, base before, c or
None, forced F) of every commit attempt, and `commits` (first frame, last frame) of every committed segment, for the tests.

What a committed frame with pair (h, q) appends: label[q] to the path, state[q] to the states, h to the LM states; the label to
the tokens if it is not `carry`; word_of_state[carry_state] to the words if the label is the separator and `carry` is another
label (not -1: frame 0 has no edge); then carry, carry_state = label[q], state[q].  `result` walks the uncommitted tail by the
same rule, started from the carries, without changing them.
"""
import numpy as np

from beam_word_stream_ref import BeamWordStreamRef

COMMIT = ("path", "states", "lm_states", "tokens", "words", "frames", "token_lengths", "word_lengths")
RESULT = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths", "frames", "committed",
          "status")


class _Slot:
    def __init__(self, W):
        self.pos, self.base, self.carry, self.carry_state, self.status = 0, 0, -1, -1, 0
        self.A = []
        self.back, self.sizes, self.cands, self.kept = [], [], [], []     # (what _frame appends to; the ring is filled from it)
        self.ring = [None] * W
        self.attempts, self.commits = [], []


class BeamWordWindowRef:
    def __init__(self, transition, lexicon, lm, batch_size=1, window=1, commit_every=None, beam_size=1, beam_threshold=np.inf,
                 lm_weight=1.0, word_score=0.0, token_score=0.0, dtype=np.float32):
        self.W = int(window)
        self.P = max(1, self.W // 4) if commit_every is None else int(commit_every)
        assert self.W >= 1 and 1 <= self.P <= self.W
        self.s = BeamWordStreamRef(transition, lexicon, lm, batch_size, 1, beam_size, beam_threshold, lm_weight, word_score,
                                   token_score, dtype)
        self.B, self.dt = self.s.B, self.s.dt
        self.slots = [_Slot(self.W) for _ in range(self.B)]

    # ---- the three entry points
    def reset(self, mask=None):
        for b in range(self.B):
            if mask is None or mask[b]:
                self.slots[b] = _Slot(self.W)

    def advance(self, chunk, chunk_lengths=None, transition=None, beam_threshold=None):
        """-> new_path, new_states, new_lm_states, new_tokens, new_words [B][W + Tc], new_frames, new_token_lengths,
        new_word_lengths [B] (the order of COMMIT)"""
        x = np.asarray(chunk)
        Tc, B, N = x.shape
        s = self.s
        assert B == self.B and x.dtype.type == self.dt
        tr = np.ascontiguousarray(np.asarray(s.transition if transition is None else transition), dtype=self.dt)
        theta = self.dt(s.beam_threshold if beam_threshold is None else beam_threshold)
        assert theta >= 0
        cols = self.W + Tc
        wide = [np.full((B, cols), -1, np.int64) for _ in range(5)]
        narrow = [np.zeros(B, np.int64) for _ in range(3)]
        with np.errstate(invalid="ignore", over="ignore"):
            for b, v in enumerate(self.slots):
                n = Tc if chunk_lengths is None else int(min(max(int(chunk_lengths[b]), 0), Tc))
                out = ([], [], [], [], [])                   # path, states, lm_states, tokens, words
                for t in range(n):
                    u = v.pos
                    s._frame(v, x[t, b], tr, theta)          # pos += 1, the set, back[-1] = {kept pair: source pair}
                    v.ring[u % self.W] = (u, v.back.pop())
                    v.sizes.pop(), v.cands.pop(), v.kept.pop()
                    if v.pos % self.P == 0 and v.A:
                        self._attempt(v, out)
                assert all(len(o) <= cols for o in out) and len(out[0]) == len(out[1]) == len(out[2])
                for a, o in zip(wide, out):
                    a[b, :len(o)] = o
                narrow[0][b], narrow[1][b], narrow[2][b] = len(out[0]), len(out[3]), len(out[4])
        return tuple(wide) + tuple(narrow)

    def result(self, final=False):
        """-> a dict with the keys of RESULT"""
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
                win = None                                   # (end, pair, final word or -1)
                for (h, q), val in v.A:
                    fw = -1
                    if not final:
                        e = val                              # the best prefix: no final weight, no LM end, no final word
                    else:
                        st_ = s.state[q]
                        if st_ == 0:
                            endw = s.ew[h]
                        elif s.wos[st_] >= 0:
                            w = s.step(h, int(s.wos[st_]))
                            if w is None:
                                continue
                            endw = dt(w[1] + s.ew[w[0]])
                            fw = int(s.wos[st_])
                        else:
                            continue                         # mid-word: no end
                        e = dt(dt(val + s.finw[st_]) + endw)
                    if e > s.ninf and (win is None or e > win[0] or (e == win[0] and (h, q) < win[1])):
                        win = (e, (h, q), fw)
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

    # ---- the ring and the commit attempt
    def _row(self, v, u):
        """{kept pair: source pair} of frame u, which must still be in the ring."""
        assert v.base <= u < v.pos and v.pos - v.base <= self.W
        row = v.ring[u % self.W]
        assert row is not None and row[0] == u, "the row of frame %d was overwritten" % u
        return row[1]

    def _walk(self, v, p, top, lo):
        """The pairs of the frames lo .. top on the path that holds pair p at frame `top`, ascending."""
        ps = []
        for u in range(top, lo - 1, -1):
            ps.append(p)
            if u > lo:
                p = self._row(v, u)[p]
        return ps[::-1]

    def _append(self, carry, carry_state, pairs, out):
        """The five lists of a segment of pairs behind (carry, carry_state) -> the carries behind it."""
        s = self.s
        for h, q in pairs:
            lab, sta = int(s.label[q]), int(s.state[q])
            out[0].append(lab)
            out[1].append(sta)
            out[2].append(int(h))
            if lab != carry:
                out[3].append(lab)
            if lab == s.sep and carry != s.sep and carry != -1:
                out[4].append(int(s.wos[carry_state]))
            carry, carry_state = lab, sta
        return carry, carry_state

    def _commit(self, v, pairs, out):
        if pairs:
            v.commits.append((v.base, v.base + len(pairs) - 1))
        v.carry, v.carry_state = self._append(v.carry, v.carry_state, pairs, out)
        v.base += len(pairs)

    def _attempt(self, v, out):
        W, P, pos, base0 = self.W, self.P, v.pos, v.base
        # 1. convergence
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
        # 2. forced commit
        F = 0
        if pos - v.base > W - P:
            F = (pos - v.base) - (W - P)
            best = min(v.A, key=lambda it: (-it[1], it[0]))  # the best prefix pair: v descending, pair order
            self._commit(v, self._walk(v, best[0], pos - 1, v.base)[:F], out)
            v.status |= 1
        assert pos - v.base <= W - P
        v.attempts.append((pos, base0, c, F))
