"""Test-only numpy restatement of WINDOWED streaming beam decoding (`torch_asg_amd.BeamWindowStream`), written from the
specification (include/asg_hip.h::asg_beam_window_advance) and not from the package.  The frame step is that of
tests/beam_stream_ref.py (`BeamStreamRef._frame`): the window never touches the search.

The carried state is explicit, per slot: `pos`, `base`, the active set `aq` / `av`, `carry`, the sticky `status` and the `ring`
of W rows -- row u mod W holds (u, active states of frame u, their sources) and every read checks that the row still belongs to
the frame it is read for, so a commit rule that let a live row be overwritten fails here and not silently.  A row names a source
by its product state where the device names it by its slot: a state is in a set once, so the two say the same.  `attempts`
records, per slot, (pos, base before, c or None, forced F) of every commit attempt, for the tests.
"""
import numpy as np

from beam_stream_ref import BeamStreamRef


class _Slot:
    def __init__(self, W):
        self.pos, self.base, self.carry, self.status = 0, 0, -1, 0
        self.aq, self.av = np.zeros(0, np.int64), None
        self.history, self.sizes = [], []                    # (what _frame appends to; the ring is filled from it)
        self.ring = [None] * W
        self.attempts = []


class BeamWindowRef:
    def __init__(self, transition, next_, weight, final, start=0, batch_size=1, window=1, commit_every=None, beam_size=1,
                 beam_threshold=np.inf, lm_weight=1.0, token_score=0.0, dtype=np.float32):
        self.W = int(window)
        self.P = max(1, self.W // 4) if commit_every is None else int(commit_every)
        assert self.W >= 1 and 1 <= self.P <= self.W
        self.s = BeamStreamRef(transition, next_, weight, final, start, batch_size, 1, beam_size, beam_threshold, lm_weight,
                               token_score, dtype)
        self.B, self.dt = self.s.B, self.s.dt
        self.slots = [_Slot(self.W) for _ in range(self.B)]

    # ---- the three entry points
    def reset(self, mask=None):
        for b in range(self.B):
            if mask is None or mask[b]:
                self.slots[b] = _Slot(self.W)

    def advance(self, chunk, chunk_lengths=None, transition=None, beam_threshold=None):
        """-> new_path, new_states, new_tokens [B][W + Tc], new_frames [B], new_token_lengths [B]"""
        x = np.asarray(chunk)
        Tc, B, N = x.shape
        s = self.s
        assert B == self.B and x.dtype.type == self.dt
        tr = np.ascontiguousarray(np.asarray(s.transition if transition is None else transition), dtype=self.dt)
        theta = self.dt(s.beam_threshold if beam_threshold is None else beam_threshold)
        assert theta >= 0
        cols = self.W + Tc
        new_path = np.full((B, cols), -1, np.int64)
        new_states = np.full((B, cols), -1, np.int64)
        new_tokens = np.full((B, cols), -1, np.int64)
        new_frames = np.zeros(B, np.int64)
        new_tlen = np.zeros(B, np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            for b, v in enumerate(self.slots):
                n = Tc if chunk_lengths is None else int(min(max(int(chunk_lengths[b]), 0), Tc))
                out = ([], [], [])
                for t in range(n):
                    u = v.pos
                    s._frame(v, x[t, b], tr, theta)          # pos += 1, the set, history[-1] = (aq, sources)
                    v.ring[u % self.W] = (u,) + v.history.pop()
                    v.sizes.pop()
                    if v.pos % self.P == 0 and v.aq.size:
                        self._attempt(v, out)
                assert len(out[0]) <= cols
                new_path[b, :len(out[0])], new_states[b, :len(out[1])], new_tokens[b, :len(out[2])] = out
                new_frames[b], new_tlen[b] = len(out[0]), len(out[2])
        return new_path, new_states, new_tokens, new_frames, new_tlen

    def result(self, final=False):
        """-> scores, path, tokens, token_lengths, states, frames, committed, status"""
        B, W, dt, s = self.B, self.W, self.dt, self.s
        scores = np.full(B, -np.inf, dt)
        path = np.full((B, W), -1, np.int64)
        tokens = np.full((B, W), -1, np.int64)
        token_lengths = np.zeros(B, np.int64)
        states = np.full((B, W), -1, np.int64)
        frames = np.array([v.pos for v in self.slots], np.int64)
        committed = np.array([v.base for v in self.slots], np.int64)
        status = np.array([v.status | (2 if v.pos >= 1 and v.aq.size == 0 else 0) for v in self.slots], np.int64)
        for b, v in enumerate(self.slots):
            if v.pos == 0 or v.aq.size == 0:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                end = v.av + s.finw[s.state[v.aq]] if final else v.av
            o = np.lexsort((v.aq, -end))[0]                  # end descending, q ascending
            if not end[o] > s.ninf:
                continue
            scores[b] = end[o]
            qs = self._walk(v, int(v.aq[o]), v.pos - 1, v.base)
            lab = s.label[qs]
            path[b, :len(qs)], states[b, :len(qs)] = lab, s.state[qs]
            prev = np.concatenate([[v.carry], lab[:-1]])
            tk = lab[lab != prev]
            tokens[b, :len(tk)] = tk
            token_lengths[b] = len(tk)
        return scores, path, tokens, token_lengths, states, frames, committed, status

    # ---- the ring and the commit attempt
    def _row(self, v, u):
        """(active states, their sources) of frame u, which must still be in the ring."""
        assert v.base <= u < v.pos and v.pos - v.base <= self.W
        row = v.ring[u % self.W]
        assert row is not None and row[0] == u, "the row of frame %d was overwritten" % u
        return row[1], row[2]

    def _walk(self, v, q, top, lo):
        """The product states of the frames lo .. top on the path that is in state q at frame `top`, ascending."""
        qs = []
        for u in range(top, lo - 1, -1):
            qs.append(q)
            if u > lo:
                fq, fs = self._row(v, u)
                q = int(fs[np.nonzero(fq == q)[0][0]])
        return np.array(qs[::-1], np.int64)

    def _commit(self, v, qs, out):
        s = self.s
        for q in qs:
            lab = int(s.label[q])
            out[0].append(lab)
            out[1].append(int(s.state[q]))
            if lab != v.carry:
                out[2].append(lab)
            v.carry = lab
        v.base += len(qs)

    def _attempt(self, v, out):
        W, P, pos, base0 = self.W, self.P, v.pos, v.base
        # 1. convergence
        R = set(int(q) for q in v.aq)
        c = None
        if len(R) == 1:
            c = pos - 1
        else:
            for u in range(pos - 1, v.base, -1):
                fq, fs = self._row(v, u)
                R = set(int(fs[i]) for i in range(fq.size) if int(fq[i]) in R)
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
            o = np.lexsort((v.aq, -v.av))[0]                 # the best prefix state: v descending, q ascending
            qs = self._walk(v, int(v.aq[o]), pos - 1, v.base)
            self._commit(v, qs[:F], out)
            v.status |= 1
        assert pos - v.base <= W - P
        v.attempts.append((pos, base0, c, F))


# ---- the automaton of the forced-commit tests
def two_components_automaton(N=6):
    """Two automata that never meet behind one start state that is never entered again: the labels below N/2 lead from the
    start into the states {1, 2} and loop among them, the other labels into {3, 4}, and no arc joins the halves.  The product
    graph has two disconnected components with start states in each; emissions that favour label 0 and label N/2 alike keep a
    hypothesis of each half in a beam of K >= 2 (`two_component_emissions`), and their ancestries never share a frame.
    -> next, weight, final of the automaton (start state 0)."""
    h = N // 2
    nxt = np.full((5, N), -1, np.int64)
    nxt[0, :h], nxt[1, :h], nxt[2, :h] = 1, 2, 1
    nxt[0, h:], nxt[3, h:], nxt[4, h:] = 3, 4, 3
    return nxt, np.zeros((5, N)), np.zeros(5)


def chain_automaton(S, N):
    """One chain walked DOWN from its last state: every token leads from s to s - 1.  The product states are sorted by automaton
    state, so a search from the start lives in the LAST product states.  -> next, weight, final, start."""
    nxt = np.repeat(np.arange(-1, S - 1)[:, None], N, 1)
    return nxt, np.log(np.random.default_rng(S).dirichlet(np.ones(N), size=S)), np.zeros(S), S - 1


def two_component_emissions(T, B, N, dtype, seed=5):
    """Label 0 and label N/2 ahead by 1 in every frame, the others at 0 (slot 0) or at 0 / 0.25 (the other slots): with zero
    transitions and a token score below zero the two best hypotheses are "stay on 0" and "stay on N/2", tied, one per half."""
    x = np.zeros((T, B, N), dtype)
    x[:, 1:] = np.random.default_rng(seed).integers(0, 2, size=(T, B - 1, N)) * 0.25
    x[:, :, 0] = x[:, :, N // 2] = 1.0
    return x
