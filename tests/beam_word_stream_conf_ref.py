"""Test-only numpy restatement of the LATTICE-KEEPING word-LM beam stream (`torch_asg_amd.BeamWordStream(..., keep_lattice=True)`),
written from the specification (include/asg_hip.h::asg_beam_word_conf_stream_confidence) and not from the kernels.

The search, its carried state and `result` are tests/beam_word_stream_ref.py's `BeamWordStreamRef` or, with `order`, the look-ahead
stream of tests/beam_word_la_stream_ref.py (`BeamWordLaStreamRef`); the model of a pair's edges and ends is
tests/beam_word_loss_ref.py's (`word_model`, plain weights, also behind a look-ahead search); the events of `final=True`, the
end frames and the window sums are tests/beam_word_conf_ref.py's (`word_events`, `hypothesis_frames`, by import).  What is added
is the state that the confidences need, explicit per slot: the kept emissions `em` (one row per consumed frame), `apos` (the
frames whose lattice rows are valid), and for every frame below apos the sorted set `U[t]`, the alpha row `alpha[t]` and the
edges into it.  `result_confidence` first catches the rows up from apos to pos -- resuming from row apos-1, never recomputing a
row -- and then runs beta with the end of the mode: the end rule (final), or 0 in every kept pair of the last set and no event
at frame L (prefix; added here, beam_word_conf_ref has no such mode).  alpha, beta and every P(w, t) in float64 by word_events'
formulas, in its order of operations, so that `final=True` is beam_word_conf_ref's result byte for byte.  No tables, no ranks.
"""
import numpy as np

from beam_word_conf_ref import hypothesis_frames, word_events
from beam_word_la_stream_ref import BeamWordLaStreamRef
from beam_word_loss_ref import _lse, word_model
from beam_word_stream_ref import NAMES, BeamWordStreamRef


class _LatticeKeeping:
    """The carried lattice state and `result_confidence`, over either search (mixed in in front of it)."""

    def _init_lattice(self, lexicon, lm, lm_weight, word_score, token_score):
        self.m = word_model(lexicon, lm, self.dt, lm_weight, word_score, token_score)
        assert self.m.Q == self.Q and np.array_equal(self.m.label, self.label)
        for s in self.slots:
            self._fresh(s)

    @staticmethod
    def _fresh(s):
        s.em, s.apos, s.U, s.alpha, s.edges = [], 0, [], [], []

    def reset(self, mask=None):
        super().reset(mask)
        for b, s in enumerate(self.slots):
            if mask is None or mask[b]:
                self._fresh(s)                               # apos goes back to 0 in the chosen slots only

    def _frame(self, s, xt, tr, theta):
        super()._frame(s, xt, tr, theta)
        s.em.append(np.array(xt, self.dt))                   # the frame's N emissions, as they came

    # ---- the lazy part: the lattice rows of the frames [apos, pos)
    def _catch_up(self, s, tr):
        m = self.m
        lab, start = m.label, int(m.lm.start)
        for t in range(s.apos, s.pos):
            U = [tuple(p) for p in s.kept[t]]                # the kept pairs of the frame, sorted: nothing is forced
            assert U == sorted(set(U)) and len(U) == s.sizes[t]
            x = s.em[t].astype(np.float64)
            if t == 0:
                a = {p: (m.start_w[p[1]] + x[lab[p[1]]] if p[0] == start else -np.inf) for p in U}
                ed = None
            else:
                prev = s.alpha[t - 1]
                inc = {p: [] for p in U}
                ed = []
                for p in s.U[t - 1]:
                    ap = prev[p]
                    for k, (p2, w, i) in enumerate(m.edges(p)):
                        if p2 in inc:
                            ed.append((p, p2, w, i, k > 0 and i == m.sep))   # (edge 0 is the stay: never a word's end)
                            if ap > -np.inf:
                                inc[p2].append((ap + tr[i, lab[p[1]]]) + w)
                a = {p: _lse(c) + x[lab[p[1]]] for p, c in inc.items()}
            assert len(s.U) == t and len(s.alpha) == t       # a row is computed once
            s.U.append(U)
            s.alpha.append(a)
            s.edges.append(ed)
        s.apos = s.pos

    def _events(self, s, tr, final):
        """-> (Z, {(word, frame): P}) of one slot from its stored rows; the end is the end rule (final) or 0 (prefix)."""
        m = self.m
        L, lab = s.pos, m.label
        if L == 0:
            return -np.inf, {}
        x = np.stack(s.em).astype(np.float64)
        U, alpha, edges = s.U, s.alpha, s.edges
        end = (lambda p: m.endw(p)) if final else (lambda p: 0.0)
        Z = _lse([alpha[L - 1][p] + end(p) for p in U[L - 1]])
        if Z == -np.inf:
            return Z, {}
        beta = [None] * L
        beta[L - 1] = {p: end(p) for p in U[L - 1]}
        for t in range(L - 1, 0, -1):
            out = {p: [] for p in U[t - 1]}
            for p, p2, w, i, _ in edges[t]:
                out[p].append(((beta[t][p2] + tr[i, lab[p[1]]]) + w) + x[t, i])
            beta[t - 1] = {p: _lse(c) for p, c in out.items()}
        P = {}
        for t in range(1, L):
            for p, p2, w, i, word_end in edges[t]:
                if not word_end:
                    continue
                v = alpha[t - 1][p] + tr[i, lab[p[1]]] + w + x[t, i] + beta[t][p2] - Z
                if v > -np.inf:
                    key = (int(m.wos[m.state[p[1]]]), t)
                    P[key] = P.get(key, 0.0) + np.exp(v)
        if final:                                            # the final step of the end rule; a prefix has none
            for p in U[L - 1]:
                st = int(m.state[p[1]])
                v = alpha[L - 1][p] + m.endw(p) - Z
                if st != 0 and v > -np.inf:
                    key = (int(m.wos[st]), L)
                    P[key] = P.get(key, 0.0) + np.exp(v)
        return Z, P

    def result_confidence(self, frame_tolerance=0, final=False, transition=None):
        """-> dict with the thirteen fields of BeamWordStreamConfidence (confidences and normalisers float64) and, per slot,
        `events` ({(word, frame): P}) and `sets`.  It writes apos, U, alpha and the edges and nothing else."""
        tol = int(frame_tolerance)
        assert 0 <= tol
        B, T = self.B, self.max_frames
        tr = np.asarray(self.transition if transition is None else transition).astype(self.dt).astype(np.float64)
        out = dict(self.result(final))
        assert set(out) == set(NAMES)
        out.update(word_frames=np.full((B, T), -1, np.int64), word_confidences=np.zeros((B, T)), normalisers=np.full(B, -np.inf),
                   events=[], sets=[])
        for b, s in enumerate(self.slots):
            self._catch_up(s, tr)
            L = s.pos
            Z, P = self._events(s, tr, final)
            if final and L:                                  # the carried rows are the one-shot's rows
                Z1, P1 = word_events(self.m, np.stack(s.em).astype(np.float64), tr, L, s.U)
                assert np.array_equal(Z, Z1) and P == P1
            assert all(1 <= t <= (L if final else L - 1) for _, t in P)
            out["normalisers"][b] = Z
            out["events"].append(P)
            out["sets"].append([list(u) for u in s.U])
            nw = int(out["word_lengths"][b])
            if nw == 0:
                continue
            frames = hypothesis_frames(out["path"][b], nw, L, self.m.sep)
            assert final or all(t < L for t in frames)       # a prefix counts the separator words only
            out["word_frames"][b, :nw] = frames
            for k, tk in enumerate(frames):
                w = int(out["words"][b, k])
                out["word_confidences"][b, k] = sum(P.get((w, t), 0.0) for t in range(max(1, tk - tol), min(L, tk + tol) + 1))
        return out


class _Plain(_LatticeKeeping, BeamWordStreamRef):
    pass


class _Look(_LatticeKeeping, BeamWordLaStreamRef):
    pass


def BeamWordStreamConfRef(transition, lexicon, lm, batch_size=1, max_frames=1, beam_size=1, beam_threshold=np.inf, lm_weight=1.0,
                          word_score=0.0, token_score=0.0, dtype=np.float32, order=None):
    """The lattice-keeping stream over the plain search, or over the look-ahead search of `order`."""
    if order is None:
        s = _Plain(transition, lexicon, lm, batch_size, max_frames, beam_size, beam_threshold, lm_weight, word_score, token_score,
                   dtype)
    else:
        s = _Look(transition, lexicon, lm, order, batch_size, max_frames, beam_size, beam_threshold, lm_weight, word_score,
                  token_score, dtype)
    s._init_lattice(lexicon, lm, lm_weight, word_score, token_score)
    return s
