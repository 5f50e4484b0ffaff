"""Test-only numpy restatement of the LATTICE-KEEPING window stream (`torch_asg_amd.BeamWindowStream(..., keep_lattice=True)`),
written from the specification (include/asg_hip.h::asg_beam_conf_window_advance) BY DEFINITION and not by ring: there is no ring
of lattice rows, no attempt log and no resumed pull here.

The commits, the attempt positions and the carried collapse are tests/beam_window_ref.py's (`BeamWindowRef`; what is added to it
is the start frame of every committed token: the absolute frame at which the carried collapse kept its label).  The cell
posteriors are tests/beam_stream_conf_ref.py's: a `BeamStreamConfRef` without a bound is fed the same frames, slot by slot, up to
the position p1 of a commit attempt, and its prefix-mode events P [p1, N] over the lattice A_0 .. A_{p1-1} give every token the
attempt commits its confidence, P[f - tol .. f + tol clipped to 0 .. p1-1, label].sum().  A forced commit of the same attempt uses
the same p1.  `ends` records, per slot, (p1, base before, first token, one past the last token, status after) of every attempt
that committed a token, for the tests.
"""
import numpy as np

from beam_stream_conf_ref import BeamStreamConfRef
from beam_window_ref import BeamWindowRef


class BeamWindowConfRef(BeamWindowRef):
    def __init__(self, transition, next_, weight, final, start=0, batch_size=1, window=1, commit_every=None, beam_size=1,
                 beam_threshold=np.inf, lm_weight=1.0, token_score=0.0, dtype=np.float32, frame_tolerance=0, max_chunk=None):
        super().__init__(transition, next_, weight, final, start, batch_size, window, commit_every, beam_size, beam_threshold,
                         lm_weight, token_score, dtype)
        self.tol = int(frame_tolerance)
        self.C = self.W if max_chunk is None else int(max_chunk)
        assert self.tol >= 0 and self.C >= 1
        # the growing stream of the same frames (no bound: its `result` is never called, only its lattice rows)
        self.g = BeamStreamConfRef(transition, next_, weight, final, start, batch_size, 1 << 40, beam_size, beam_threshold, lm_weight,
                                   token_score, dtype)
        self._em = [[] for _ in range(self.B)]               # every frame a slot consumed since its reset, as it came
        self._par = [[] for _ in range(self.B)]              # ... and the (transition, threshold) it was searched with
        self.ends = [[] for _ in range(self.B)]

    def reset(self, mask=None):
        super().reset(mask)
        self.g.reset(mask)
        for b in range(self.B):
            if mask is None or mask[b]:
                self._em[b], self._par[b], self.ends[b] = [], [], []

    # ---- the growing stream of slot b at position `upto`, with its lattice rows
    def _grown(self, b, upto):
        s = self.g.slots[b]
        assert s.pos <= upto <= len(self._em[b])
        with np.errstate(invalid="ignore", over="ignore"):
            while s.pos < upto:
                tr, theta = self._par[b][s.pos]
                self.g._frame(s, self._em[b][s.pos], tr, theta)
        tr64 = self._par[b][upto - 1][0].astype(np.float64) if upto else None
        if upto:
            self.g._catch_up(s, tr64)
        return s, tr64

    def _cells(self, b, upto, final):
        """-> (Z, P [upto, N]) of slot b over the lattice A_0 .. A_{upto-1}."""
        s, tr64 = self._grown(b, upto)
        if upto == 0:
            return -np.inf, np.zeros((0, 0))
        return self.g._events(s, tr64, final)

    def _confidence(self, P, L, frame, label):
        lo, hi = max(0, frame - self.tol), min(L - 1, frame + self.tol)
        return P[lo:hi + 1, label].sum()

    # ---- the commit, with start frames
    def _commit(self, v, qs, out):
        carry = v.carry
        for i, q in enumerate(qs):
            lab = int(self.s.label[q])
            if lab != carry:
                self._tf.append(v.base + i)
            carry = lab
        super()._commit(v, qs, out)

    def _attempt(self, v, out):
        b = [i for i, w in enumerate(self.slots) if w is v][0]
        p1, b0, k0 = v.pos, v.base, len(out[2])
        super()._attempt(v, out)
        k1 = len(out[2])
        assert len(self._tf) == k1
        if k1 == k0:
            return
        Z, P = self._cells(b, p1, False)
        for k in range(k0, k1):
            assert b0 <= self._tf[k] < p1
            self._cf.append(self._confidence(P, p1, self._tf[k], out[2][k]) if Z > -np.inf else 0.0)
        self.ends[b].append((p1, b0, k0, k1, v.status))

    # ---- the entry points
    def advance(self, chunk, chunk_lengths=None, transition=None, beam_threshold=None):
        """-> BeamWindowRef.advance's five, then new_token_frames int64 [B][W + Tc] (-1 behind the data) and
        new_token_confidences float64 [B][W + Tc] (0 behind the data)."""
        x = np.asarray(chunk)
        Tc, B, N = x.shape
        assert Tc <= self.C, "a chunk longer than max_chunk"
        s = self.s
        tr = np.ascontiguousarray(np.asarray(s.transition if transition is None else transition), dtype=self.dt)
        theta = self.dt(s.beam_threshold if beam_threshold is None else beam_threshold)
        tf = np.full((B, self.W + Tc), -1, np.int64)
        cf = np.zeros((B, self.W + Tc))
        outs = []
        for b in range(B):                                   # slot by slot, so that an attempt knows its slot's lists
            n = Tc if chunk_lengths is None else int(min(max(int(chunk_lengths[b]), 0), Tc))
            self._em[b] += [np.array(x[t, b], self.dt) for t in range(n)]
            self._par[b] += [(tr, theta)] * n
        for b in range(B):                                   # one slot per pass (the others get no frame): its lists are its own
            lens = np.zeros(B, np.int64)
            lens[b] = Tc if chunk_lengths is None else int(chunk_lengths[b])
            self._tf, self._cf = [], []
            o = BeamWindowRef.advance(self, x, lens, transition, beam_threshold)
            outs.append([a[b] for a in o])
            tf[b, :len(self._tf)] = self._tf
            cf[b, :len(self._cf)] = self._cf
        five = tuple(np.stack([o[i] for o in outs]) for i in range(5))
        return five + (tf, cf)

    def result_confidence(self, final=False):
        """-> dict with the eleven fields of BeamWindowConfidence (confidences and normalisers float64)."""
        scores, path, tokens, token_lengths, states, frames, committed, status = self.result(final)
        B, W = self.B, self.W
        out = dict(scores=scores, path=path, tokens=tokens, token_lengths=token_lengths, states=states,
                   token_frames=np.full((B, W), -1, np.int64), token_confidences=np.zeros((B, W)), normalisers=np.full(B, -np.inf),
                   frames=frames, committed=committed, status=status)
        for b, v in enumerate(self.slots):
            Z, P = self._cells(b, v.pos, final)
            out["normalisers"][b] = Z
            n = int(token_lengths[b])
            if n == 0:
                continue
            lab = path[b, :v.pos - v.base]
            prev = np.concatenate([[v.carry], lab[:-1]])
            f = v.base + np.nonzero(lab != prev)[0]
            assert len(f) == n
            out["token_frames"][b, :n] = f
            if Z > -np.inf:
                out["token_confidences"][b, :n] = [self._confidence(P, v.pos, int(f[k]), int(tokens[b, k])) for k in range(n)]
        return out
