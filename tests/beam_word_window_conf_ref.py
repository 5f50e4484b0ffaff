"""Test-only numpy restatement of the LATTICE-KEEPING word window stream (`torch_asg_amd.BeamWordWindowStream(...,
keep_lattice=True)`), written from the specification (include/asg_hip.h::asg_beam_word_conf_window_advance) BY DEFINITION and not
by ring: there is no ring of lattice rows, no attempt log and no resumed pull here.

The commits, the attempt positions and the carried walk are tests/beam_word_window_ref.py's (`BeamWordWindowRef`, or with `order`
the look-ahead window of tests/beam_word_la_stream_ref.py; what is added is the frame of the separator of every committed word).
The cell posteriors are tests/beam_word_stream_conf_ref.py's: a `BeamWordStreamConfRef` without a bound is fed the same frames,
slot by slot, up to the position p1 of a commit attempt, and its prefix-mode events {(word, frame): P} over the lattice A_0 ..
A_{p1-1} give every word the attempt commits its confidence, the sum over the frames f - tol .. f + tol clipped to 1 .. p1-1.  A
forced commit of the same attempt uses the same p1.  Everything in float64.  `ends` records, per slot, (p1, base before, first
word, one past the last word, status after) of every attempt that committed a word, for the tests.
"""
import numpy as np

from beam_word_la_stream_ref import BeamWordLaWindowRef
from beam_word_stream_conf_ref import BeamWordStreamConfRef
from beam_word_window_ref import BeamWordWindowRef


class _Conf:
    def _init_conf(self, transition, lexicon, lm, order, beam_size, beam_threshold, weights, dtype, frame_tolerance, max_chunk):
        self.tol = int(frame_tolerance)
        self.C = self.W if max_chunk is None else int(max_chunk)
        assert self.tol >= 0 and self.C >= 1
        # the growing stream of the same frames (no bound: its `result` is never called, only its lattice rows)
        self.g = BeamWordStreamConfRef(transition, lexicon, lm, self.B, 1 << 40, beam_size, beam_threshold, *weights, dtype=dtype,
                                       order=order)
        self._em = [[] for _ in range(self.B)]               # every frame a slot consumed since its reset, as it came
        self._par = [[] for _ in range(self.B)]              # ... and the (transition, threshold) it was searched with
        self.ends = [[] for _ in range(self.B)]

    def reset(self, mask=None):
        super().reset(mask)
        self.g.reset(mask)
        for b in range(self.B):
            if mask is None or mask[b]:
                self._em[b], self._par[b], self.ends[b] = [], [], []

    def _cells(self, b, upto, final):
        """-> (Z, {(word, frame): P}) of slot b over the lattice A_0 .. A_{upto-1}."""
        s = self.g.slots[b]
        assert s.pos <= upto <= len(self._em[b])
        if upto == 0:
            return -np.inf, {}
        with np.errstate(invalid="ignore", over="ignore"):
            while s.pos < upto:
                tr, theta = self._par[b][s.pos]
                self.g._frame(s, self._em[b][s.pos], tr, theta)
        tr64 = self._par[b][upto - 1][0].astype(np.float64)
        self.g._catch_up(s, tr64)
        return self.g._events(s, tr64, final)

    def _confidence(self, P, last, frame, word):
        return sum(P.get((word, t), 0.0) for t in range(max(1, frame - self.tol), min(last, frame + self.tol) + 1))

    def _separators(self, pairs, carry, first):
        """The absolute frames of the separators that end a word on the segment `pairs` behind the label `carry`."""
        s, out = self.s, []
        for i, (_, q) in enumerate(pairs):
            lab = int(s.label[q])
            if lab == s.sep and carry != s.sep and carry != -1:
                out.append(first + i)
            carry = lab
        return out

    def _commit(self, v, pairs, out):
        self._wf += self._separators(pairs, v.carry, v.base)
        super()._commit(v, pairs, out)

    def _attempt(self, v, out):
        b = [i for i, w in enumerate(self.slots) if w is v][0]
        p1, b0, k0 = v.pos, v.base, len(out[4])
        super()._attempt(v, out)
        k1 = len(out[4])
        assert len(self._wf) == k1
        if k1 == k0:
            return
        Z, P = self._cells(b, p1, False)
        for k in range(k0, k1):
            assert max(b0, 1) <= self._wf[k] < p1
            self._cf.append(self._confidence(P, p1 - 1, self._wf[k], out[4][k]) if Z > -np.inf else 0.0)
        self.ends[b].append((p1, b0, k0, k1, v.status))

    def advance(self, chunk, chunk_lengths=None, transition=None, beam_threshold=None):
        """-> the window restatement's eight, then new_word_frames int64 [B][W + Tc] (-1 behind the data) and
        new_word_confidences float64 [B][W + Tc] (0 behind the data)."""
        x = np.asarray(chunk)
        Tc, B, _ = x.shape
        assert Tc <= self.C, "a chunk longer than max_chunk"
        s = self.s
        tr = np.ascontiguousarray(np.asarray(s.transition if transition is None else transition), dtype=self.dt)
        theta = self.dt(s.beam_threshold if beam_threshold is None else beam_threshold)
        wf = np.full((B, self.W + Tc), -1, np.int64)
        cf = np.zeros((B, self.W + Tc))
        outs = []
        for b in range(B):                                   # one slot per pass (the others get no frame): its lists are its own
            n = Tc if chunk_lengths is None else int(min(max(int(chunk_lengths[b]), 0), Tc))
            self._em[b] += [np.array(x[t, b], self.dt) for t in range(n)]
            self._par[b] += [(tr, theta)] * n
            lens = np.zeros(B, np.int64)
            lens[b] = n
            self._wf, self._cf = [], []
            o = super().advance(x, lens, transition, beam_threshold)
            outs.append([a[b] for a in o])
            wf[b, :len(self._wf)] = self._wf
            cf[b, :len(self._cf)] = self._cf
        return tuple(np.stack([o[i] for o in outs]) for i in range(8)) + (wf, cf)

    def result_confidence(self, final=False):
        """-> dict with the fourteen fields of BeamWordWindowConfidence (confidences and normalisers float64)."""
        out = dict(self.result(final))
        B, W = self.B, self.W
        out.update(word_frames=np.full((B, W), -1, np.int64), word_confidences=np.zeros((B, W)), normalisers=np.full(B, -np.inf))
        for b, v in enumerate(self.slots):
            Z, P = self._cells(b, v.pos, final)
            out["normalisers"][b] = Z
            n = int(out["word_lengths"][b])
            if n == 0:
                continue
            live = v.pos - v.base
            f = []
            carry = v.carry
            for i, lab in enumerate(out["path"][b, :live]):   # the carried walk over the tail's labels
                if lab == self.s.sep and carry != self.s.sep and carry != -1:
                    f.append(v.base + i)
                carry = int(lab)
            f += [v.pos] * (n - len(f))                      # the word the final step closes
            assert len(f) == n and (final or f[-1] < v.pos)
            out["word_frames"][b, :n] = f
            if Z > -np.inf:
                last = v.pos if final else v.pos - 1
                out["word_confidences"][b, :n] = [self._confidence(P, last, f[k], int(out["words"][b, k])) for k in range(n)]
        return out


class _Plain(_Conf, BeamWordWindowRef):
    pass


class _Look(_Conf, BeamWordLaWindowRef):
    pass


def BeamWordWindowConfRef(transition, lexicon, lm, batch_size=1, window=1, commit_every=None, beam_size=1, beam_threshold=np.inf,
                          lm_weight=1.0, word_score=0.0, token_score=0.0, dtype=np.float32, frame_tolerance=0, max_chunk=None,
                          order=None):
    """The lattice-keeping window over the plain search, or over the look-ahead search of `order`."""
    w = (lm_weight, word_score, token_score)
    if order is None:
        s = _Plain(transition, lexicon, lm, batch_size, window, commit_every, beam_size, beam_threshold, *w, dtype)
    else:
        s = _Look(transition, lexicon, lm, order, batch_size, window, commit_every, beam_size, beam_threshold, *w, dtype)
    s._init_conf(transition, lexicon, lm, order, beam_size, beam_threshold, w, dtype, frame_tolerance, max_chunk)
    return s
