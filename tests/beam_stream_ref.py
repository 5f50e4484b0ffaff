"""Test-only numpy restatement of STREAMING beam decoding (`torch_asg_amd.BeamStream`), written from the specification
(include/asg_hip.h::asg_beam_stream_advance) and not from the package.  Folding and product states are those of
tests/graph_decode_ref.py (`fold`, `product`).

The state that is carried from chunk to chunk is explicit, per slot: `pos` (frames consumed), the active set `aq` with its values
`av`, the `history` of (active states, their sources) of every consumed frame, the sticky `overflow` word -- and, for the tests,
`sizes`, the |A_t| of every consumed frame.  `reset` / `advance` / `result(final)` are the three entry points.  A frame never
looks at anything but the stored set and its own emissions: frame 0 of an utterance takes its candidates from the start weights,
every other frame -- the first of a chunk included -- from the stored set.  All arithmetic in the dtype of the stream, in the
kernels' order: stay v + tr[i][i]; move (v + tr[i][j]) + arcw; then + emission.
"""
import numpy as np

from graph_decode_ref import fold, product


class _Slot:
    def __init__(self):
        self.pos, self.overflow = 0, 0
        self.aq, self.av = np.zeros(0, np.int64), None
        self.history, self.sizes = [], []


class BeamStreamRef:
    def __init__(self, transition, next_, weight, final, start=0, batch_size=1, max_frames=1, beam_size=1, beam_threshold=np.inf,
                 lm_weight=1.0, token_score=0.0, dtype=np.float32):
        self.dt = dt = np.dtype(dtype).type
        self.B, self.max_frames, self.K = int(batch_size), int(max_frames), int(beam_size)
        assert self.B >= 1 and self.max_frames >= 1 and self.K >= 1
        self.transition, self.beam_threshold = transition, beam_threshold
        nxt = np.asarray(next_, np.int64)
        present, arcw, self.finw = fold(nxt, weight, final, dt, lm_weight, token_score)
        self.label, self.state, src, tgt, self.Q = product(nxt, present)
        label, state, Q = self.label, self.state, self.Q
        self.ninf = dt(-np.inf)
        if Q:
            self.start_w = np.where(present[start, label] & (nxt[start, label] == state), arcw[start, label], self.ninf).astype(dt)
            order = np.lexsort((tgt, src))                   # the edges from the source side
            self.osrc, self.otgt = src[order], tgt[order]
            self.orow = np.zeros(Q + 1, np.int64)
            np.cumsum(np.bincount(self.osrc, minlength=Q), out=self.orow[1:])
            self.ow = arcw[state[self.osrc], label[self.otgt]]
        self.slots = [_Slot() for _ in range(self.B)]

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
        scores = np.full(B, -np.inf, dt)
        path = np.full((B, T), -1, np.int64)
        tokens = np.full((B, T), -1, np.int64)
        token_lengths = np.zeros(B, np.int64)
        states = np.full((B, T), -1, np.int64)
        frames = np.array([s.pos for s in self.slots], np.int64)
        status = np.array([s.overflow for s in self.slots], np.int64)
        for b, s in enumerate(self.slots):
            L = s.pos
            if L == 0 or s.aq.size == 0:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                end = s.av + self.finw[self.state[s.aq]] if final else s.av
            o = np.lexsort((s.aq, -end))[0]                  # end descending, q ascending
            if not end[o] > self.ninf:
                continue
            scores[b] = end[o]
            q = int(s.aq[o])
            for t in range(L - 1, -1, -1):
                path[b, t], states[b, t] = self.label[q], self.state[q]
                if t >= 1:
                    fq, fs = s.history[t]
                    q = int(fs[np.nonzero(fq == q)[0][0]])
            p = path[b, :L]
            keep = np.ones(L, bool)
            keep[1:] = p[1:] != p[:-1]
            tk = p[keep]
            tokens[b, :len(tk)] = tk
            token_lengths[b] = len(tk)
        return scores, path, tokens, token_lengths, states, frames, status

    def sizes(self):
        """Per slot the list of |A_t| of the frames consumed so far."""
        return [list(s.sizes) for s in self.slots]

    # ---- one frame of one slot
    def _prune(self, q, c, theta):
        """candidate states q with values c -> the active set (q, c) and the positions kept."""
        idx = np.nonzero(c > self.ninf)[0]
        q, c = q[idx], c[idx]
        if q.size == 0:
            return q, c, idx
        lo = c.max() - theta
        rank = np.lexsort((q, -c))[:self.K]                  # c descending, q ascending
        rank = rank[c[rank] >= lo]
        return q[rank], c[rank], idx[rank]

    def _frame(self, s, xt, tr, theta):
        label = self.label
        if self.Q == 0:
            s.aq, s.av = np.zeros(0, np.int64), np.zeros(0, self.dt)
            src = None
        elif s.pos == 0:
            s.aq, s.av, _ = self._prune(np.arange(self.Q), self.start_w + xt[label], theta)
            src = None
        elif s.aq.size == 0:                                 # an empty set stays empty
            src = s.aq
        else:
            aq, av, orow = s.aq, s.av, self.orow
            cnt = orow[aq + 1] - orow[aq]
            k_of = np.repeat(np.arange(aq.size), cnt)
            e = orow[aq][k_of] + (np.arange(k_of.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))
            ct = np.concatenate([aq, self.otgt[e]])
            cs = np.concatenate([aq, aq[k_of]])
            cv = np.concatenate([av + tr[label[aq], label[aq]], (av[k_of] + tr[label[self.otgt[e]], label[aq[k_of]]]) + self.ow[e]])
            o = np.lexsort((cs, -cv, ct))                    # per target: value descending, source ascending
            ct, cs, cv = ct[o], cs[o], cv[o]
            first = np.ones(ct.size, bool)
            first[1:] = ct[1:] != ct[:-1]
            bt, bsrc, bv = ct[first], cs[first], cv[first]
            s.aq, s.av, kept = self._prune(bt, bv + xt[label[bt]], theta)
            src = bsrc[kept]
        s.history.append((s.aq, src))
        s.sizes.append(int(s.aq.size))
        s.pos += 1
