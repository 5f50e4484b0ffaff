"""Test-only numpy restatement of the LATTICE-KEEPING beam stream (`torch_asg_amd.BeamStream(..., keep_lattice=True)`), written
from the specification (include/asg_hip.h::asg_beam_conf_stream_confidence) and not from the kernels.

The search, its carried state and `result` are tests/beam_stream_ref.py's `BeamStreamRef`; the events, the start frames and the
windows are tests/beam_conf_ref.py's (`token_events`, `start_frames`, `window_confidences`, by import).  What is added is the state
that the confidences need, explicit per slot: the kept emissions `em` (one row per consumed frame), `apos` (the frames whose
lattice rows are valid), and for every frame below apos the sorted set `U[t]` and the alpha row `alpha[t]`.  `result_confidence`
first catches the rows up from apos to pos -- resuming from row apos-1, never recomputing a row -- and then runs beta with the end
term of the mode: the final weight (final), or 0 in every kept state of the last set (prefix; added here, beam_conf_ref has no
such mode).  alpha, beta and every P(i, t) in float64 by token_events' formulas, in its order of operations, so that `final=True`
is beam_conf_ref's result byte for byte.  No tables and no ranks.
"""
import numpy as np

from beam_conf_ref import start_frames, token_events, window_confidences
from beam_stream_ref import BeamStreamRef
from graph_loss_ref import Composed, _grouped_lse, _lse


class BeamStreamConfRef(BeamStreamRef):
    def __init__(self, transition, next_, weight, final, start=0, batch_size=1, max_frames=1, beam_size=1, beam_threshold=np.inf,
                 lm_weight=1.0, token_score=0.0, dtype=np.float32):
        super().__init__(transition, next_, weight, final, start, batch_size, max_frames, beam_size, beam_threshold, lm_weight,
                         token_score, dtype)
        self.c = Composed(np.asarray(next_, np.int64), weight, final, start, lm_weight, token_score, fold_dt=self.dt)
        assert self.c.Q == self.Q and np.array_equal(self.c.label, self.label)
        for s in self.slots:
            self._fresh(s)

    @staticmethod
    def _fresh(s):
        s.em, s.apos, s.U, s.alpha = [], 0, [], []

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
        c = self.c
        Q, lab, src, tgt = c.Q, c.label, c.src, c.tgt
        stay = tr[lab, lab]
        etr = tr[lab[tgt], lab[src]]
        for t in range(s.apos, s.pos):
            U = np.sort(np.asarray(s.history[t][0], np.int64))
            mask = np.zeros(Q, bool)
            mask[U] = True
            x = s.em[t].astype(np.float64)
            if t == 0:
                a = np.where(mask, c.start_w + x[lab], -np.inf)
            else:
                prev = s.alpha[t - 1]
                cand = np.concatenate([prev + stay, prev[src] + etr + c.edge_w])
                a = np.where(mask, _grouped_lse(cand, np.concatenate([np.arange(Q), tgt]), Q) + x[lab], -np.inf)
            assert len(s.U) == t and len(s.alpha) == t       # a row is computed once
            s.U.append(U)
            s.alpha.append(a)
        s.apos = s.pos

    def _events(self, s, tr, final):
        """-> (Z, P [L,N]) of one slot from its stored rows; the end term is final_w (final) or 0 (prefix)."""
        c = self.c
        L, N = s.pos, len(tr)
        Q, lab, src, tgt = c.Q, c.label, c.src, c.tgt
        P = np.zeros((L, N))
        if L == 0 or Q == 0:
            return -np.inf, P
        x = np.stack(s.em).astype(np.float64)
        mask = np.zeros((L, Q), bool)
        for t in range(L):
            mask[t, s.U[t]] = True
        stay = tr[lab, lab]
        etr = tr[lab[tgt], lab[src]]
        alpha = s.alpha
        end = c.final_w if final else np.zeros(Q)
        with np.errstate(invalid="ignore"):
            Z = _lse(alpha[L - 1] + end) if final else _lse(alpha[L - 1])
        if Z == -np.inf:
            return Z, P
        beta = np.full((L, Q), -np.inf)
        beta[L - 1] = np.where(mask[L - 1], end, -np.inf)
        for t in range(L - 1, 0, -1):
            cand = np.concatenate([beta[t] + stay + x[t, lab], beta[t][tgt] + etr + c.edge_w + x[t, lab[tgt]]])
            beta[t - 1] = np.where(mask[t - 1], _grouped_lse(cand, np.concatenate([np.arange(Q), src]), Q), -np.inf)
        with np.errstate(invalid="ignore"):
            np.add.at(P[0], lab, np.nan_to_num(np.exp(alpha[0] + beta[0] - Z)))
            for t in range(1, L):
                pe = np.nan_to_num(np.exp(alpha[t - 1][src] + etr + c.edge_w + x[t, lab[tgt]] + beta[t][tgt] - Z))
                np.add.at(P[t], lab[tgt], pe)
        return Z, P

    def result_confidence(self, frame_tolerance=0, final=False, transition=None):
        """-> dict with the ten fields of BeamStreamConfidence (confidences and normalisers float64) and, per slot, `events`
        (P [pos,N]) and `sets`.  It writes apos, U and alpha and nothing else."""
        tol = int(frame_tolerance)
        assert 0 <= tol
        B, T = self.B, self.max_frames
        tr = np.asarray(self.transition if transition is None else transition).astype(self.dt).astype(np.float64)
        scores, path, tokens, token_lengths, states, frames, status = self.result(final)
        out = dict(scores=scores, path=path, tokens=tokens, token_lengths=token_lengths, states=states,
                   token_frames=np.full((B, T), -1, np.int64), token_confidences=np.zeros((B, T)), normalisers=np.full(B, -np.inf),
                   frames=frames, status=status, events=[], sets=[])
        for b, s in enumerate(self.slots):
            self._catch_up(s, tr)
            Z, P = self._events(s, tr, final)
            if final and s.pos:                              # the carried rows are the one-shot's rows
                Z1, P1 = token_events(self.c, np.stack(s.em).astype(np.float64), tr, s.pos, s.U)
                assert np.array_equal(Z, Z1) and np.array_equal(P, P1)
            out["normalisers"][b] = Z
            out["events"].append(P)
            out["sets"].append(list(s.U))
            n = int(token_lengths[b])
            if n:
                sf = start_frames(path[b, :s.pos])
                assert len(sf) == n and [int(path[b, t]) for t in sf] == [int(v) for v in tokens[b, :n]]
                out["token_frames"][b, :n] = sf
        out["token_confidences"] = window_confidences(out, frames, tol)
        return out
