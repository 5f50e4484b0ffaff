"""Test-only float64 numpy restatement of the full score of the ASG lattice composed with a token automaton, its gradients and
the automaton's target score (`torch_asg_amd.graph_full_score`, `graph_asg_loss`), written from the spec and not from the
kernels.  Product graph and folding as in tests/graph_decode_ref.py.

    alpha[0][q] = start_w[q] + I[0][i];   alpha[t][q] = lse(alpha[t-1][q] + tr[i][i], {alpha[t-1][q'] + tr[i][j] + w_e}) + I[t][i]
    Z = lse_q(alpha[len-1][q] + final_w[q]);   beta the mirror image;   gamma_t(q) = exp(alpha[t][q] + beta[t][q] - Z)
    dZ/dI[t][b][i] = sum of gamma_t over the q of label i;   dZ/dtr[i][j] = sum over t >= 1 of the posteriors of the stays
    (i == j) and edges with that label pair.   A(y) = arcw[start][y1] + sum_k arcw[s_k][y_k+1] + finw[s_end] (-inf if rejected)
"""
import numpy as np

from graph_decode_ref import fold, product


def _lse(a, axis=None):
    a = np.asarray(a, np.float64)
    m = np.max(a, axis=axis, keepdims=True) if a.size else np.full((1,) * max(a.ndim, 1), -np.inf)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        r = np.log(np.sum(np.exp(a - ms), axis=axis, keepdims=True)) + ms
    r = np.where(m == -np.inf, -np.inf, r)
    return r.squeeze(axis) if axis is not None else float(r.reshape(-1)[0])


def _grouped_lse(cands, groups, Q):
    """lse of candidate values per group index (q), -inf for empty groups."""
    m = np.full(Q, -np.inf)
    np.maximum.at(m, groups, cands)
    ms = np.where(np.isfinite(m), m, 0.0)
    s = np.zeros(Q)
    np.add.at(s, groups, np.exp(cands - ms[groups]))
    with np.errstate(divide="ignore"):
        return np.where(m == -np.inf, -np.inf, np.log(s) + ms)


class Composed:
    """The composed lattice of one automaton in float64 (weights folded in `fold_dt`, then widened)."""

    def __init__(self, next_, weight, final, start=0, lm_weight=1.0, token_score=0.0, fold_dt=np.float64):
        nxt = np.asarray(next_, np.int64)
        present, arcw, finw = fold(nxt, weight, final, fold_dt, lm_weight, token_score)
        self.nxt, self.present, self.start = nxt, present, int(start)
        self.arcw, self.finw = arcw.astype(np.float64), finw.astype(np.float64)
        self.label, self.state, self.src, self.tgt, self.Q = product(nxt, present)
        Q = self.Q
        self.start_w = np.full(Q, -np.inf)
        for q in range(Q):
            i = self.label[q]
            if present[self.start, i] and nxt[self.start, i] == self.state[q]:
                self.start_w[q] = self.arcw[self.start, i]
        self.final_w = self.finw[self.state] if Q else np.zeros(0)
        self.edge_w = self.arcw[self.state[self.src], self.label[self.tgt]] if Q else np.zeros(0)

    def utterance(self, x, tr, L):
        """x [T,N], tr [N,N] float64, length L -> (Z, dZ/dx [T,N], dZ/dtr [N,N])."""
        T, N = x.shape
        Q, lab, src, tgt = self.Q, self.label, self.src, self.tgt
        gx, gtr = np.zeros((T, N)), np.zeros((N, N))
        if L == 0 or Q == 0:
            return -np.inf, gx, gtr
        stay = tr[lab, lab]
        etr = tr[lab[tgt], lab[src]]
        alpha = np.full((L, Q), -np.inf)
        alpha[0] = self.start_w + x[0, lab]
        for t in range(1, L):
            c = np.concatenate([alpha[t - 1] + stay, alpha[t - 1][src] + etr + self.edge_w])
            g = np.concatenate([np.arange(Q), tgt])
            alpha[t] = _grouped_lse(c, g, Q) + x[t, lab]
        Z = _lse(alpha[L - 1] + self.final_w)
        if Z == -np.inf:
            return Z, gx, gtr
        beta = np.full((L, Q), -np.inf)
        beta[L - 1] = self.final_w
        for t in range(L - 1, 0, -1):
            c = np.concatenate([beta[t] + stay + x[t, lab], beta[t][tgt] + etr + self.edge_w + x[t, lab[tgt]]])
            g = np.concatenate([np.arange(Q), src])
            beta[t - 1] = _grouped_lse(c, g, Q)
        with np.errstate(invalid="ignore"):
            gam = np.exp(alpha + beta - Z)
        gam = np.nan_to_num(gam)
        for t in range(L):
            np.add.at(gx[t], lab, gam[t])
        for t in range(1, L):
            ps = np.exp(alpha[t - 1] + stay + x[t, lab] + beta[t] - Z)
            np.add.at(gtr, (lab, lab), ps)
            pe = np.exp(alpha[t - 1][src] + etr + self.edge_w + x[t, lab[tgt]] + beta[t][tgt] - Z)
            np.add.at(gtr, (lab[tgt], lab[src]), pe)
        return Z, gx, gtr

    def target_score(self, y):
        """A(collapse(y)) in float64; -inf if rejected (or any label out of range)."""
        s, st, prev = 0.0, self.start, None
        N = self.nxt.shape[1]
        for v in y:
            v = int(v)
            if v == prev:
                continue
            if not 0 <= v < N or not self.present[st, v]:
                return -np.inf
            s += self.arcw[st, v]
            st = int(self.nxt[st, v])
            prev = v
        return s + self.finw[st]


def full_graph_ref(inputs, transition, next_, weight, final, start=0, input_lengths=None, lm_weight=1.0, token_score=0.0,
                   grad_scores=None, fold_dt=np.float64):
    """inputs [T,B,N] -> (Z [B], grad_inputs [T,B,N], grad_transition [N,N]) of sum_b grad_scores[b] * Z[b], in float64."""
    x = np.asarray(inputs, np.float64)
    tr = np.asarray(transition, np.float64)
    T, B, N = x.shape
    lens = np.full(B, T) if input_lengths is None else np.clip(np.asarray(input_lengths, np.int64), 0, T)
    g = np.ones(B) if grad_scores is None else np.asarray(grad_scores, np.float64)
    c = Composed(next_, weight, final, start, lm_weight, token_score, fold_dt)
    Z, gx, gtr = np.zeros(B), np.zeros((T, B, N)), np.zeros((N, N))
    for b in range(B):
        Z[b], gxb, gtb = c.utterance(x[:, b], tr, int(lens[b]))
        gx[:, b] = g[b] * gxb
        gtr += g[b] * gtb
    return Z, gx, gtr


def target_scores_ref(targets, target_lengths, next_, weight, final, start=0, lm_weight=1.0, token_score=0.0,
                      fold_dt=np.float64):
    c = Composed(next_, weight, final, start, lm_weight, token_score, fold_dt)
    tg = np.asarray(targets)
    S = tg.shape[1]
    tl = np.full(tg.shape[0], S) if target_lengths is None else np.clip(np.asarray(target_lengths), 0, S)
    return np.array([c.target_score(tg[b, :int(tl[b])]) for b in range(tg.shape[0])])
