"""Test-only numpy restatement of the token confidences and start frames of the token-graph beam decoder
(`torch_asg_amd.beam_decode_graph_confidence`), written from the specification (include/asg_hip.h::asg_beam_graph_confidence)
and not from the kernels.  The sets come from beam_loss_ref.search (the search in the dtype of the emissions), the edges and the
ends from graph_loss_ref.Composed (the model beam_loss_ref.lattice sums over), the hypothesis from beam_decode_ref; alpha, beta and
every P(i, t) are computed by the formula in float64.  No tables and no ranks.
"""
import numpy as np

from beam_decode_ref import beam_decode_ref
from beam_loss_ref import search
from graph_decode_ref import _clamped_lengths
from graph_loss_ref import Composed, _grouped_lse, _lse


def token_events(c, x, tr, L, U):
    """One utterance: c a Composed, x [T,N] and tr [N,N] float64, U the list of its L kept sets -> (Z_K, P [L,N]) with
    P[t, i] the posterior of "a token with label i starts at frame t" (zeros when Z_K is -inf)."""
    N = x.shape[1]
    Q, lab, src, tgt = c.Q, c.label, c.src, c.tgt
    P = np.zeros((L, N))
    if L == 0 or Q == 0:
        return -np.inf, P
    mask = np.zeros((L, Q), bool)
    for t in range(L):
        mask[t, U[t]] = True
    stay = tr[lab, lab]
    etr = tr[lab[tgt], lab[src]]
    alpha = np.full((L, Q), -np.inf)
    alpha[0] = np.where(mask[0], c.start_w + x[0, lab], -np.inf)
    for t in range(1, L):
        cand = np.concatenate([alpha[t - 1] + stay, alpha[t - 1][src] + etr + c.edge_w])
        alpha[t] = np.where(mask[t], _grouped_lse(cand, np.concatenate([np.arange(Q), tgt]), Q) + x[t, lab], -np.inf)
    Z = _lse(alpha[L - 1] + c.final_w)
    if Z == -np.inf:
        return Z, P
    beta = np.full((L, Q), -np.inf)
    beta[L - 1] = np.where(mask[L - 1], c.final_w, -np.inf)
    for t in range(L - 1, 0, -1):
        cand = np.concatenate([beta[t] + stay + x[t, lab], beta[t][tgt] + etr + c.edge_w + x[t, lab[tgt]]])
        beta[t - 1] = np.where(mask[t - 1], _grouped_lse(cand, np.concatenate([np.arange(Q), src]), Q), -np.inf)
    with np.errstate(invalid="ignore"):
        np.add.at(P[0], lab, np.nan_to_num(np.exp(alpha[0] + beta[0] - Z)))
        for t in range(1, L):
            pe = np.nan_to_num(np.exp(alpha[t - 1][src] + etr + c.edge_w + x[t, lab[tgt]] + beta[t][tgt] - Z))
            np.add.at(P[t], lab[tgt], pe)
    return Z, P


def start_frames(path):
    """The first frame of every run of a label path."""
    return [t for t in range(len(path)) if t == 0 or path[t] != path[t - 1]]


def window_confidences(out, input_lengths, tol):
    """The token_confidences [B,T] of a `beam_conf_ref` result at another frame_tolerance (the events do not depend on it)."""
    B, T = out["token_frames"].shape
    lens = _clamped_lengths(input_lengths, T, B)
    conf = np.zeros((B, T))
    for b in range(B):
        L, P = int(lens[b]), out["events"][b]
        for k in range(int(out["token_lengths"][b])):
            s = int(out["token_frames"][b, k])
            conf[b, k] = P[max(0, s - tol):min(L - 1, s + tol) + 1, int(out["tokens"][b, k])].sum()
    return conf


def beam_conf_ref(inputs, transition, next_, weight, final, start=0, input_lengths=None, beam_size=1, beam_threshold=np.inf,
                  lm_weight=1.0, token_score=0.0, frame_tolerance=0):
    """inputs [T,B,N] (their dtype is the search's dtype) -> dict with the eight outputs of the call (scores in the dtype of the
    emissions, confidences and normalisers float64) and, per utterance, `events` (P [len,N]), `sets` and `sizes`."""
    xs = np.asarray(inputs)
    dt = xs.dtype.type
    T, B, N = xs.shape
    tol = int(frame_tolerance)
    nxt = np.asarray(next_, np.int64)
    lens = _clamped_lengths(input_lengths, T, B)
    scores, path, tokens, token_lengths, states = beam_decode_ref(xs, transition, nxt, weight, final, start, input_lengths,
                                                                  beam_size, beam_threshold, lm_weight, token_score)
    c = Composed(nxt, weight, final, start, lm_weight, token_score, fold_dt=dt)
    x = xs.astype(np.float64)
    tr = np.asarray(transition).astype(dt).astype(np.float64)
    out = dict(scores=scores, path=path, tokens=tokens, token_lengths=token_lengths, states=states,
               token_frames=np.full((B, T), -1, np.int64), token_confidences=np.zeros((B, T)), normalisers=np.full(B, -np.inf),
               events=[], sets=[], sizes=[])
    cache = {}
    for b in range(B):
        L = int(lens[b])
        r = search(xs[:, b], np.asarray(transition).astype(dt), nxt, weight, final, start, L, int(beam_size), beam_threshold,
                   lm_weight, token_score, cache)
        Z, P = token_events(c, x[:, b], tr, L, r["sets"])
        out["normalisers"][b] = Z
        out["events"].append(P)
        out["sets"].append(r["sets"])
        out["sizes"].append(r["sizes"])
        n = int(token_lengths[b])
        if n == 0:
            continue
        s = start_frames(path[b, :L])
        assert len(s) == n and [int(path[b, t]) for t in s] == [int(v) for v in tokens[b, :n]]
        out["token_frames"][b, :n] = s
        for k in range(n):
            lo, hi = max(0, s[k] - tol), min(L - 1, s[k] + tol)
            out["token_confidences"][b, k] = P[lo:hi + 1, int(tokens[b, k])].sum()
    return out
