"""float64 numpy restatement of the per-final-node scores of a target graph and their gradients
(include/asg_hip.h::asg_target_graph_final_forward): the scores from the definition's alpha; the gradients as
tests/target_graph_ref.py (alpha, beta) run once per final node with the other finals masked to -inf, weighted by g and summed
-- the beta formulation, not the kernels' linear reverse recursion."""
import numpy as np

from target_graph_ref import _lse, target_graph_ref

NI = -np.inf


def final_scores_ref(inputs, transition, graphs, input_lengths=None):
    """graphs: `TargetGraphs.graphs` -> final_scores [B,Kmax], -inf wherever the definition says so."""
    T, B, N = inputs.shape
    out = np.full((B, max(len(g[0]) for g in graphs)), NI)
    for b, (lab, sw, fw, src, dst, ew) in enumerate(graphs):
        K = len(lab)
        ln = T if input_lengths is None else int(np.clip(input_lengths[b], 0, T))
        if ln == 0 or K == 0:
            continue
        alpha = np.asarray(sw, np.float64) + inputs[0, b, lab]
        for t in range(1, ln):
            cand = [[alpha[k] + transition[lab[k], lab[k]]] for k in range(K)]
            for e in range(len(src)):
                cand[dst[e]].append(alpha[src[e]] + (transition[lab[dst[e]], lab[src[e]]] + ew[e]))
            alpha = np.array([_lse(c) for c in cand]) + inputs[t, b, lab]
        out[b, :K] = alpha + np.asarray(fw, np.float64)
    return out


def target_graph_final_ref(inputs, transition, graphs, input_lengths, grad):
    """-> final_scores [B,Kmax], grad_inputs [T,B,N], grad_transition [N,N] of sum grad * final_scores over the finite scores
    (grad is read nowhere else)."""
    T, B, N = inputs.shape
    fs = final_scores_ref(inputs, transition, graphs, input_lengths)
    gin, gtr = np.zeros((T, B, N)), np.zeros((N, N))
    for b, (lab, sw, fw, src, dst, ew) in enumerate(graphs):
        il = None if input_lengths is None else input_lengths[b:b + 1]
        for k in np.flatnonzero(fs[b] > NI):
            if grad[b, k] == 0:
                continue
            only = np.full(len(lab), NI)
            only[k] = fw[k]
            s, a, c = target_graph_ref(inputs[:, b:b + 1], transition, [(lab, sw, only, src, dst, ew)], il, grad[b, k:k + 1])
            assert abs(s[0] - fs[b, k]) <= 1e-9 * max(1.0, abs(s[0]))
            gin[:, b:b + 1] += a
            gtr += c
    return fs, gin, gtr


def risk_ref(alt_scores, costs):
    """[B] expected cost under the softmax of the finite alternative scores and its derivative by the scores [B,A]."""
    ok = np.isfinite(alt_scores)
    p = np.zeros_like(alt_scores)
    for b in range(len(p)):
        if ok[b].any():
            e = np.exp(alt_scores[b, ok[b]] - alt_scores[b, ok[b]].max())
            p[b, ok[b]] = e / e.sum()
    risk = (p * np.where(ok, costs, 0.0)).sum(1)
    return risk, p * (np.where(ok, costs, 0.0) - risk[:, None])
