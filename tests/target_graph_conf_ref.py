"""float64 numpy restatement of the target-graph confidences (include/asg_hip.h::asg_target_graph_confidence), written from the
definition with loops over t, k and edges.  The hypothesis is an argument, so a tie cannot make it speak of other tokens."""
import numpy as np

from target_graph_ref import _lse, target_graph_ref


def target_graph_conf_ref(inputs, transition, graphs, tokens, token_frames, token_lengths, input_lengths=None, tol=0):
    """graphs: `TargetGraphs.graphs` -> normalisers [B], token_confidences [B,T], final_posteriors [B,Kmax], P [B,N,T]."""
    T, B, N = inputs.shape
    tr = transition
    Z = target_graph_ref(inputs, tr, graphs, input_lengths)[0]
    conf, post, P = np.zeros((B, T)), np.zeros((B, max(len(g[0]) for g in graphs))), np.zeros((B, N, T))
    for b, (lab, sw, fw, src, dst, ew) in enumerate(graphs):
        if Z[b] == -np.inf:
            continue
        K, E, I = len(lab), len(src), inputs[:, b, :]
        ln = T if input_lengths is None else int(np.clip(input_lengths[b], 0, T))
        f = [tr[lab[dst[e]], lab[src[e]]] + ew[e] for e in range(E)]
        into, out = [[] for _ in range(K)], [[] for _ in range(K)]
        for e in range(E):
            into[dst[e]].append(e)
            out[src[e]].append(e)
        alpha, beta = np.full((ln, K), -np.inf), np.full((ln, K), -np.inf)
        alpha[0] = [sw[k] + I[0, lab[k]] for k in range(K)]
        for t in range(1, ln):
            for k in range(K):
                c = [alpha[t - 1, k] + tr[lab[k], lab[k]]] + [alpha[t - 1, src[e]] + f[e] for e in into[k]]
                alpha[t, k] = _lse(c) + I[t, lab[k]]
        beta[ln - 1] = fw
        for t in range(ln - 1, 0, -1):
            for k in range(K):
                c = [(beta[t, k] + tr[lab[k], lab[k]]) + I[t, lab[k]]]
                c += [(beta[t, dst[e]] + f[e]) + I[t, lab[dst[e]]] for e in out[k]]
                beta[t - 1, k] = _lse(c)
        for k in range(K):
            post[b, k] = np.exp((alpha[ln - 1, k] + fw[k]) - Z[b])
            P[b, lab[k], 0] += np.exp((alpha[0, k] + beta[0, k]) - Z[b])
        for t in range(1, ln):
            for e in range(E):
                k = dst[e]
                P[b, lab[k], t] += np.exp((alpha[t - 1, src[e]] + ((beta[t, k] + f[e]) + I[t, lab[k]])) - Z[b])
        for j in range(int(token_lengths[b])):
            s = int(token_frames[b][j])
            conf[b, j] = sum(P[b, int(tokens[b][j]), t] for t in range(max(s - tol, 0), min(s + tol, ln - 1) + 1))
    return Z, conf, post, P
