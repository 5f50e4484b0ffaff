"""float64 numpy restatement of the target-graph score and its gradients (include/asg_hip.h::asg_target_graphs), written from
the definition with loops over t, k and edges and an explicit beta pass -- not from the kernels."""
import numpy as np


def _lse(c):
    m = max(c)
    return -np.inf if m == -np.inf else m + np.log(sum(np.exp(x - m) for x in c))


def target_graph_ref(inputs, transition, graphs, input_lengths=None, grad_scores=None):
    """graphs: `TargetGraphs.graphs` (edges in incoming-CSR order) -> scores [B], grad_inputs [T,B,N], grad_transition [N,N]."""
    T, B, N = inputs.shape
    tr = transition
    scores = np.full(B, -np.inf)
    gin, gtr = np.zeros((T, B, N)), np.zeros((N, N))
    with np.errstate(invalid="ignore"):
        for b, (lab, sw, fw, src, dst, ew) in enumerate(graphs):
            K, E = len(lab), len(src)
            ln = T if input_lengths is None else int(np.clip(input_lengths[b], 0, T))
            if ln == 0 or K == 0:
                continue
            I = inputs[:, b, :]
            f = [tr[lab[dst[e]], lab[src[e]]] + ew[e] for e in range(E)]
            into, out = [[] for _ in range(K)], [[] for _ in range(K)]
            for e in range(E):                        # (ascending e: by source within a target, by target within a source)
                into[dst[e]].append(e)
                out[src[e]].append(e)
            alpha = np.full((ln, K), -np.inf)
            for k in range(K):
                alpha[0, k] = sw[k] + I[0, lab[k]]
            for t in range(1, ln):
                for k in range(K):
                    c = [alpha[t - 1, k] + tr[lab[k], lab[k]]] + [alpha[t - 1, src[e]] + f[e] for e in into[k]]
                    alpha[t, k] = _lse(c) + I[t, lab[k]]
            Z = _lse([alpha[ln - 1, k] + fw[k] for k in range(K)])
            scores[b] = Z
            if Z == -np.inf:
                continue
            g = 1.0 if grad_scores is None else grad_scores[b]
            beta = np.full((ln, K), -np.inf)
            beta[ln - 1] = fw
            for t in range(ln - 1, 0, -1):
                for k in range(K):
                    stay = (beta[t, k] + tr[lab[k], lab[k]]) + I[t, lab[k]]
                    cs = [(beta[t, dst[e]] + f[e]) + I[t, lab[dst[e]]] for e in out[k]]
                    beta[t - 1, k] = _lse([stay] + cs)
                    gtr[lab[k], lab[k]] += g * np.exp((alpha[t - 1, k] + stay) - Z)
                    for e, c in zip(out[k], cs):
                        gtr[lab[dst[e]], lab[k]] += g * np.exp((alpha[t - 1, k] + c) - Z)
            for t in range(ln):
                for k in range(K):
                    gin[t, b, lab[k]] += g * np.exp((alpha[t, k] + beta[t, k]) - Z)
    return scores, gin, gtr
