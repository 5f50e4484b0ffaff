"""numpy restatement of the n best paths of a target graph, one per final node (include/asg_hip.h::asg_target_graph_nbest),
written from the definition with loops over t, k and edges, in the dtype it is given: adds and compares only, so a kernel
that follows the definition agrees with it bit for bit.  The forward restates tests/target_graph_viterbi_ref.py's (that
function returns neither v nor bp)."""
import numpy as np

FIELDS = ("num_hyps", "scores", "end_nodes", "emission_scores", "tokens", "token_frames", "token_lengths", "nodes", "labels")


def target_graph_nbest_ref(inputs, transition, graphs, input_lengths=None, nbest=10):
    """graphs: `TargetGraphs.graphs` (edges in incoming-CSR order) -> the arrays of FIELDS, in that order."""
    T, B, N = inputs.shape
    dt = inputs.dtype.type
    tr = transition.astype(dt)
    num = np.zeros(B, np.int64)
    scores, emis = (np.full((B, nbest), -np.inf, dt) for _ in range(2))
    ends = np.full((B, nbest), -1, np.int64)
    tokens, frames, nodes, labels = (np.full((B, nbest, T), -1, np.int64) for _ in range(4))
    lengths = np.zeros((B, nbest), np.int64)
    for b, (lab, sw, fw, src, dst, ew) in enumerate(graphs):
        K, E = len(lab), len(src)
        ln = T if input_lengths is None else int(np.clip(input_lengths[b], 0, T))
        if ln == 0 or K == 0:
            continue
        I = inputs[:, b, :]
        f = [tr[lab[dst[e]], lab[src[e]]] + dt(ew[e]) for e in range(E)]
        into = [[] for _ in range(K)]
        for e in range(E):                                                       # ascending e: ascending source within a target
            into[dst[e]].append(e)
        v = np.array([dt(sw[k]) + I[0, lab[k]] for k in range(K)], dt)
        bp = np.zeros((ln, K), np.int64)
        for t in range(1, ln):
            nv = np.empty(K, dt)
            for k in range(K):
                best, bp[t, k] = v[k] + tr[lab[k], lab[k]], k
                for e in into[k]:
                    c = v[src[e]] + f[e]
                    if c > best:
                        best, bp[t, k] = c, src[e]
                nv[k] = best + I[t, lab[k]]
            v = nv
        end = v + np.array(fw, dt)
        cand = sorted((k for k in range(K) if end[k] > -np.inf), key=lambda k: (-end[k], k))[:nbest]
        num[b] = len(cand)
        for r, k in enumerate(cand):
            ends[b, r], scores[b, r] = k, end[k]
            nd = nodes[b, r]
            nd[ln - 1] = k
            for t in range(ln - 1, 0, -1):
                nd[t - 1] = bp[t, nd[t]]
            lb = labels[b, r]
            lb[:ln] = np.asarray(lab)[nd[:ln]]
            at = [t for t in range(ln) if t == 0 or nd[t] != nd[t - 1]]
            lengths[b, r] = len(at)
            tokens[b, r, :len(at)], frames[b, r, :len(at)] = lb[at], at
            a = I[0, lb[0]]
            for t in range(1, ln):
                a = (a + tr[lb[t], lb[t - 1]]) + I[t, lb[t]]
            emis[b, r] = a
    return num, scores, ends, emis, tokens, frames, lengths, nodes, labels
