"""numpy restatement of the best path of a target graph (include/asg_hip.h::asg_target_graph_viterbi), written from the
definition with loops over t, k and edges, in the dtype it is given: adds and compares only, so a kernel that follows the
definition agrees with it bit for bit."""
import numpy as np

from torch_asg_amd import TargetGraphs

NI = -np.inf


def target_graph_viterbi_ref(inputs, transition, graphs, input_lengths=None, edges_win_ties=False):
    """graphs: `TargetGraphs.graphs` (edges in incoming-CSR order) -> scores [B], nodes, labels, tokens, token_frames [B,T],
    token_lengths [B].  `edges_win_ties`: the rule the definition does NOT have (>= in place of >), to show that ties bite."""
    T, B, N = inputs.shape
    dt = inputs.dtype.type
    tr = transition.astype(dt)
    scores = np.full(B, -np.inf, dt)
    nodes, labels, tokens, frames = (np.full((B, T), -1, np.int64) for _ in range(4))
    lengths = np.zeros(B, np.int64)
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
                    if c > best or (edges_win_ties and c >= best):
                        best, bp[t, k] = c, src[e]
                nv[k] = best + I[t, lab[k]]
            v = nv
        end = v + np.array(fw, dt)
        scores[b] = end.max()
        if scores[b] == -np.inf:
            continue
        nodes[b, ln - 1] = int(np.argmax(end))                                  # the lowest k that attains the maximum
        for t in range(ln - 1, 0, -1):
            nodes[b, t - 1] = bp[t, nodes[b, t]]
        labels[b, :ln] = np.asarray(lab)[nodes[b, :ln]]
        at = [t for t in range(ln) if t == 0 or nodes[b, t] != nodes[b, t - 1]]
        lengths[b] = len(at)
        tokens[b, :len(at)], frames[b, :len(at)] = labels[b, at], at
    return scores, nodes, labels, tokens, frames, lengths


def tie_case(T, seed, alts=((0, 1, 2, 3), (0, 1, 3), (0, 2, 1), (2, 0, 1, 3))):
    """Integer emissions in {-2..2} and transitions in {-1, 0, 1}, all weights 0: a 4-alternative prefix tree with shared
    prefixes and the diamond (one label on both branches).  Sums of small integers are exact in either dtype: real ties."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, (T, 2, 4)).astype(np.float64)
    tr = rng.integers(-1, 2, (4, 4)).astype(np.float64)
    tree = TargetGraphs.from_alternatives([[list(a) for a in alts]], 4).graphs[0]
    spec = [(tree[0], tree[1], tree[2], list(zip(*tree[3:]))), ([0, 1, 1, 2], [0, NI, NI, NI], [NI, NI, NI, 0],
                                                                 [(0, 1, 0.0), (0, 2, 0.0), (1, 3, 0.0), (2, 3, 0.0)])]
    return x, tr, TargetGraphs(*[[s[n] for s in spec] for n in range(4)], 4)
