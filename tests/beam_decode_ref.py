"""Test-only numpy restatement of beam-pruned Viterbi decoding over the ASG lattice composed with a token automaton
(`torch_asg_amd.beam_decode_graph`), written from the specification (include/asg_hip.h::asg_beam_decode_graph) and not from the
package.  Folding and product states are those of tests/graph_decode_ref.py (`fold`, `product`).

Per utterance and frame, vectorised over the candidates: the candidates of frame t come only from the active set of frame t-1
(the stay of an active q, whose source is q, and every edge out of an active q'); a target keeps its largest candidate, the
smallest source on a tie; c = best + emission; states with c = -inf are dropped; with m = max c and lo = fl(m - threshold) the new
active set is the first K states in (c descending, q ascending) order that have c >= lo.  All arithmetic in the dtype of the
emissions, in the kernels' order: stay v + tr[i][i]; move (v + tr[i][j]) + arcw; then + emission.
"""
import numpy as np

from graph_decode_ref import _clamped_lengths, fold, product


def beam_decode_ref(inputs, transition, next_, weight, final, start=0, input_lengths=None, beam_size=1, beam_threshold=np.inf,
                    lm_weight=1.0, token_score=0.0, sizes=None):
    """inputs [T,B,N], transition [N,N], the automaton -> scores [B], path, tokens [B,T], token_lengths [B], states [B,T] as
    `decode_graph_ref`.  `sizes`, if a list, receives per utterance the list of |A_t|."""
    x = np.asarray(inputs)
    T, B, N = x.shape
    dt = x.dtype.type
    K = int(beam_size)
    theta = dt(beam_threshold)
    assert K >= 1 and theta >= 0
    tr = np.ascontiguousarray(np.asarray(transition), dtype=dt)
    nxt = np.asarray(next_, np.int64)
    present, arcw, finw = fold(nxt, weight, final, dt, lm_weight, token_score)
    label, state, src, tgt, Q = product(nxt, present)
    lens = _clamped_lengths(input_lengths, T, B)
    scores = np.full(B, -np.inf, dt)
    path = np.full((B, T), -1, np.int64)
    tokens = np.full((B, T), -1, np.int64)
    token_lengths = np.zeros(B, np.int64)
    states = np.full((B, T), -1, np.int64)
    if T == 0 or Q == 0:
        return scores, path, tokens, token_lengths, states
    ninf = dt(-np.inf)
    start_w = np.where(present[start, label] & (nxt[start, label] == state), arcw[start, label], ninf).astype(dt)
    # the edges from the source side
    order = np.lexsort((tgt, src))
    osrc, otgt = src[order], tgt[order]
    orow = np.zeros(Q + 1, np.int64)
    np.cumsum(np.bincount(osrc, minlength=Q), out=orow[1:])
    otr = tr[label[otgt], label[osrc]]
    ow = arcw[state[osrc], label[otgt]]
    stay_tr = tr[label, label]

    def prune(q, c):
        """candidate states q with values c -> the active set (q, c, positions kept)."""
        ok = c > ninf
        idx = np.nonzero(ok)[0]
        q, c = q[idx], c[idx]
        if q.size == 0:
            return q, c, idx
        lo = c.max() - theta
        rank = np.lexsort((q, -c))                       # c descending, q ascending
        rank = rank[:K]
        rank = rank[c[rank] >= lo]
        return q[rank], c[rank], idx[rank]

    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            L = int(lens[b])
            if L == 0:
                continue
            xb = x[:, b]
            q0 = np.arange(Q)
            aq, av, _ = prune(q0, start_w + xb[0, label])
            hist = [(aq, None)]                               # per frame: active states, their sources
            nact = [aq.size]
            for t in range(1, L):
                if aq.size == 0:
                    hist.append((aq, aq))
                    nact.append(0)
                    continue
                cnt = orow[aq + 1] - orow[aq]
                k_of = np.repeat(np.arange(aq.size), cnt)
                e = orow[aq][k_of] + (np.arange(k_of.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))
                ct = np.concatenate([aq, otgt[e]])
                cs = np.concatenate([aq, aq[k_of]])
                cv = np.concatenate([av + stay_tr[aq], (av[k_of] + otr[e]) + ow[e]])
                o = np.lexsort((cs, -cv, ct))                # per target: value descending, source ascending
                ct, cs, cv = ct[o], cs[o], cv[o]
                first = np.ones(ct.size, bool)
                first[1:] = ct[1:] != ct[:-1]
                bt, bsrc, bv = ct[first], cs[first], cv[first]
                aq, av, kept = prune(bt, bv + xb[t, label[bt]])
                hist.append((aq, bsrc[kept]))
                nact.append(aq.size)
            if sizes is not None:
                sizes.append(nact)
            if aq.size == 0:
                continue
            end = av + finw[state[aq]]
            o = np.lexsort((aq, -end))[0]
            if not end[o] > ninf:
                continue
            scores[b] = end[o]
            q = int(aq[o])
            for t in range(L - 1, -1, -1):
                path[b, t], states[b, t] = label[q], state[q]
                if t >= 1:
                    fq, fs = hist[t]
                    q = int(fs[np.nonzero(fq == q)[0][0]])
            p = path[b, :L]
            keep = np.ones(L, bool)
            keep[1:] = p[1:] != p[:-1]
            tk = p[keep]
            tokens[b, :len(tk)] = tk
            token_lengths[b] = len(tk)
    return scores, path, tokens, token_lengths, states
