"""Test-only numpy restatement of the n-best beam decoder with its score split (`torch_asg_amd.beam_decode_graph_nbest`),
written from the specification (include/asg_hip.h::asg_beam_decode_graph_nbest and ::asg_beam_decode_graph) and not from the
package.  Folding and product states are those of tests/graph_decode_ref.py (`fold`, `product`); the search is restated here.

Search, per utterance and frame: the candidates of frame t come only from the active set of frame t-1 (the stay of an active q,
whose source is q, and every edge out of an active q'); a target keeps its largest candidate, the smallest source on a tie;
c = best + emission; states with c = -inf are dropped; with m = max c and lo = fl(m - threshold) the new active set is the first
K states in (c descending, q ascending) order that have c >= lo.  End: end[q] = v[q] + final_w[q] over the last set; the
candidates are the q with end > -inf in (end descending, q ascending) order; the first nbest of them are the hypotheses, each
with its back-pointer path.  The two partial scores add the path's own terms in frame order.  All arithmetic in the dtype of
the emissions, adds only (one subtraction for lo).
"""
import numpy as np

from graph_decode_ref import fold, product


def beam_nbest_ref(inputs, transition, next_, weight, final, start=0, input_lengths=None, beam_size=1, nbest=1,
                   beam_threshold=np.inf, lm_weight=1.0, token_score=0.0, sizes=None, terms=None):
    """inputs [T,B,N], transition [N,N] (tr[i][j] scores j -> i), the automaton (next [S,N], weight [S,N], final [S], start).
    -> scores, emission_scores, graph_scores [B,nbest] (dtype of inputs), tokens [B,nbest,T], token_lengths [B,nbest],
    num_hyps [B], path, states [B,nbest,T] (int64).  `sizes`, if a list, receives per utterance the list of |A_t|; `terms`,
    if a dict, receives under (b, r) the list of every term added on the path of hypothesis r of utterance b."""
    x = np.asarray(inputs)
    T, B, N = x.shape
    dt = x.dtype.type
    K, nbest = int(beam_size), int(nbest)
    theta = dt(beam_threshold)
    assert K >= 1 and nbest >= 1 and theta >= 0
    ninf = dt(-np.inf)
    tr = np.ascontiguousarray(np.asarray(transition), dtype=dt)
    nxt = np.asarray(next_, np.int64)
    present, arcw, finw = fold(nxt, weight, final, dt, lm_weight, token_score)
    label, state, src, tgt, Q = product(nxt, present)
    if input_lengths is None:
        lens = np.full(B, T, np.int64)
    else:
        lens = np.clip(np.asarray(input_lengths, dtype=np.int64).reshape(B), 0, T)
    scores = np.full((B, nbest), ninf, dt)
    escores = np.full((B, nbest), ninf, dt)
    gscores = np.full((B, nbest), ninf, dt)
    tokens = np.full((B, nbest, T), -1, np.int64)
    token_lengths = np.zeros((B, nbest), np.int64)
    num_hyps = np.zeros(B, np.int64)
    path = np.full((B, nbest, T), -1, np.int64)
    states = np.full((B, nbest, T), -1, np.int64)
    out = (scores, escores, gscores, tokens, token_lengths, num_hyps, path, states)
    if T == 0 or Q == 0:
        return out
    start_w = np.where(present[start, label] & (nxt[start, label] == state), arcw[start, label], ninf).astype(dt)
    final_w = finw[state]
    # the edges grouped by source, targets ascending
    order = np.lexsort((tgt, src))
    osrc, otgt = src[order], tgt[order]
    orow = np.zeros(Q + 1, np.int64)
    np.cumsum(np.bincount(osrc, minlength=Q), out=orow[1:])
    ow = arcw[state[osrc], label[otgt]]

    def prune(q, c, s):
        ok = c > ninf
        q, c, s = q[ok], c[ok], s[ok]
        if q.size == 0:
            return q, c, s
        lo = c.max() - theta
        rank = np.lexsort((q, -c))[:K]                      # c descending, q ascending
        rank = rank[c[rank] >= lo]
        return q[rank], c[rank], s[rank]

    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            L = int(lens[b])
            if L == 0:
                if sizes is not None:
                    sizes.append([])
                continue
            xb = x[:, b]
            allq = np.arange(Q)
            aq, av, _ = prune(allq, start_w + xb[0, label], allq)
            frames = [(aq, None)]                             # per frame: the active states and the source of each
            for t in range(1, L):
                if aq.size == 0:
                    frames.append((aq, aq))
                    continue
                deg = orow[aq + 1] - orow[aq]
                k_of = np.repeat(np.arange(aq.size), deg)
                e = orow[aq][k_of] + (np.arange(k_of.size) - np.repeat(np.cumsum(deg) - deg, deg))
                ct = np.concatenate([aq, otgt[e]])
                cs = np.concatenate([aq, aq[k_of]])
                cv = np.concatenate([av + tr[label[aq], label[aq]], (av[k_of] + tr[label[otgt[e]], label[aq[k_of]]]) + ow[e]])
                o = np.lexsort((cs, -cv, ct))                 # per target: value descending, source ascending
                ct, cs, cv = ct[o], cs[o], cv[o]
                first = np.ones(ct.size, bool)
                first[1:] = ct[1:] != ct[:-1]
                bt, bsrc, bv = ct[first], cs[first], cv[first]
                aq, av, asrc = prune(bt, bv + xb[t, label[bt]], bsrc)
                frames.append((aq, asrc))
            if sizes is not None:
                sizes.append([f[0].size for f in frames])
            if aq.size == 0:
                continue
            end = av + final_w[aq]
            cand = np.nonzero(end > ninf)[0]
            cand = cand[np.lexsort((aq[cand], -end[cand]))]   # end descending, q ascending (-0 == +0 under -end too)
            nh = min(nbest, cand.size)
            num_hyps[b] = nh
            for r in range(nh):
                scores[b, r] = end[cand[r]]
                q = int(aq[cand[r]])
                qs = [0] * L
                for t in range(L - 1, -1, -1):
                    qs[t] = q
                    if t >= 1:
                        fq, fs = frames[t]
                        q = int(fs[np.nonzero(fq == q)[0][0]])
                lab = label[qs]
                path[b, r, :L], states[b, r, :L] = lab, state[qs]
                keep = np.ones(L, bool)
                keep[1:] = lab[1:] != lab[:-1]
                tk = lab[keep]
                tokens[b, r, :tk.size] = tk
                token_lengths[b, r] = tk.size
                a = xb[0, lab[0]]
                g = start_w[qs[0]]
                used = [a, g]
                for t in range(1, L):
                    a = (a + tr[lab[t], lab[t - 1]]) + xb[t, lab[t]]
                    used += [tr[lab[t], lab[t - 1]], xb[t, lab[t]]]
                    if qs[t] != qs[t - 1]:
                        row = slice(orow[qs[t - 1]], orow[qs[t - 1] + 1])
                        w = ow[row][np.nonzero(otgt[row] == qs[t])[0][0]]
                        g = g + w
                        used.append(w)
                g = g + final_w[qs[-1]]
                used.append(final_w[qs[-1]])
                escores[b, r], gscores[b, r] = a, g
                if terms is not None:
                    terms[(b, r)] = used
    return out
