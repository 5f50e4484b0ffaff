"""Test-only numpy restatement of the beam-pruned full score of the ASG lattice composed with a token automaton and of its
gradients (`torch_asg_amd.beam_graph_full_score`, `beam_graph_asg_loss`), written from the specification
(include/asg_hip.h::asg_beam_graph_full_forward) and not from the kernels.

Step 1, the search, in the dtype of the emissions (restated here: tests/beam_decode_ref.py does not return its sets): the
candidates of frame t come only from A_{t-1}; a target keeps its largest candidate, the smallest source on a tie; c = best +
emission; with m = max c and lo = fl(m - threshold), A_t = the first K states in (c descending, q ascending) order with c >= lo.
Steps 2-4 in float64 (weights folded in the emissions' dtype, then widened): the forced states F_t of the merged target, the
lattice U_t = A_t | F_t, alpha / beta / posteriors over it.
"""
import numpy as np

from graph_decode_ref import _clamped_lengths, fold, product
from graph_loss_ref import Composed, _grouped_lse, _lse


def search(xb, tr, nxt, weight, final, start, L, K, theta, lm_weight=1.0, token_score=0.0, _cache=None):
    """One utterance xb [T,N] in its own dtype -> dict(sets=[A_t ascending], sizes, score, path, states, margin).
    margin = the smallest distance, over the frames, of the K-th to the (K+1)-th candidate value and of any candidate to lo
    (inf where neither rule had a candidate to cut)."""
    x = np.asarray(xb)
    dt = x.dtype.type
    tr = np.ascontiguousarray(np.asarray(tr), dtype=dt)
    theta = dt(theta)
    if _cache is not None and "g" in _cache:
        g = _cache["g"]
    else:
        present, arcw, finw = fold(nxt, weight, final, dt, lm_weight, token_score)
        label, state, src, tgt, Q = product(nxt, present)
        ninf = dt(-np.inf)
        g = dict(label=label, state=state, Q=Q, finw=finw)
        if Q:
            g["start_w"] = np.where(present[start, label] & (nxt[start, label] == state), arcw[start, label], ninf).astype(dt)
            order = np.lexsort((tgt, src))
            osrc, otgt = src[order], tgt[order]
            orow = np.zeros(Q + 1, np.int64)
            np.cumsum(np.bincount(osrc, minlength=Q), out=orow[1:])
            g.update(otgt=otgt, orow=orow, otr=tr[label[otgt], label[osrc]], ow=arcw[state[osrc], label[otgt]],
                     stay_tr=tr[label, label])
        if _cache is not None:
            _cache["g"] = g
    label, state, Q = g["label"], g["state"], g["Q"]
    ninf = dt(-np.inf)
    out = dict(sets=[np.zeros(0, np.int64) for _ in range(L)], sizes=[0] * L, score=ninf, path=None, states=None, margin=np.inf)
    if L == 0 or Q == 0:
        return out
    margin = [np.inf]

    def prune(q, c):
        ok = c > ninf
        idx = np.nonzero(ok)[0]
        q, c = q[idx], c[idx]
        if q.size == 0:
            return q, c, idx
        lo = c.max() - theta
        rank = np.lexsort((q, -c))
        cs = c[rank].astype(np.float64)
        if cs.size > K:
            margin[0] = min(margin[0], float(cs[K - 1] - cs[K]))
        if np.isfinite(lo):
            margin[0] = min(margin[0], float(np.abs(cs - np.float64(lo)).min()))
        rank = rank[:K]
        rank = rank[c[rank] >= lo]
        return q[rank], c[rank], idx[rank]

    with np.errstate(invalid="ignore", over="ignore"):
        aq, av, _ = prune(np.arange(Q), g["start_w"] + x[0, label])
        hist = [(aq, None)]
        for t in range(1, L):
            if aq.size == 0:
                hist.append((aq, aq))
                continue
            orow, otgt = g["orow"], g["otgt"]
            cnt = orow[aq + 1] - orow[aq]
            k_of = np.repeat(np.arange(aq.size), cnt)
            e = orow[aq][k_of] + (np.arange(k_of.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))
            ct = np.concatenate([aq, otgt[e]])
            cs = np.concatenate([aq, aq[k_of]])
            cv = np.concatenate([av + g["stay_tr"][aq], (av[k_of] + g["otr"][e]) + g["ow"][e]])
            o = np.lexsort((cs, -cv, ct))
            ct, cs, cv = ct[o], cs[o], cv[o]
            first = np.ones(ct.size, bool)
            first[1:] = ct[1:] != ct[:-1]
            bt, bsrc, bv = ct[first], cs[first], cv[first]
            aq, av, kept = prune(bt, bv + x[t, label[bt]])
            hist.append((aq, bsrc[kept]))
        out["sets"] = [np.sort(h[0]) for h in hist]
        out["sizes"] = [int(h[0].size) for h in hist]
        out["margin"] = margin[0]
        if aq.size:
            end = av + g["finw"][state[aq]]
            o = np.lexsort((aq, -end))[0]
            if end[o] > ninf:
                out["score"] = end[o]
                q = int(aq[o])
                path, sts = np.zeros(L, np.int64), np.zeros(L, np.int64)
                for t in range(L - 1, -1, -1):
                    path[t], sts[t] = label[q], state[q]
                    if t >= 1:
                        fq, fs = hist[t]
                        q = int(fs[np.nonzero(fq == q)[0][0]])
                out["path"], out["states"] = path, sts
    return out


def forced_sets(c, y, L):
    """The F_t of one utterance: c a graph_loss_ref.Composed, y the raw target (already cut to its length), L frames.
    -> list of L int arrays (all empty when nothing is forced)."""
    empty = [np.zeros(0, np.int64) for _ in range(L)]
    tl = len(y)
    if tl == 0 or tl > L:
        return empty
    N = c.nxt.shape[1]
    st, prev, qs = c.start, None, []
    for v in y:
        v = int(v)
        if v == prev:
            continue
        if not 0 <= v < N or not c.present[st, v]:
            return empty
        st = int(c.nxt[st, v])
        qs.append(int(np.nonzero((c.state == st) & (c.label == v))[0][0]))
        prev = v
    if c.finw[st] == -np.inf:
        return empty
    n = len(qs)
    return [np.array(sorted({qs[k - 1] for k in range(1, n + 1) if k - 1 <= t and n - k <= L - 1 - t}), np.int64)
            for t in range(L)]


def lattice(c, x, tr, L, U):
    """alpha / beta over the lattice U (list of L ascending int arrays) in float64 -> (Z, dZ/dx [T,N], dZ/dtr [N,N])."""
    T, N = x.shape
    Q, lab, src, tgt = c.Q, c.label, c.src, c.tgt
    gx, gtr = np.zeros((T, N)), np.zeros((N, N))
    if L == 0 or Q == 0:
        return -np.inf, gx, gtr
    mask = np.zeros((L, Q), bool)
    for t in range(L):
        mask[t, U[t]] = True
    stay = tr[lab, lab]
    etr = tr[lab[tgt], lab[src]]
    grp = np.concatenate([np.arange(Q), tgt])
    grp_b = np.concatenate([np.arange(Q), src])
    alpha = np.full((L, Q), -np.inf)
    alpha[0] = np.where(mask[0], c.start_w + x[0, lab], -np.inf)
    for t in range(1, L):
        cand = np.concatenate([alpha[t - 1] + stay, alpha[t - 1][src] + etr + c.edge_w])
        alpha[t] = np.where(mask[t], _grouped_lse(cand, grp, Q) + x[t, lab], -np.inf)
    Z = _lse(alpha[L - 1] + c.final_w)
    if Z == -np.inf:
        return Z, gx, gtr
    beta = np.full((L, Q), -np.inf)
    beta[L - 1] = np.where(mask[L - 1], c.final_w, -np.inf)
    for t in range(L - 1, 0, -1):
        cand = np.concatenate([beta[t] + stay + x[t, lab], beta[t][tgt] + etr + c.edge_w + x[t, lab[tgt]]])
        beta[t - 1] = np.where(mask[t - 1], _grouped_lse(cand, grp_b, Q), -np.inf)
    with np.errstate(invalid="ignore"):
        gam = np.nan_to_num(np.exp(alpha + beta - Z))
        for t in range(L):
            np.add.at(gx[t], lab, gam[t])
        for t in range(1, L):
            ps = np.nan_to_num(np.exp(alpha[t - 1] + stay + x[t, lab] + beta[t] - Z))
            np.add.at(gtr, (lab, lab), ps)
            pe = np.nan_to_num(np.exp(alpha[t - 1][src] + etr + c.edge_w + x[t, lab[tgt]] + beta[t][tgt] - Z))
            np.add.at(gtr, (lab[tgt], lab[src]), pe)
    return Z, gx, gtr


def beam_loss_ref(inputs, transition, next_, weight, final, start=0, input_lengths=None, beam_size=1, beam_threshold=np.inf,
                  lm_weight=1.0, token_score=0.0, targets=None, target_lengths=None, grad_scores=None, info=None):
    """inputs [T,B,N] (their dtype is the search's dtype) -> (Z_K [B], grad_inputs [T,B,N], grad_transition [N,N], U) with
    U[b] the list of the utterance's U_t.  `info`, if a dict, receives 'search' (the per-utterance results of `search`) and
    'margin' (the smallest margin over the batch)."""
    xs = np.asarray(inputs)
    dt = xs.dtype.type
    T, B, N = xs.shape
    x = xs.astype(np.float64)
    tr = np.asarray(transition, np.float64)
    nxt = np.asarray(next_, np.int64)
    lens = _clamped_lengths(input_lengths, T, B)
    g = np.ones(B) if grad_scores is None else np.asarray(grad_scores, np.float64)
    c = Composed(nxt, weight, final, start, lm_weight, token_score, fold_dt=dt)
    Z, gx, gtr, Us, found = np.zeros(B), np.zeros((T, B, N)), np.zeros((N, N)), [], []
    cache = {}
    if targets is not None:
        tg = np.asarray(targets)
        S = tg.shape[1]
        tls = np.full(B, S) if target_lengths is None else np.clip(np.asarray(target_lengths), 0, S)
    for b in range(B):
        L = int(lens[b])
        r = search(xs[:, b], np.asarray(transition).astype(dt), nxt, weight, final, start, L, int(beam_size), beam_threshold,
                   lm_weight, token_score, cache)
        found.append(r)
        U = r["sets"]
        if targets is not None:
            F = forced_sets(c, tg[b, :int(tls[b])], L)
            U = [np.union1d(a, f).astype(np.int64) for a, f in zip(U, F)]
        Us.append(U)
        Z[b], gxb, gtb = lattice(c, x[:, b], tr, L, U)
        gx[:, b] = g[b] * gxb
        gtr += g[b] * gtb
    if info is not None:
        info["search"] = found
        info["margin"] = min([r["margin"] for r in found] + [np.inf])
    return Z, gx, gtr, Us
