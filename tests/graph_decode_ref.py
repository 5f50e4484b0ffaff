"""Test-only numpy restatement of Viterbi decoding over the ASG lattice composed with a token automaton
(`torch_asg_amd.viterbi_decode_graph`), written from the spec and not from torch_asg_amd/graph.py.

Folding in the decode dtype: arcw = fl(fl(lm_weight * weight) + token_score), finw = fl(lm_weight * final) (-inf where final
is -inf).  Product states (i, s'), one per pair reached by some arc s --i--> s', numbered in (s', i) order.  Each candidate is
formed in the kernels' order -- stay: v + tr[i][i]; move: (v + tr[i][j]) + arcw -- then the emission is added; the winner is
the largest value, the smallest source index on a tie, and the final argmax takes the smallest q.  Adds and maxes only, so the
GPU results must equal these bit for bit.
"""
import numpy as np


def _clamped_lengths(input_lengths, T, B):
    if input_lengths is None:
        return np.full(B, T, np.int64)
    return np.clip(np.asarray(input_lengths, dtype=np.int64).reshape(B), 0, T)


def fold(next_, weight, final, dt, lm_weight, token_score):
    """-> (present [S,N] bool, arcw [S,N] dt, finw [S] dt)."""
    dt = np.dtype(dt).type
    lw, ts = dt(lm_weight), dt(token_score)
    present = (np.asarray(next_) >= 0) & (np.asarray(weight) != -np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        arcw = (lw * np.asarray(weight, np.float64).astype(dt)) + ts
        finw = np.where(np.asarray(final) == -np.inf, dt(-np.inf), lw * np.asarray(final, np.float64).astype(dt)).astype(dt)
    return present, arcw.astype(dt), finw


def product(next_, present):
    """Product states and edges, enumerated from the SOURCES: (label [Q], state [Q], src [E], tgt [E]) with the edges sorted
    by (tgt, src)."""
    nxt = np.asarray(next_)
    S, N = nxt.shape
    s_a, i_a = np.nonzero(present)
    keys = np.unique(nxt[s_a, i_a] * N + i_a)
    label, state = keys % N, keys // N
    Q = keys.size
    # every source q' = (j, s) moves on every token i != j that has an arc from s
    ok = present[state] & (np.arange(N)[None, :] != label[:, None])        # [Q, N]
    src, tok = np.nonzero(ok)
    tgt = np.searchsorted(keys, nxt[state[src], tok] * N + tok)
    order = np.lexsort((src, tgt))
    return label, state, src[order], tgt[order], Q


def decode_graph_ref(inputs, transition, next_, weight, final, start=0, input_lengths=None, lm_weight=1.0, token_score=0.0):
    """inputs [T,B,N], transition [N,N] (tr[i][j] scores j -> i), the automaton (next [S,N], weight [S,N], final [S],
    start).  -> scores [B] (dtype of inputs), path, tokens [B,T] int64, token_lengths [B] int64, states [B,T] int64."""
    x = np.asarray(inputs)
    T, B, N = x.shape
    dt = x.dtype.type
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
    start_w = np.where(present[start, label] & (nxt[start, label] == state), arcw[start, label], dt(-np.inf)).astype(dt)
    stay_tr = tr[label, label]
    edge_tr = tr[label[tgt], label[src]]
    edge_w = arcw[state[src], label[tgt]]
    has = np.bincount(tgt, minlength=Q) > 0
    starts = np.searchsorted(tgt, np.nonzero(has)[0])
    big = np.iinfo(np.int64).max
    v = start_w[None, :] + x[0][:, label]                                  # [B, Q]
    vs, bps = [v], [None]
    for t in range(1, int(lens.max(initial=0))):
        best = v + stay_tr[None, :]
        arg = np.broadcast_to(np.arange(Q), (B, Q)).copy()
        if src.size:
            cand = (v[:, src] + edge_tr[None, :]) + edge_w[None, :]           # [B, E]
            emax = np.maximum.reduceat(cand, starts, axis=1)
            eq = cand == np.repeat(emax, np.diff(np.append(starts, src.size)), axis=1)
            esrc = np.minimum.reduceat(np.where(eq, src[None, :], big), starts, axis=1)
            cols = np.nonzero(has)[0]
            sb, sa = best[:, cols], arg[:, cols]
            win = (emax > sb) | ((emax == sb) & (esrc < sa))
            best[:, cols] = np.where(win, emax, sb)
            arg[:, cols] = np.where(win, esrc, sa)
        v = best + x[t][:, label]
        vs.append(v)
        bps.append(arg)
    for b in range(B):
        L = int(lens[b])
        if L == 0:
            continue
        end = vs[L - 1][b] + finw[state]
        q = int(np.argmax(end))                                             # first index of the max
        if not end[q] > -np.inf:                                            # no finite path (NaN is unspecified)
            continue
        scores[b] = end[q]
        for t in range(L - 1, -1, -1):
            path[b, t], states[b, t] = label[q], state[q]
            if t >= 1:
                q = int(bps[t][b, q])
        p = path[b, :L]
        keep = np.ones(L, bool)
        keep[1:] = p[1:] != p[:-1]
        tk = p[keep]
        tokens[b, :len(tk)] = tk
        token_lengths[b] = len(tk)
    return scores, path, tokens, token_lengths, states


def path_score_graph(inputs_b, transition, next_, weight, final, labels, start=0, lm_weight=1.0, token_score=0.0):
    """Score of one label sequence through the composed lattice, in the kernels' order; -inf if the automaton rejects it.
    -> (score, automaton state after every frame)."""
    x = np.asarray(inputs_b)
    dt = x.dtype.type
    tr = np.asarray(transition, dtype=dt)
    nxt = np.asarray(next_, np.int64)
    present, arcw, finw = fold(nxt, weight, final, dt, lm_weight, token_score)
    ninf = dt(-np.inf)
    l0 = int(labels[0])
    if not present[start, l0]:
        return ninf, None
    s = int(nxt[start, l0])
    sts = [s]
    v = arcw[start, l0] + x[0, l0]
    for t in range(1, len(labels)):
        i, j = int(labels[t]), int(labels[t - 1])
        if i == j:
            v = (v + tr[i, i]) + x[t, i]
        else:
            if not present[s, i]:
                return ninf, None
            v = ((v + tr[i, j]) + arcw[s, i]) + x[t, i]
            s = int(nxt[s, i])
        sts.append(s)
    return v + finw[s], sts
