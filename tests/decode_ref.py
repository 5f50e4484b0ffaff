"""Test-only numpy restatement of Viterbi decoding over the fully-connected ASG lattice (`torch_asg_amd.viterbi_decode`).

Arithmetic in the dtype of the emissions and in the kernels' order -- each candidate is (v + tr), then the emission is
added -- adds and maxes only, every argmax the smallest index on a tie; so the GPU results must equal these bit for bit.
"""
import numpy as np

_CHUNK = 1 << 24          # candidate elements per numpy step (bounds the memory of the large-alphabet cases)


def _clamped_lengths(input_lengths, T, B):
    if input_lengths is None:
        return np.full(B, T, np.int64)
    return np.clip(np.asarray(input_lengths, dtype=np.int64).reshape(B), 0, T)


def _frame(v, tr):
    """max_j (v[b][j] + tr[i][j]) for every b, i -> [B, N] in the dtype of v."""
    B, N = v.shape
    out = np.empty((B, N), v.dtype)
    rows = max(1, _CHUNK // max(1, B * N))
    for i0 in range(0, N, rows):
        out[:, i0:i0 + rows] = (v[:, None, :] + tr[None, i0:i0 + rows, :]).max(axis=2)
    return out


def decode_ref(inputs, transition, input_lengths=None, argmax=np.argmax):
    """inputs [T,B,N], transition [N,N] (tr[i][j] = score of j -> i), input_lengths [B] or None.
    -> scores [B] (dtype of inputs), path [B,T] int64, tokens [B,T] int64, token_lengths [B] int64.
    argmax(vector) -> index: the default is the kernels' first index of the max.  Tests pass another rule only to build WRONG
    variants and show that their inputs tell the two apart."""
    x = np.asarray(inputs)
    T, B, N = x.shape
    dt = x.dtype
    tr = np.ascontiguousarray(np.asarray(transition), dtype=dt)
    lens = _clamped_lengths(input_lengths, T, B)
    scores = np.full(B, -np.inf, dt)
    path = np.full((B, T), -1, np.int64)
    tokens = np.full((B, T), -1, np.int64)
    token_lengths = np.zeros(B, np.int64)
    if T == 0:
        return scores, path, tokens, token_lengths
    # forward over all utterances at once; every frame's vector is kept for the backtrace
    vs = [np.array(x[0], dtype=dt)]
    for t in range(1, int(lens.max(initial=0))):
        vs.append(_frame(vs[-1], tr) + x[t])
    for b in range(B):
        L = int(lens[b])
        if L == 0:
            continue
        last = vs[L - 1][b]
        best = last.max()
        if not best > -np.inf:                      # no finite path (NaN is unspecified)
            continue
        scores[b] = best
        s = int(argmax(last))                       # first index of the max
        path[b, L - 1] = s
        for t in range(L - 1, 0, -1):
            s = int(argmax(vs[t - 1][b] + tr[s]))
            path[b, t - 1] = s
        p = path[b, :L]
        keep = np.ones(L, bool)
        keep[1:] = p[1:] != p[:-1]
        tk = p[keep]
        tokens[b, :len(tk)] = tk
        token_lengths[b] = len(tk)
    return scores, path, tokens, token_lengths


def path_score(inputs_b, transition, labels):
    """Score of one label sequence through the lattice, in the kernels' order: ((v + tr) + I)."""
    x = np.asarray(inputs_b)
    tr = np.asarray(transition, dtype=x.dtype)
    v = x[0, labels[0]]
    for t in range(1, len(labels)):
        v = (v + tr[labels[t], labels[t - 1]]) + x[t, labels[t]]
    return v
