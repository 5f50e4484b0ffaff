"""Test-only numpy restatement of best-path force alignment (`torch_asg_amd.viterbi_align`, csrc/asg_viterbi.hip), written
from the formula in the kernel file's header:

    v[0][s] = I[0][O_0] for s == 0 else -inf
    v[t][s] = I[t][O_s] + max(v[t-1][s] + Tr[O_s][O_s], v[t-1][s-1] + Tr[O_s][O_{s-1}])          ties keep "stay"
    score = v[len-1][ol-1];  positions by back-pointers, -1 for t >= len and for utterances without a finite alignment

Arithmetic in the dtype of the emissions and in the kernels' order -- (v + tr) first, then the emission is added -- adds and
compares only, so the GPU results must equal these bit for bit.  The lengths, the -1 and the -inf conventions are those of
oracle/asg_oracle_impl.inc::asg_oracle_viterbi.  All utterances advance together, one numpy step per frame over [B, S].
"""
import numpy as np


def _lengths(lengths, B, top):
    if lengths is None:
        return np.full(B, top, np.int64)
    return np.minimum(np.asarray(lengths, dtype=np.int64).reshape(B), top)


def viterbi_ref(inputs, targets, transition, input_lengths=None, target_lengths=None, take=None):
    """inputs [T,B,N], targets [B,S] int64, transition [N,N] (tr[i][j] = score of j -> i), lengths [B] or None.
    -> scores [B] (dtype of inputs), positions [B,T] int64.
    take(come, stay) -> bool array: which predecessor wins; the default is the kernels' `come > stay`.  Tests pass another rule
    only to build WRONG variants and show that their inputs tell the two apart."""
    x = np.asarray(inputs)
    T, B, N = x.shape
    dt = x.dtype
    tg = np.asarray(targets, dtype=np.int64)
    S = tg.shape[1]
    tr = np.asarray(transition).astype(dt)
    if take is None:
        take = lambda come, stay: come > stay                                          # noqa: E731
    lens, ols = _lengths(input_lengths, B, T), _lengths(target_lengths, B, S)
    feasible = (lens >= 1) & (ols >= 1) & (ols <= lens)
    scores = np.full(B, -np.inf, dt)
    pos = np.full((B, T), -1, np.int64)
    if not feasible.any():
        return scores, pos
    ninf = dt.type(-np.inf)
    act = np.arange(S)[None, :] < ols[:, None]                                          # [B,S]: position s belongs to utterance b
    H = tr[tg, tg]                                                                      # stay on O_s
    D = np.full((B, S), ninf, dt)
    D[:, 1:] = tr[tg[:, 1:], tg[:, :-1]]                                                # come from O_{s-1}
    rows = np.arange(B)[:, None]
    v = np.full((B, S), ninf, dt)
    v[:, 0] = x[0, np.arange(B), tg[:, 0]]
    Tmax = int(lens[feasible].max())
    bits = np.zeros((Tmax, B, (S + 7) // 8), np.uint8)                                  # back-pointers, packed along s
    left = np.full((B, S), ninf, dt)
    with np.errstate(invalid="ignore"):
        for t in range(1, Tmax):
            stay = v + H
            left[:, 1:] = v[:, :-1]
            come = left + D
            tk = take(come, stay)
            em = np.where(act, x[t][rows, tg], ninf)
            w = em + np.where(tk, come, stay)
            live = (t < lens)[:, None]
            v = np.where(live, w, v)                                                    # a finished utterance keeps its last frame
            bits[t] = np.packbits(tk & live, axis=1)
    for b in np.nonzero(feasible)[0]:
        L, ol = int(lens[b]), int(ols[b])
        best = v[b, ol - 1]
        if not best > -np.inf:                                                          # no finite alignment (NaN: unspecified)
            continue
        scores[b] = best
        s = ol - 1
        for t in range(L - 1, -1, -1):
            pos[b, t] = s
            if t >= 1 and (bits[t, b, s >> 3] >> (7 - (s & 7))) & 1:
                s -= 1
    return scores, pos


def labels_of(targets, pos):
    """The label emitted at every frame: targets gathered at the positions, -1 where the position is -1."""
    tg = np.asarray(targets, dtype=np.int64)
    return np.where(pos >= 0, np.take_along_axis(tg, np.maximum(pos, 0), axis=1), -1)
