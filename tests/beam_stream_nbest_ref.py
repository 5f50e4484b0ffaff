"""Test-only numpy restatement of the N BEST hypotheses of the two token-graph beam streams (`BeamStream.result_nbest`,
`BeamWindowStream.result_nbest`), written from the specification (include/asg_hip.h::asg_beam_stream_nbest and
::asg_beam_window_nbest) and not from the package.  It works over the carried state of the two stream restatements
(tests/beam_stream_ref.py: `aq`, `av`, `history`; tests/beam_window_ref.py: `ring`, `base`, `carry`, through its `_walk`), which it
only reads.

Candidates, both calls: end[q] = v[q] + final_w[q] (final) or v[q] (prefix) over the stored set, the q with end > -inf in
(end descending, q ascending) order; the first nbest of them are the rows.  The stream follows a row's back-pointers over all pos
frames and adds start weight, the weight of every edge taken in frame order and -- final only -- the final weight.  The window
follows them down to `base` only, and collapses the tail behind `carry`.
"""
import numpy as np


def _candidates(s, aq, av, final):
    """The positions in the set (aq, av) of the candidates in order, and every end."""
    with np.errstate(invalid="ignore", over="ignore"):
        end = av + s.finw[s.state[aq]] if final else av
    cand = np.nonzero(end > s.ninf)[0]
    return cand[np.lexsort((aq[cand], -end[cand]))], end     # end descending, q ascending (-0 == +0 under -end too)


def stream_nbest(ref, nbest, final):
    """ref: a BeamStreamRef -> scores, graph_scores [B,nbest], tokens [B,nbest,max_frames], token_lengths [B,nbest], num_hyps [B],
    path, states [B,nbest,max_frames], frames, status [B]."""
    B, T, dt, nbest = ref.B, ref.max_frames, ref.dt, int(nbest)
    assert nbest >= 1
    scores = np.full((B, nbest), -np.inf, dt)
    gscores = np.full((B, nbest), -np.inf, dt)
    tokens = np.full((B, nbest, T), -1, np.int64)
    token_lengths = np.zeros((B, nbest), np.int64)
    num_hyps = np.zeros(B, np.int64)
    path = np.full((B, nbest, T), -1, np.int64)
    states = np.full((B, nbest, T), -1, np.int64)
    frames = np.array([s.pos for s in ref.slots], np.int64)
    status = np.array([s.overflow for s in ref.slots], np.int64)
    for b, s in enumerate(ref.slots):
        L = s.pos
        if L == 0 or s.aq.size == 0:
            continue
        cand, end = _candidates(ref, s.aq, s.av, final)
        num_hyps[b] = nh = min(nbest, cand.size)
        for r in range(nh):
            scores[b, r] = end[cand[r]]
            q = int(s.aq[cand[r]])
            qs = [0] * L
            for t in range(L - 1, -1, -1):
                qs[t] = q
                if t >= 1:
                    fq, fs = s.history[t]
                    q = int(fs[np.nonzero(fq == q)[0][0]])
            lab = ref.label[qs]
            path[b, r, :L], states[b, r, :L] = lab, ref.state[qs]
            keep = np.ones(L, bool)
            keep[1:] = lab[1:] != lab[:-1]
            tk = lab[keep]
            tokens[b, r, :tk.size] = tk
            token_lengths[b, r] = tk.size
            with np.errstate(invalid="ignore", over="ignore"):
                g = ref.start_w[qs[0]]
                for t in range(1, L):
                    if qs[t] != qs[t - 1]:
                        row = slice(ref.orow[qs[t - 1]], ref.orow[qs[t - 1] + 1])
                        g = g + ref.ow[row][np.nonzero(ref.otgt[row] == qs[t])[0][0]]
                if final:
                    g = g + ref.finw[ref.state[qs[-1]]]
            gscores[b, r] = g
    return scores, gscores, tokens, token_lengths, num_hyps, path, states, frames, status


def window_nbest(ref, nbest, final):
    """ref: a BeamWindowRef -> scores [B,nbest], tokens [B,nbest,W], token_lengths [B,nbest], num_hyps [B], path, states
    [B,nbest,W], frames, committed, status [B]."""
    B, W, dt, s, nbest = ref.B, ref.W, ref.dt, ref.s, int(nbest)
    assert nbest >= 1
    scores = np.full((B, nbest), -np.inf, dt)
    tokens = np.full((B, nbest, W), -1, np.int64)
    token_lengths = np.zeros((B, nbest), np.int64)
    num_hyps = np.zeros(B, np.int64)
    path = np.full((B, nbest, W), -1, np.int64)
    states = np.full((B, nbest, W), -1, np.int64)
    frames = np.array([v.pos for v in ref.slots], np.int64)
    committed = np.array([v.base for v in ref.slots], np.int64)
    status = np.array([v.status | (2 if v.pos >= 1 and v.aq.size == 0 else 0) for v in ref.slots], np.int64)
    for b, v in enumerate(ref.slots):
        if v.pos == 0 or v.aq.size == 0:
            continue
        cand, end = _candidates(s, v.aq, v.av, final)
        num_hyps[b] = nh = min(nbest, cand.size)
        for r in range(nh):
            scores[b, r] = end[cand[r]]
            qs = ref._walk(v, int(v.aq[cand[r]]), v.pos - 1, v.base)     # empty when base == pos: the row still counts
            lab = s.label[qs]
            path[b, r, :len(qs)], states[b, r, :len(qs)] = lab, s.state[qs]
            prev = np.concatenate([[v.carry], lab[:-1]])[:len(lab)]
            tk = lab[lab != prev]
            tokens[b, r, :len(tk)] = tk
            token_lengths[b, r] = len(tk)
    return scores, tokens, token_lengths, num_hyps, path, states, frames, committed, status
