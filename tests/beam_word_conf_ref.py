"""Test-only numpy restatement of the word confidences and end frames of the word-LM beam decoder
(`torch_asg_amd.beam_decode_words_confidence`), written from the specification (include/asg_hip.h::asg_beam_words_confidence)
and not from the kernels.

The kept sets A_t and the hypothesis come from tests/beam_word_ref.py (`beam_word_ref(..., info=)`) or, with `order`, from
tests/beam_word_la_ref.py; the model of a pair's edges and ends is tests/beam_word_loss_ref.py's (`word_model`, plain weights).
alpha and beta run over the lattice U_t = A_t in float64 with plain loops; the posterior of every word-end event is formed by
the formula, event by event, into a dict keyed by (word, frame).  No tables and no ranks.
"""
import numpy as np

from beam_word_la_loss_ref import la_lattice_sets
from beam_word_loss_ref import _lse, lattice_sets

DECODE = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths")


def word_events(m, x, tr, L, U):
    """One utterance: x [T,N] and tr [N,N] float64, U the list of its L lattice sets -> (Z_K, {(word, frame): P(word, frame)})."""
    if L == 0:
        return -np.inf, {}
    lab, start = m.label, int(m.lm.start)
    alpha = [{p: (m.start_w[p[1]] + x[0, lab[p[1]]] if p[0] == start else -np.inf) for p in U[0]}]
    edges = [None]
    for t in range(1, L):
        inc = {p: [] for p in U[t]}
        ed = []
        for p in U[t - 1]:
            a = alpha[t - 1][p]
            for k, (p2, w, i) in enumerate(m.edges(p)):
                if p2 in inc:
                    ed.append((p, p2, w, i, k > 0 and i == m.sep))         # (edge 0 is the stay: never a word's end)
                    if a > -np.inf:
                        inc[p2].append((a + tr[i, lab[p[1]]]) + w)
        edges.append(ed)
        alpha.append({p: _lse(c) + x[t, lab[p[1]]] for p, c in inc.items()})
    Z = _lse([alpha[L - 1][p] + m.endw(p) for p in U[L - 1]])
    if Z == -np.inf:
        return Z, {}
    beta = [None] * L
    beta[L - 1] = {p: m.endw(p) for p in U[L - 1]}
    for t in range(L - 1, 0, -1):
        out = {p: [] for p in U[t - 1]}
        for p, p2, w, i, _ in edges[t]:
            out[p].append(((beta[t][p2] + tr[i, lab[p[1]]]) + w) + x[t, i])
        beta[t - 1] = {p: _lse(c) for p, c in out.items()}
    P = {}
    for t in range(1, L):
        for p, p2, w, i, word_end in edges[t]:
            if not word_end:
                continue
            v = alpha[t - 1][p] + tr[i, lab[p[1]]] + w + x[t, i] + beta[t][p2] - Z
            if v > -np.inf:
                key = (int(m.wos[m.state[p[1]]]), t)
                P[key] = P.get(key, 0.0) + np.exp(v)
    for p in U[L - 1]:                                                       # the final step of the end rule
        s = int(m.state[p[1]])
        v = alpha[L - 1][p] + m.endw(p) - Z
        if s != 0 and v > -np.inf:
            key = (int(m.wos[s]), L)
            P[key] = P.get(key, 0.0) + np.exp(v)
    return Z, P


def hypothesis_frames(path, n_words, L, sep):
    """End frames of the words of a winning path: the frames whose label is the separator behind another label, then L for
    the word of the final step."""
    frames = [t for t in range(1, L) if path[t] == sep and path[t - 1] != sep]
    if len(frames) < n_words:
        frames.append(L)
    assert len(frames) == n_words
    return frames


def beam_word_conf_ref(inputs, transition, lexicon, lm, input_lengths=None, beam_size=1, beam_threshold=np.inf, lm_weight=1.0,
                       word_score=0.0, token_score=0.0, frame_tolerance=0, order=None, info=None):
    """inputs [T,B,N] (their dtype is the search's dtype) -> dict: the decoder's eight outputs (of the look-ahead search of
    `order` when given), word_frames [B,T] int64, word_confidences [B,T] float64, normalisers [B] float64, events (per utterance
    the dict {(word, frame): P}) and sets (per utterance the list of its A_t).  `info`, if a dict, receives the search's info."""
    xs = np.asarray(inputs)
    T, B, N = xs.shape
    inf = {}
    if order is None:
        m, lens, _, _, Us = lattice_sets(xs, transition, lexicon, lm, input_lengths, beam_size, beam_threshold, lm_weight,
                                         word_score, token_score, info=inf)
    else:
        m, lens, _, _, Us = la_lattice_sets(xs, transition, lexicon, lm, order, input_lengths, beam_size, beam_threshold,
                                            lm_weight, word_score, token_score, info=inf)
    dec = inf["decode"]
    if info is not None:
        info.update(inf)
    x, tr = xs.astype(np.float64), np.asarray(transition, np.float64)
    tol = int(frame_tolerance)
    res = {n: dec[n] for n in DECODE}
    res["word_frames"] = np.full((B, T), -1, np.int64)
    res["word_confidences"] = np.zeros((B, T))
    res["normalisers"] = np.full(B, -np.inf)
    res["events"], res["sets"] = [], Us
    for b in range(B):
        L = int(lens[b])
        Z, P = word_events(m, x[:, b], tr, L, Us[b])
        res["normalisers"][b] = Z
        res["events"].append(P)
        nw = int(dec["word_lengths"][b])
        if nw == 0:
            continue
        frames = hypothesis_frames(dec["path"][b], nw, L, m.sep)
        res["word_frames"][b, :nw] = frames
        for k, tk in enumerate(frames):
            w = int(dec["words"][b, k])
            res["word_confidences"][b, k] = sum(P.get((w, t), 0.0) for t in range(max(1, tk - tol), min(L, tk + tol) + 1))
    return res
