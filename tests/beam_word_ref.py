"""Test-only numpy restatement of beam decoding with a lexicon and a word n-gram LM composed on the fly
(`torch_asg_amd.beam_decode_words`), written from the specification (include/asg_hip.h::asg_beam_decode_words) and not from the
package.  Folding and product states of the lexicon automaton are those of tests/graph_decode_ref.py (`fold`, `product`, with
lm_weight 1); the word LM is folded here: lw = fl(fl(lm_weight * logp) + word_score), bw = fl(lm_weight * bow), ew =
fl(lm_weight * eos), -inf staying -inf.

A search state is a pair (h, q): LM history and product state of the lexicon.  Plain loops over the candidates, one at a time,
in the dtype of the emissions and the order of adds the specification gives: stay v + tr[j][j]; edge (v + tr[i][j]) + ow, and
on a separator edge + a, a being the LM walk's own sum (0, + bw per backoff step, + lw of the arc); then + emission.  Pairs
order by h, then q.
"""
import numpy as np

from beam_decode_ref import select_info
from graph_decode_ref import _clamped_lengths, fold, product


def fold_lm(lm, dt, lm_weight, word_score):
    dt = np.dtype(dt).type
    m, ws = dt(lm_weight), dt(word_score)
    ninf = dt(-np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        sc = lambda a: np.where(np.asarray(a) == -np.inf, ninf, m * np.asarray(a, np.float64).astype(dt)).astype(dt)  # noqa: E731
        lw = np.where(np.asarray(lm.logp) == -np.inf, ninf, sc(lm.logp) + ws).astype(dt)
        return lw, sc(lm.bow), sc(lm.eos)


def beam_word_ref(inputs, transition, lexicon, lm, input_lengths=None, beam_size=1, beam_threshold=np.inf, lm_weight=1.0,
                  word_score=0.0, token_score=0.0, info=None, rank=None, max_backoff=None,
                  rank_where=("cut", "source", "end")):
    """inputs [T,B,N], transition [N,N]; lexicon: an object with .graph (next, weight, final, start = 0), .word_of_state and
    .separator; lm: an object with row, word, logp, next, backoff, bow, start, eos.
    -> dict scores [B], path, tokens, states, lm_states, words [B,T], token_lengths, word_lengths [B].
    `info`, if a dict, receives per utterance: sizes (|A_t|), cands (candidates of frame t, the -inf ones excluded), kept (the
    pairs of A_t as a sorted list), and the totals tie_cuts (frames whose K-th and (K+1)-th candidate state had equal values)
    and src_ties (targets whose best value came from more than one source); Q, qbits and pbits (the pair (h, q) as the integer
    h << qbits | q, qbits = bits_of(Q), pbits = qbits + bits_of(H)); cuts, one (b, t, last pair taken, first pair dropped) per
    tie cut; tied, one (b, t, target pair, sorted source pairs at the best value) per source tie; select, per utterance and frame
    the record of tests/beam_decode_ref.py::select_info (the width `rem` of the key select and the exit it takes), the pairs as
    the integers h << qbits | q.
    Two hooks for the tests that ask whether an input can tell a wrong kernel from a right one; the defaults are the
    specification.  `rank`: pairs order by rank(h << qbits | q) instead of by (h, q), wherever pairs are compared (the cut, the
    source of a target, the winning end; `rank_where` names those of the three that use it).  Two pairs that the wrong rank cannot
    tell apart come out in REVERSED true order: one representative of what a kernel that ignores those bits may do.  Where the
    bits ignored are the last of the pair (9 bits: the second digit is bit 0) the bite of the hook rests on that choice alone.
    `max_backoff`: an LM walk of more backoff steps than this rejects."""
    x = np.asarray(inputs)
    T, B, N = x.shape
    dt = x.dtype.type
    K = int(beam_size)
    theta = dt(beam_threshold)
    assert K >= 1 and theta >= 0
    tr = np.asarray(transition).astype(dt)
    g = lexicon.graph
    sep = int(lexicon.separator)
    wos = np.asarray(lexicon.word_of_state, np.int64)
    nxt = np.asarray(g.next, np.int64)
    present, arcw, finw = fold(nxt, g.weight, g.final, dt, 1.0, token_score)
    label, state, src, tgt, Q = product(nxt, present)
    ninf = dt(-np.inf)
    start_w = np.where(present[0, label] & (nxt[0, label] == state), arcw[0, label], ninf).astype(dt)
    out_edges = [[] for _ in range(Q)]                     # per source: (target, weight)
    for s_, t_ in zip(src, tgt):
        out_edges[s_].append((int(t_), arcw[state[s_], label[t_]]))
    lw, bw, ew = fold_lm(lm, dt, lm_weight, word_score)
    row, word, lnext, backoff = (np.asarray(a, np.int64) for a in (lm.row, lm.word, lm.next, lm.backoff))
    qbits = max(1, int(Q - 1).bit_length())
    pbits = qbits + max(1, int(len(backoff) - 1).bit_length())
    plain = lambda p: p                                    # noqa: E731
    # (two pairs that a wrong rank cannot tell apart come out in the wrong order)
    wrong = plain if rank is None else (lambda p: (rank(p[0] << qbits | p[1]), -p[0], -p[1]))
    rk_cut, rk_src, rk_end = (wrong if n in rank_where else plain for n in ("cut", "source", "end"))

    def step(h, w):
        a = dt(0)
        n = 0
        while True:
            lo, hi = row[h], row[h + 1]
            k = lo + np.searchsorted(word[lo:hi], w)
            if k < hi and word[k] == w:
                return int(lnext[k]), dt(a + lw[k])
            if backoff[h] < 0 or (max_backoff is not None and n >= max_backoff):
                return None
            a = dt(a + bw[h])
            h = int(backoff[h])
            n += 1

    lens = _clamped_lengths(input_lengths, T, B)
    res = {"scores": np.full(B, -np.inf, dt), "token_lengths": np.zeros(B, np.int64), "word_lengths": np.zeros(B, np.int64)}
    for n in ("path", "tokens", "states", "lm_states", "words"):
        res[n] = np.full((B, T), -1, np.int64)
    if info is not None:
        info.update(sizes=[], cands=[], kept=[], tie_cuts=0, src_ties=0, Q=Q, qbits=qbits, pbits=pbits, cuts=[], tied=[],
                    select=[], out_degree=[len(e) for e in out_edges], sep_q=[q for q in range(Q) if state[q] == 0])
    at = [0, 0]                                            # (b, t) of the frame in hand, for info

    def prune(cand):
        """{pair: c} -> the kept list [(pair, c)]."""
        items = [(p, c) for p, c in cand.items() if c > ninf]
        if info is not None:
            info["select"][-1].append(select_info(np.array([p[0] << qbits | p[1] for p, _ in items], np.int64),
                                                  np.array([c for _, c in items], dt), K, theta))
        if not items:
            return []
        lo = dt(max(c for _, c in items) - theta)
        items = [it for it in sorted(items, key=lambda it: (-it[1], rk_cut(it[0]))) if it[1] >= lo]
        if info is not None and len(items) > K and items[K - 1][1] == items[K][1]:
            info["tie_cuts"] += 1
            info["cuts"].append((at[0], at[1], items[K - 1][0], items[K][0]))
        return items[:K]

    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            L = int(lens[b])
            sizes, ncand, keptl = [], [], []
            if info is not None:
                info["select"].append([])
            if L == 0 or Q == 0:
                if info is not None:
                    info["sizes"].append(sizes), info["cands"].append(ncand), info["kept"].append(keptl)
                continue
            xb = x[:, b]
            at[:] = b, 0
            cand = {(lm.start, q): dt(start_w[q] + xb[0, label[q]]) for q in range(Q) if start_w[q] > ninf}
            A = prune(cand)
            back = [{p: None for p, _ in A}]
            sizes.append(len(A)), ncand.append(len(cand)), keptl.append(sorted(p for p, _ in A))
            for t in range(1, L):
                best = {}                                    # target pair -> [value, source pair, sources at that value]
                nc = 0

                def offer(tp, c, sp):
                    cur = best.get(tp)
                    if cur is None or c > cur[0]:
                        best[tp] = [c, sp, 1, [sp]]
                    elif c == cur[0]:
                        cur[2] += 1
                        cur[3].append(sp)
                        if rk_src(sp) < rk_src(cur[1]):
                            cur[1] = sp
                for (h, q), v in A:
                    j = label[q]
                    c = dt(v + tr[j, j])
                    if c > ninf:
                        nc += 1
                        offer((h, q), c, (h, q))
                    for q2, w_e in out_edges[q]:
                        i = label[q2]
                        c = dt(dt(v + tr[i, j]) + w_e)
                        h2 = h
                        if i == sep:
                            st = step(h, int(wos[state[q]]))
                            if st is None:
                                continue
                            h2 = st[0]
                            c = dt(c + st[1])
                        if c > ninf:
                            nc += 1
                            offer((h2, q2), c, (h, q))
                if info is not None:
                    info["src_ties"] += sum(1 for v_ in best.values() if v_[2] > 1)
                    info["tied"] += [(b, t, tp, sorted(v_[3])) for tp, v_ in best.items() if v_[2] > 1]
                at[:] = b, t
                A = prune({tp: dt(v_[0] + xb[t, label[tp[1]]]) for tp, v_ in best.items()})
                back.append({p: best[p][1] for p, _ in A})
                sizes.append(len(A)), ncand.append(nc), keptl.append(sorted(p for p, _ in A))
            if info is not None:
                info["sizes"].append(sizes), info["cands"].append(ncand), info["kept"].append(keptl)
            win = None                                        # (end, pair, final word or -1)
            for (h, q), v in A:
                s = state[q]
                fw = -1
                if s == 0:
                    endw = ew[h]
                elif wos[s] >= 0:
                    st = step(h, int(wos[s]))
                    if st is None:
                        continue
                    endw = dt(st[1] + ew[st[0]])
                    fw = int(wos[s])
                else:
                    continue
                e = dt(dt(v + finw[s]) + endw)
                if e > ninf and (win is None or e > win[0] or (e == win[0] and rk_end((h, q)) < rk_end(win[1]))):
                    win = (e, (h, q), fw)
            if win is None:
                continue
            res["scores"][b] = win[0]
            p = win[1]
            pairs = [None] * L
            for t in range(L - 1, -1, -1):
                pairs[t] = p
                p = back[t][p]
            wl = []
            for t in range(L):
                h, q = pairs[t]
                res["path"][b, t], res["states"][b, t], res["lm_states"][b, t] = label[q], state[q], h
                if t >= 1 and pairs[t][1] != pairs[t - 1][1] and label[q] == sep:
                    wl.append(int(wos[state[pairs[t - 1][1]]]))
            if win[2] >= 0:
                wl.append(win[2])
            res["words"][b, :len(wl)] = wl
            res["word_lengths"][b] = len(wl)
            pl = res["path"][b, :L]
            keep = np.ones(L, bool)
            keep[1:] = pl[1:] != pl[:-1]
            tk = pl[keep]
            res["tokens"][b, :len(tk)] = tk
            res["token_lengths"][b] = len(tk)
    return res
