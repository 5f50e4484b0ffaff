"""Test-only numpy restatement of beam decoding with a lexicon, a word n-gram LM and LM LOOK-AHEAD
(`torch_asg_amd.beam_decode_words(..., lookahead=)`), written from the specification
(include/asg_hip.h::asg_beam_decode_words_la) and not from the package: no ranks, no sorted rows, no table.  The words below a
trie node are a set, E(s, n) is a plain loop over the arcs of row s, and LA walks the backoff chain as the header writes it.
Folding and product states are those of tests/beam_word_ref.py (`fold_lm`) and tests/graph_decode_ref.py (`fold`, `product`);
the search is beam_word_ref's loop with the look-ahead terms added where the header adds them.
"""
import numpy as np

from beam_word_ref import fold_lm
from graph_decode_ref import _clamped_lengths, fold, product


def words_below(lexicon):
    """Per trie node the set of words that end at it or below it (the separator arcs lead back to the root and are no tree
    edges)."""
    nxt = np.asarray(lexicon.graph.next, np.int64)
    wos = np.asarray(lexicon.word_of_state, np.int64)
    sep = int(lexicon.separator)
    S = nxt.shape[0]
    below = [None] * S

    def visit(n):
        s = {int(wos[n])} if wos[n] >= 0 else set()
        for x in range(nxt.shape[1]):
            if x != sep and nxt[n, x] >= 0:
                s |= visit(int(nxt[n, x]))
        below[n] = s
        return s
    visit(0)
    return below


def truncated_state(lm, order, whole_arrays=None):
    """la_state [H]: h backed off until at most order - 1 backoff steps remain to a state without a backoff.  `whole_arrays`
    chooses between the plain loop and the same states computed whole arrays at a time (default: above 4096 states, for LMs
    of millions of states; tests/test_beam_word_regimes_cpu.py holds the two forms to each other)."""
    backoff = np.asarray(lm.backoff, np.int64)
    if len(backoff) > 4096 if whole_arrays is None else whole_arrays:
        depth = np.where(backoff < 0, 0, -1)
        while (depth < 0).any():
            todo = depth < 0
            d = depth[backoff[todo]]
            depth[todo] = np.where(d >= 0, d + 1, -1)
        out = np.arange(len(backoff))
        while (depth[out] > order - 1).any():
            out = np.where(depth[out] > order - 1, backoff[out], out)
        return out.tolist()

    def depth(h):
        d = 0
        while backoff[h] >= 0:
            h, d = int(backoff[h]), d + 1
        return d
    out = []
    for h in range(len(backoff)):
        while depth(h) > order - 1:
            h = int(backoff[h])
        out.append(h)
    return out


# A test module that runs many restatements over one large lexicon and LM may lend them a dict for the time it runs (a fixture
# of tests/test_hip_beam_word_regimes.py does): (lexicon, LM, order, dtype, folded weights) -> the memos of E and L, with the two
# objects kept alive beside them so that their ids stay theirs.  None: every Look has its own memos.
shared_memos = None


class Look:
    """E, LA and L of the header by plain loops, in dtype dt with the folded weights lw / bw."""

    def __init__(self, lexicon, lm, order, dt, lw, bw):
        assert order >= 1
        self.dt = dt
        self.below = words_below(lexicon)
        self.la_state = truncated_state(lm, order)
        self.row, self.word, self.backoff = (np.asarray(a, np.int64) for a in (lm.row, lm.word, lm.backoff))
        self.lw, self.bw = lw, bw
        self.memo, self.ememo = {}, {}
        if shared_memos is not None:
            key = (id(lexicon), id(lm), int(order), np.dtype(dt).str, hash(np.asarray(lw).tobytes()), hash(np.asarray(bw).tobytes()))
            self.memo, self.ememo, _, _ = shared_memos.setdefault(key, (self.memo, self.ememo, lexicon, lm))

    def E(self, s, n):
        if (s, n) in self.ememo:                            # (a row of thousands of arcs is looped over once per node)
            return self.ememo[s, n]
        dt = self.dt
        best = dt(-np.inf)
        for k in range(self.row[s], self.row[s + 1]):
            if int(self.word[k]) in self.below[n]:
                x = dt(self.lw[k] + dt(0))                  # (-0 counts as +0)
                if x > best:
                    best = x
        self.ememo[s, n] = best
        return best

    def LA(self, s, n):
        dt = self.dt
        r, a = dt(-np.inf), dt(0)
        while True:
            x = dt(a + self.E(s, n))
            if x > r:
                r = x
            if self.backoff[s] < 0:
                return r
            a = dt(a + self.bw[s])
            s = int(self.backoff[s])

    def L(self, h, n):
        if n == 0:
            return self.dt(0)
        key = (self.la_state[h], n)
        if key not in self.memo:
            self.memo[key] = self.LA(*key)
        return self.memo[key]


def beam_word_la_ref(inputs, transition, lexicon, lm, order, input_lengths=None, beam_size=1, beam_threshold=np.inf,
                     lm_weight=1.0, word_score=0.0, token_score=0.0, info=None):
    """The arguments of beam_word_ref plus `order` -> its dict of eight outputs.  `info`, if a dict, receives what
    beam_word_ref's does, plus dead (candidates dropped because the look-ahead of their target is -inf)."""
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
    out_edges = [[] for _ in range(Q)]
    for s_, t_ in zip(src, tgt):
        out_edges[s_].append((int(t_), arcw[state[s_], label[t_]]))
    lw, bw, ew = fold_lm(lm, dt, lm_weight, word_score)
    row, word, lnext, backoff = (np.asarray(a, np.int64) for a in (lm.row, lm.word, lm.next, lm.backoff))
    look = Look(lexicon, lm, int(order), dt, lw, bw)

    def step(h, w):
        a = dt(0)
        while True:
            lo, hi = row[h], row[h + 1]
            k = lo + np.searchsorted(word[lo:hi], w)
            if k < hi and word[k] == w:
                return int(lnext[k]), dt(a + lw[k])
            if backoff[h] < 0:
                return None
            a = dt(a + bw[h])
            h = int(backoff[h])

    lens = _clamped_lengths(input_lengths, T, B)
    res = {"scores": np.full(B, -np.inf, dt), "token_lengths": np.zeros(B, np.int64), "word_lengths": np.zeros(B, np.int64)}
    for n in ("path", "tokens", "states", "lm_states", "words"):
        res[n] = np.full((B, T), -1, np.int64)
    if info is not None:
        info.update(sizes=[], cands=[], kept=[], tie_cuts=0, src_ties=0, dead=0)

    def prune(cand):
        items = [(p, c) for p, c in cand.items() if c > ninf]
        if not items:
            return []
        lo = dt(max(c for _, c in items) - theta)
        items = [it for it in sorted(items, key=lambda it: (-it[1], it[0])) if it[1] >= lo]
        if info is not None and len(items) > K and items[K - 1][1] == items[K][1]:
            info["tie_cuts"] += 1
        return items[:K]

    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            L = int(lens[b])
            sizes, ncand, keptl = [], [], []
            if L == 0 or Q == 0:
                if info is not None:
                    info["sizes"].append(sizes), info["cands"].append(ncand), info["kept"].append(keptl)
                continue
            xb = x[:, b]
            cand = {(lm.start, q): dt(dt(start_w[q] + look.L(lm.start, state[q])) + xb[0, label[q]])
                    for q in range(Q) if start_w[q] > ninf}
            A = prune(cand)
            back = [{p: None for p, _ in A}]
            sizes.append(len(A)), ncand.append(len(cand)), keptl.append(sorted(p for p, _ in A))
            for t in range(1, L):
                best = {}
                nc = 0

                def offer(tp, c, sp):
                    cur = best.get(tp)
                    if cur is None or c > cur[0]:
                        best[tp] = [c, sp, 1]
                    elif c == cur[0]:
                        cur[2] += 1
                        if sp < cur[1]:
                            cur[1] = sp
                for (h, q), v in A:
                    j = label[q]
                    ls = look.L(h, state[q])
                    assert ls > ninf                          # the look-ahead of a kept pair is finite by construction
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
                            c = dt(c + dt(st[1] - ls))
                        else:
                            lt = look.L(h, state[q2])
                            if not lt > ninf:
                                if info is not None:
                                    info["dead"] += 1
                                continue
                            c = dt(c + dt(lt - ls))
                        if c > ninf:
                            nc += 1
                            offer((h2, q2), c, (h, q))
                if info is not None:
                    info["src_ties"] += sum(1 for v_ in best.values() if v_[2] > 1)
                A = prune({tp: dt(v_[0] + xb[t, label[tp[1]]]) for tp, v_ in best.items()})
                back.append({p: best[p][1] for p, _ in A})
                sizes.append(len(A)), ncand.append(nc), keptl.append(sorted(p for p, _ in A))
            if info is not None:
                info["sizes"].append(sizes), info["cands"].append(ncand), info["kept"].append(keptl)
            win = None
            for (h, q), v in A:
                s = state[q]
                fw = -1
                if s == 0:
                    endw = ew[h]
                elif wos[s] >= 0:
                    st = step(h, int(wos[s]))
                    if st is None:
                        continue
                    ls = look.L(h, s)
                    assert ls > ninf
                    endw = dt(dt(st[1] - ls) + ew[st[0]])
                    fw = int(wos[s])
                else:
                    continue
                e = dt(dt(v + finw[s]) + endw)
                if e > ninf and (win is None or e > win[0] or (e == win[0] and (h, q) < win[1])):
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
