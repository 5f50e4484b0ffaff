"""Test-only numpy restatement of the beam-pruned full score over the pairs of the word decoder and of its gradients
(`torch_asg_amd.beam_words_full_score`, `beam_words_asg_loss`), written from the specification
(include/asg_hip.h::asg_beam_words_full_forward) and not from the kernels.

Step 1, the kept sets A_t, comes from tests/beam_word_ref.py (`beam_word_ref(..., info=)`, in the dtype of the emissions).
Steps 2-4 in float64 with the weights folded in the emissions' dtype and then widened: the forced pairs of the merged target,
the lattice U_t = A_t | F_t as sorted lists of (h, q), alpha / beta / posteriors over it with plain loops over a pair's own
candidates -- the stay, the lexicon edges, the LM walk on a separator edge.
"""
import numpy as np

from beam_word_ref import beam_word_ref, fold_lm
from graph_decode_ref import _clamped_lengths, fold, product


def _lse(vals):
    vals = [v for v in vals if v > -np.inf]
    if not vals:
        return -np.inf
    m = max(vals)
    return m + np.log(sum(np.exp(v - m) for v in vals))


class WordModel:
    """The lexicon's product graph and the folded LM, as the specification reads them; float64 copies of weights folded in dt."""

    def __init__(self, lexicon, lm, dt, lm_weight=1.0, word_score=0.0, token_score=0.0):
        g = lexicon.graph
        self.lm = lm
        self.num_tokens = int(g.N)
        self.sep = int(lexicon.separator)
        self.wos = np.asarray(lexicon.word_of_state, np.int64)
        nxt = np.asarray(g.next, np.int64)
        present, arcw, finw = fold(nxt, g.weight, g.final, dt, 1.0, token_score)
        self.label, self.state, src, tgt, self.Q = product(nxt, present)
        ninf = -np.inf
        self.start_w = np.where(present[0, self.label] & (nxt[0, self.label] == self.state), arcw[0, self.label], ninf).astype(np.float64)
        self.finw = np.asarray(finw, np.float64)
        self.out = [[] for _ in range(self.Q)]                 # per source q: (target q, folded weight)
        for s_, t_ in zip(src, tgt):
            self.out[s_].append((int(t_), float(arcw[self.state[s_], self.label[t_]])))
        lw, bw, ew = fold_lm(lm, dt, lm_weight, word_score)
        self.lw, self.bw, self.ew = (np.asarray(a, np.float64) for a in (lw, bw, ew))
        self.row, self.word, self.lnext, self.backoff = (np.asarray(a, np.int64) for a in (lm.row, lm.word, lm.next, lm.backoff))
        self._steps = {}

    def step(self, h, w):
        key = (h, w)
        if key not in self._steps:
            self._steps[key] = self._step(h, w)
        return self._steps[key]

    def _step(self, h, w):
        if w < 0:
            return None
        a = 0.0
        while True:
            lo, hi = self.row[h], self.row[h + 1]
            k = lo + np.searchsorted(self.word[lo:hi], w)
            if k < hi and self.word[k] == w:
                return int(self.lnext[k]), a + self.lw[k]
            if self.backoff[h] < 0:
                return None
            a = a + self.bw[h]
            h = int(self.backoff[h])

    def edges(self, p):
        """The candidates out of pair p: [(target pair, w, label of the target)], the stay first."""
        h, q = p
        res = [(p, 0.0, int(self.label[q]))]
        for q2, w in self.out[q]:
            i = int(self.label[q2])
            if i == self.sep:
                st = self.step(h, int(self.wos[self.state[q]]))
                if st is None:
                    continue
                res.append(((st[0], q2), w + st[1], i))
            else:
                res.append(((h, q2), w, i))
        return res

    def endw(self, p):
        """final_w[q] + endw(p), -inf where the pair has no end."""
        h, q = p
        s = int(self.state[q])
        if s == 0:
            return self.finw[s] + self.ew[h]
        if self.wos[s] < 0:
            return -np.inf
        st = self.step(h, int(self.wos[s]))
        if st is None:
            return -np.inf
        return self.finw[s] + (st[1] + self.ew[st[0]])

    def walk(self, y):
        """The merged target y -> (pairs p_1 .. p_n, lexicon + LM score with the end terms) or ([], -inf)."""
        pairs, h, q, prev, s = [], int(self.lm.start), None, None, 0.0
        for v in y:
            v = int(v)
            if v == prev:
                continue
            if v < 0 or v >= self.num_tokens:
                return [], -np.inf
            if q is None:
                cand = [q2 for q2 in range(self.Q) if self.start_w[q2] > -np.inf and self.label[q2] == v]
                if not cand:
                    return [], -np.inf
                q2 = cand[0]
                s = self.start_w[q2]
            else:
                hit = [(q2, w) for q2, w in self.out[q] if self.label[q2] == v]
                if not hit:
                    return [], -np.inf
                q2, w = hit[0]
                if v == self.sep:
                    st = self.step(h, int(self.wos[self.state[q]]))
                    if st is None:
                        return [], -np.inf
                    h, w = st[0], w + st[1]
                s = s + w
            pairs.append((h, q2))
            q, prev = q2, v
        if not pairs:
            return [], -np.inf
        e = self.endw(pairs[-1])
        if e == -np.inf:
            return [], -np.inf
        return pairs, s + e


def word_model(lexicon, lm, dt, lm_weight=1.0, word_score=0.0, token_score=0.0):
    return WordModel(lexicon, lm, dt, lm_weight, word_score, token_score)


def forced_sets(m, y, L):
    """The F_t of one utterance: y the raw target cut to its length, L frames -> list of L sorted lists of pairs."""
    empty = [[] for _ in range(L)]
    if len(y) == 0 or len(y) > L:
        return empty
    pairs, _ = m.walk(y)
    n = len(pairs)
    if n == 0:
        return empty
    return [sorted({pairs[k - 1] for k in range(1, n + 1) if k - 1 <= t and n - k <= L - 1 - t}) for t in range(L)]


def lattice(m, x, tr, L, U):
    """alpha / beta over the lattice U (list of L sorted lists of pairs) in float64 -> (Z, dZ/dx [T,N], dZ/dtr [N,N])."""
    T, N = x.shape
    gx, gtr = np.zeros((T, N)), np.zeros((N, N))
    if L == 0:
        return -np.inf, gx, gtr
    lab = m.label
    start = int(m.lm.start)
    alpha = [{p: (m.start_w[p[1]] + x[0, lab[p[1]]] if p[0] == start else -np.inf) for p in U[0]}]
    edges = [None]
    for t in range(1, L):
        inc = {p: [] for p in U[t]}
        ed = []
        for p in U[t - 1]:
            a = alpha[t - 1][p]
            for p2, w, i in m.edges(p):
                if p2 in inc:
                    ed.append((p, p2, w, i))
                    if a > -np.inf:
                        inc[p2].append((a + tr[i, lab[p[1]]]) + w)
        edges.append(ed)
        alpha.append({p: _lse(c) + x[t, lab[p[1]]] for p, c in inc.items()})
    Z = _lse([alpha[L - 1][p] + m.endw(p) for p in U[L - 1]])
    if Z == -np.inf:
        return Z, gx, gtr
    beta = [None] * L
    beta[L - 1] = {p: m.endw(p) for p in U[L - 1]}
    for t in range(L - 1, 0, -1):
        out = {p: [] for p in U[t - 1]}
        for p, p2, w, i in edges[t]:
            out[p].append(((beta[t][p2] + tr[i, lab[p[1]]]) + w) + x[t, i])
        beta[t - 1] = {p: _lse(c) for p, c in out.items()}
    for t in range(L):
        for p in U[t]:
            v = alpha[t][p] + beta[t][p] - Z
            if v > -np.inf:
                gx[t, lab[p[1]]] += np.exp(v)
    for t in range(1, L):
        for p, p2, w, i in edges[t]:
            v = alpha[t - 1][p] + tr[i, lab[p[1]]] + w + x[t, i] + beta[t][p2] - Z
            if v > -np.inf:
                gtr[i, lab[p[1]]] += np.exp(v)
    return Z, gx, gtr


def lattice_sets(inputs, transition, lexicon, lm, input_lengths=None, beam_size=1, beam_threshold=np.inf, lm_weight=1.0,
                 word_score=0.0, token_score=0.0, targets=None, target_lengths=None, info=None):
    """-> (model, lens, A, F, U): per utterance the lists of the frames' kept, forced and lattice sets (sorted lists of pairs)."""
    xs = np.asarray(inputs)
    dt = xs.dtype.type
    T, B, N = xs.shape
    lens = _clamped_lengths(input_lengths, T, B)
    inf = {}
    res = beam_word_ref(xs, np.asarray(transition).astype(dt), lexicon, lm, input_lengths, beam_size, beam_threshold, lm_weight,
                        word_score, token_score, info=inf)
    if info is not None:
        info.update(inf)
        info["decode"] = res
    m = word_model(lexicon, lm, dt, lm_weight, word_score, token_score)
    if targets is not None:
        tg = np.asarray(targets)
        S = tg.shape[1]
        tls = np.full(B, S) if target_lengths is None else np.clip(np.asarray(target_lengths), 0, S)
    As, Fs, Us = [], [], []
    for b in range(B):
        L = int(lens[b])
        A = [list(k) for k in inf["kept"][b]]
        A += [[] for _ in range(L - len(A))]
        F = forced_sets(m, tg[b, :int(tls[b])], L) if targets is not None else [[] for _ in range(L)]
        As.append(A), Fs.append(F), Us.append([sorted(set(a) | set(f)) for a, f in zip(A, F)])
    return m, lens, As, Fs, Us


def beam_word_loss_ref(inputs, transition, lexicon, lm, input_lengths=None, beam_size=1, beam_threshold=np.inf, lm_weight=1.0,
                       word_score=0.0, token_score=0.0, targets=None, target_lengths=None, grad_scores=None, info=None, sets=None):
    """inputs [T,B,N] (their dtype is the search's dtype) -> (Z_K [B], grad_inputs [T,B,N], grad_transition [N,N], U) with U[b]
    the list of the utterance's U_t.  `info`, if a dict, receives beam_word_ref's info and its result under 'decode'.  `sets`:
    a `lattice_sets` result to use instead of running the search (frozen sets for finite differences)."""
    xs = np.asarray(inputs)
    T, B, N = xs.shape
    x = xs.astype(np.float64)
    tr = np.asarray(transition, np.float64)
    if sets is None:
        sets = lattice_sets(xs, transition, lexicon, lm, input_lengths, beam_size, beam_threshold, lm_weight, word_score,
                            token_score, targets, target_lengths, info)
    m, lens, _, _, Us = sets
    g = np.ones(B) if grad_scores is None else np.asarray(grad_scores, np.float64)
    Z, gx, gtr = np.zeros(B), np.zeros((T, B, N)), np.zeros((N, N))
    for b in range(B):
        Z[b], gxb, gtb = lattice(m, x[:, b], tr, int(lens[b]), Us[b])
        gx[:, b] = g[b] * gxb
        gtr += g[b] * gtb
    return Z, gx, gtr, Us


def words_target_scores_ref(lexicon, lm, targets, target_lengths=None, dt=np.float64, lm_weight=1.0, word_score=0.0,
                            token_score=0.0):
    """[B]: asg_words_target_scores restated."""
    m = word_model(lexicon, lm, dt, lm_weight, word_score, token_score)
    tg = np.asarray(targets)
    B, S = tg.shape
    tls = np.full(B, S) if target_lengths is None else np.clip(np.asarray(target_lengths), 0, S)
    return np.array([m.walk(tg[b, :int(tls[b])])[1] for b in range(B)], np.float64)
