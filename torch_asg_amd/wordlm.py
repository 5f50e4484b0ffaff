"""Host objects of beam decoding with a lexicon and a word n-gram LM composed on the fly (`torch_asg_amd.beam_decode_words`,
include/asg_hip.h::asg_beam_decode_words).

A `Lexicon` is the trie automaton of `TokenGraph.from_lexicon` together with the word that ends at each trie node.  A `WordLM`
is a backoff automaton over word ids: H history states (state 0 the empty history), per state a row of explicit arcs
(word ascending, log-probability, next state), a backoff state with its weight, and the resolved log-probability of the end of
the sentence.  `WordLM.step(h, w)` is the walk the device runs on every separator edge.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .graph import TokenGraph, _host, abi_graph_beam

_LN10 = float(np.log(np.float64(10.0)))
MAX_PAIR_INDEX = 1 << 25            # H and Q of asg_beam_decode_words: (pair, slot) packs into one 64-bit word


class Lexicon:
    """A list of word spellings over the tokens of an ASG model, as the trie of `TokenGraph.from_lexicon` (`.graph`, built from
    the same arguments) plus `.word_of_state` [S] int64: the id of the word that ends at a trie node, -1 elsewhere.  `word_ids`
    (default range(len(spellings))) are the ids the word LM knows the spellings by.  Two words with one spelling raise
    ValueError: a word LM must be able to tell them apart, and the trie cannot."""

    def __init__(self, spellings, num_tokens, separator, word_scores=None, word_ids=None):
        spellings = [[int(x) for x in w] for w in spellings]
        self.graph = TokenGraph.from_lexicon(spellings, num_tokens, separator, word_scores)
        if word_ids is None:
            word_ids = range(len(spellings))
        word_ids = [int(w) for w in word_ids]
        if len(word_ids) != len(spellings):
            raise ValueError("Lexicon: %d word ids for %d spellings" % (len(word_ids), len(spellings)))
        if any(w < 0 for w in word_ids):
            raise ValueError("Lexicon: word ids must be >= 0")
        children = [{}]                 # the node numbering of TokenGraph.from_lexicon: order of first creation
        word_of = {}
        for toks, wid in zip(spellings, word_ids):
            node = 0
            for x in toks:
                nxt = children[node].get(x)
                if nxt is None:
                    nxt = len(children)
                    children[node][x] = nxt
                    children.append({})
                node = nxt
            if node in word_of:
                raise ValueError("Lexicon: words %d and %d share the spelling %s" % (word_of[node], wid, toks))
            word_of[node] = wid
        assert len(children) == self.graph.S
        self.word_of_state = np.full(self.graph.S, -1, np.int64)
        for node, wid in word_of.items():
            self.word_of_state[node] = wid
        self.separator = int(separator)
        self.num_words = len(spellings)
        self._compiled = {}

    def compile_words(self, device, dtype, token_score=0.0):
        """`graph.compile_beam(device, dtype, 1.0, token_score)` plus word_of_state as int32 on the device; cached."""
        base = self.graph.compile_beam(device, dtype, 1.0, token_score)
        device = base["label"].device
        key = (device, dtype, float(token_score))
        hit = self._compiled.get(key)
        if hit is None:
            hit = dict(base)
            hit["word_of_state"] = torch.from_numpy(self.word_of_state.astype(np.int32)).to(device)
            self._compiled[key] = hit
        return hit


class WordLM:
    """A backoff automaton over the word ids 0 .. V-1, from arrays: row [H+1], word [A] (ascending within a row), logp [A],
    next [A]; backoff [H] (-1: none; state 0 is the empty history and has none), bow [H]; start (the state after <s>);
    eos [H] (log-probability of </s> from each state with the backoff resolved, -inf if there is none)."""

    def __init__(self, num_words, row, word, logp, next, backoff, bow, start, eos):
        self.V = int(num_words)
        self.row = _host(row, np.int64)
        self.word = _host(word, np.int64)
        self.logp = _host(logp, np.float64)
        self.next = _host(next, np.int64)
        self.backoff = _host(backoff, np.int64)
        self.bow = _host(bow, np.float64)
        self.eos = _host(eos, np.float64)
        self.start = int(start)
        H, A = self.backoff.size, self.word.size
        self.H, self.A = H, A
        if self.V < 1 or H < 1 or H > MAX_PAIR_INDEX or A >= 1 << 31:
            raise ValueError("WordLM: V >= 1, 1 <= H <= 2^25 and A < 2^31 are required")
        if self.row.shape != (H + 1,) or self.row[0] != 0 or self.row[-1] != A or (np.diff(self.row) < 0).any():
            raise ValueError("WordLM: row must be [H+1] offsets into the %d arcs" % A)
        if self.logp.shape != (A,) or self.next.shape != (A,) or self.bow.shape != (H,) or self.eos.shape != (H,):
            raise ValueError("WordLM: logp, next must be [A] and backoff, bow, eos [H]")
        if ((self.word < 0) | (self.word >= self.V)).any() or ((self.next < 0) | (self.next >= H)).any():
            raise ValueError("WordLM: word must be in [0, V) and next in [0, H)")
        rid = np.repeat(np.arange(H), np.diff(self.row))
        if ((rid[1:] == rid[:-1]) & (self.word[1:] <= self.word[:-1])).any():
            raise ValueError("WordLM: word must ascend strictly within a row")
        if self.backoff[0] != -1 or ((self.backoff < -1) | (self.backoff >= H)).any():
            raise ValueError("WordLM: backoff[0] must be -1 and backoff in [-1, H)")
        # the backoff chain of every state must end: each step must lead to a state from which -1 is reached
        depth = np.where(self.backoff < 0, 0, -1)
        for _ in range(64):
            todo = depth < 0
            if not todo.any():
                break
            d = depth[self.backoff[todo]]
            depth[todo] = np.where(d >= 0, d + 1, -1)
        if (depth < 0).any():
            raise ValueError("WordLM: backoff chains must end within 64 steps")
        for a in (self.logp, self.bow, self.eos):
            if np.isnan(a).any() or (a == np.inf).any():
                raise ValueError("WordLM: weights must not hold NaN or +inf")
        if not 0 <= self.start < H:
            raise ValueError("WordLM: start must be in [0, %d)" % H)
        self._compiled = {}

    @classmethod
    def null(cls, num_words):
        """One state, every word with log-probability 0, eos = 0: decoding with it is decoding with the lexicon alone."""
        V = int(num_words)
        return cls(V, [0, V], np.arange(V), np.zeros(V), np.zeros(V, np.int64), [-1], [0.0], 0, [0.0])

    def find(self, h, w):
        """The arc of state h on word w, or -1."""
        lo, hi = int(self.row[h]), int(self.row[h + 1])
        k = lo + int(np.searchsorted(self.word[lo:hi], w))
        return k if k < hi and self.word[k] == w else -1

    def step(self, h, w):
        """(next state, log-probability in float64) of word w after state h, through the backoff; None if rejected."""
        a = 0.0
        h = int(h)
        while True:
            k = self.find(h, w)
            if k >= 0:
                return int(self.next[k]), a + float(self.logp[k])
            if self.backoff[h] < 0:
                return None
            a = a + float(self.bow[h])
            h = int(self.backoff[h])

    @classmethod
    def from_arpa(cls, text_or_path, vocabulary):
        """An ARPA language model of order 1 .. 4 over `vocabulary` (a list of words; word id = position).  Log10 values are
        scaled by ln 10 in float64.  N-grams that contain a word outside the vocabulary are dropped; <s> and </s> are kept (<s>
        only in front).  The states are the empty history (state 0) and every stored history -- every kept n-gram below the
        top order that does not end in </s>, and every context of a kept n-gram -- ordered by length, then by word ids (<s>
        before every word).  The next state of an n-gram is its longest suffix that is a stored history; the backoff of a
        state its longest proper suffix that is one.  start is the state of <s> (0 without one).  A vocabulary word without a
        unigram raises ValueError."""
        text = text_or_path
        if "\n" not in text and os.path.exists(text):
            with open(text) as f:
                text = f.read()
        vocab = {w: i for i, w in enumerate(vocabulary)}
        if len(vocab) != len(vocabulary):
            raise ValueError("WordLM.from_arpa: the vocabulary repeats a word")
        BOS, EOS = -1, len(vocab)                      # ids inside this function
        grams = {}                                     # tuple of ids -> (logp, bow or None)
        order, top = 0, 0
        for line in text.splitlines():
            line = line.strip()
            if not line or line == "\\data\\":
                continue
            if line.startswith("ngram ") and order == 0:
                top = max(top, int(line[6:].split("=")[0]))
                continue
            if line.startswith("\\") and line.endswith("-grams:"):
                order = int(line[1:-7])
                continue
            if line == "\\end\\":
                break
            if order == 0:
                continue
            f = line.split()
            if len(f) not in (order + 1, order + 2):
                raise ValueError("WordLM.from_arpa: cannot read %r as a %d-gram" % (line, order))
            ids = []
            for pos, w in enumerate(f[1:1 + order]):
                if w == "<s>":
                    ids.append(BOS if pos == 0 else None)
                elif w == "</s>":
                    ids.append(EOS if pos == order - 1 else None)
                else:
                    ids.append(vocab.get(w))
            if any(i is None for i in ids):
                continue
            grams[tuple(ids)] = (float(f[0]) * _LN10, float(f[order + 1]) * _LN10 if len(f) == order + 2 else None)
        if not 1 <= top <= 4 or any(len(g) > top for g in grams):
            raise ValueError("WordLM.from_arpa: orders 1 to 4 are read, the header says %d" % top)
        for w, i in vocab.items():
            if (i,) not in grams:
                raise ValueError("WordLM.from_arpa: no unigram for the vocabulary word %r" % w)
        hist = {()}
        for g in grams:
            if len(g) < top and g[-1] != EOS:
                hist.add(g)
            hist.add(g[:-1])
        hist = sorted(hist, key=lambda g: (len(g), g))
        index = {g: n for n, g in enumerate(hist)}

        def longest(g):
            while g not in index:
                g = g[1:]
            return index[g]
        H = len(hist)
        arcs = [[] for _ in range(H)]
        eos_x = {}
        for g, (lp, _) in grams.items():
            if g == (BOS,):
                continue
            if g[-1] == EOS:
                eos_x[index[g[:-1]]] = lp
            else:
                arcs[index[g[:-1]]].append((g[-1], lp, longest(g)))
        row = np.zeros(H + 1, np.int64)
        word, logp, nxt = [], [], []
        for n in range(H):
            for w, lp, nx in sorted(arcs[n]):
                word.append(w), logp.append(lp), nxt.append(nx)
            row[n + 1] = len(word)
        backoff = np.array([-1] + [longest(g[1:]) for g in hist[1:]], np.int64)
        bow = np.array([(grams.get(g, (0.0, None))[1] or 0.0) if g else 0.0 for g in hist], np.float64)
        eos = np.full(H, -np.inf)
        for n in range(H):
            a, h = np.float64(0.0), n
            while h not in eos_x and backoff[h] >= 0:
                a = a + bow[h]
                h = int(backoff[h])
            if h in eos_x:
                eos[n] = a + np.float64(eos_x[h])
        return cls(len(vocab), row, word, logp, nxt, backoff, bow, index.get((BOS,), 0), eos)

    def compile_host(self, dt, lm_weight=1.0, word_score=0.0):
        """The folded weights in dtype dt: lw [A] = fl(fl(lm_weight * logp) + word_score), bw [H] = fl(lm_weight * bow),
        ew [H] = fl(lm_weight * eos); -inf stays -inf."""
        dt = np.dtype(dt).type
        m, ws = dt(lm_weight), dt(word_score)
        if not (np.isfinite(m) and np.isfinite(ws)):
            raise ValueError("WordLM: lm_weight and word_score must be finite")
        ninf = dt(-np.inf)

        def scaled(a):
            with np.errstate(invalid="ignore", over="ignore"):
                return np.where(a == -np.inf, ninf, m * a.astype(dt)).astype(dt)
        with np.errstate(invalid="ignore", over="ignore"):
            lw = np.where(self.logp == -np.inf, ninf, scaled(self.logp) + ws).astype(dt)
        return {"lw": lw, "bw": scaled(self.bow), "ew": scaled(self.eos)}

    def compile(self, device, dtype, lm_weight=1.0, word_score=0.0):
        """The automaton on `device` for decoding in `dtype`, weights folded on the host, cached per (device, dtype,
        lm_weight, word_score): a dict of device tensors (row, word, next, backoff int32; lw, bw, ew) plus H, A, V, start."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if dtype not in (torch.float32, torch.float64):
            raise RuntimeError("torch_asg_amd: expected scalar type Float or Double but found %s" % dtype)
        key = (device, dtype, float(lm_weight), float(word_score))
        hit = self._compiled.get(key)
        if hit is not None:
            return hit
        host = self.compile_host(np.float32 if dtype == torch.float32 else np.float64, lm_weight, word_score)
        for name in ("row", "word", "next", "backoff"):
            host[name] = getattr(self, name).astype(np.int32)
        dev = {n: torch.from_numpy(a).to(device) for n, a in host.items()}
        dev["H"], dev["A"], dev["V"], dev["start"], dev["dtype"] = self.H, self.A, self.V, self.start, dtype
        self._compiled[key] = dev
        return dev


class WordLookahead:
    """LM look-ahead for `beam_decode_words(..., lookahead=)`: what lets a partial word be ranked by the best LM score any word
    below its trie node can still get, instead of by acoustics alone (include/asg_hip.h::asg_beam_decode_words_la).

    Ranks: the trie of `lexicon.graph` is walked in pre-order, children by ascending token; the word of a word-end node takes
    the next rank when the node is entered.  `rlo` / `rhi` [S] int32 are the counter on entry and on exit: the words below node
    n, its own included, have the ranks [rlo[n], rhi[n]).  `word_rank` [V] is the rank of a word, -1 for an LM word the lexicon
    does not spell.  Rows: the arcs of every LM state whose word has a rank, sorted by rank: offsets `krow` [H+1], ranks
    `krank` [A'] and `karc` [A'], the arc of the LM each one is.  `la_state` [H] int32 is h backed off until at most
    `order - 1` backoff steps remain to a state without a backoff (`depth`): order 1 is unigram smearing, an order at or above
    the LM's the full look-ahead.  E(s, n) is the largest folded arc weight of row s over the ranks of node n, -inf without
    one; `compile_host` builds the sparse table that answers it with two binary searches and two reads, `range_max` is that
    query on the host.

    order < 1 raises ValueError; so does a ranked word that has an arc in some row but none in a state without a backoff (an
    ARPA-built LM has state 0 as the only such state and every unigram in it): with that rule a look-ahead of -inf says that no
    word below the node is accepted, whatever the truncation."""

    def __init__(self, lexicon, word_lm, order=2):
        check_words(lexicon, word_lm)
        order = int(order)
        if order < 1:
            raise ValueError("WordLookahead: order must be >= 1")
        self.order = order
        self.S, self.H, self.V = lexicon.graph.S, word_lm.H, word_lm.V
        self._lm, self._lexicon = word_lm, lexicon
        nxt = np.asarray(lexicon.graph.next, np.int64)
        wos = lexicon.word_of_state
        sep = lexicon.separator
        S = self.S
        rlo, rhi = np.zeros(S, np.int32), np.zeros(S, np.int32)
        word_rank = np.full(self.V, -1, np.int64)
        count = 0
        stack = [(0, False)]
        while stack:
            n, leaving = stack.pop()
            if leaving:
                rhi[n] = count
                continue
            rlo[n] = count
            if wos[n] >= 0:
                word_rank[wos[n]] = count
                count += 1
            stack.append((n, True))
            kids = [int(nxt[n, x]) for x in np.flatnonzero(nxt[n] >= 0) if x != sep]
            stack.extend((c, False) for c in reversed(kids))
        self.rlo, self.rhi, self.word_rank, self.num_ranks = rlo, rhi, word_rank, count
        lm = word_lm
        rid = np.repeat(np.arange(lm.H), np.diff(lm.row))
        rank = word_rank[lm.word]
        arcs = np.flatnonzero(rank >= 0)
        arcs = arcs[np.argsort(rid[arcs] * (count + 1) + rank[arcs], kind="stable")]
        self.karc = arcs
        self.krank = rank[arcs].astype(np.int32)
        self.krow = np.concatenate([[0], np.cumsum(np.bincount(rid[arcs], minlength=lm.H))]).astype(np.int32)
        self.A = int(arcs.size)
        # every ranked word with an arc anywhere must have one in every state without a backoff
        seen = np.zeros(count + 1, bool)
        seen[self.krank] = True
        for s in np.flatnonzero(lm.backoff < 0):
            here = np.zeros(count + 1, bool)
            here[self.krank[self.krow[s]:self.krow[s + 1]]] = True
            if (seen & ~here).any():
                w = int(np.flatnonzero(word_rank == np.flatnonzero(seen & ~here)[0])[0])
                raise ValueError("WordLookahead: word %d has an arc in the LM but none in state %d, which has no backoff" % (w, s))
        depth = np.where(lm.backoff < 0, 0, -1)
        while (depth < 0).any():                     # (WordLM has checked that the chains end)
            todo = depth < 0
            d = depth[lm.backoff[todo]]
            depth[todo] = np.where(d >= 0, d + 1, -1)
        self.depth = depth
        la_state = np.arange(lm.H)
        while (depth[la_state] > order - 1).any():
            la_state = np.where(depth[la_state] > order - 1, lm.backoff[la_state], la_state)
        self.la_state = la_state.astype(np.int32)
        longest = int(np.diff(self.krow).max(initial=0))
        self.levels = max(1, longest.bit_length())   # tab[k] for 2^k <= the longest row
        self._compiled = {}

    def compile_host(self, dt, lm_weight=1.0, word_score=0.0):
        """tab [levels][A'] in dtype dt: tab[k][i] = the largest of `WordLM.compile_host`'s lw over the arcs i .. i + 2^k - 1 of
        the rank-ordered rows that lie in the row of i.  (-0 is stored as +0, so that a maximum is one bit pattern.)"""
        dt = np.dtype(dt).type
        lw = self._lm.compile_host(dt, lm_weight, word_score)["lw"]
        tab = np.full((self.levels, self.A), -np.inf, dt)
        tab[0] = lw[self.karc] + dt(0)
        end = np.repeat(self.krow[1:], np.diff(self.krow)).astype(np.int64)       # the end of each arc's row
        idx = np.arange(self.A)
        for k in range(1, self.levels):
            far = idx + (1 << (k - 1))
            ok = far < end
            tab[k] = tab[k - 1]
            tab[k, ok] = np.maximum(tab[k - 1, ok], tab[k - 1, far[ok]])
        return tab

    def dense_host(self, tab):
        """dense0 [S]: E(0, n) of every trie node from a `compile_host` table -- the empty history is where every backoff
        chain of an ARPA LM ends and has the longest row, so the device reads its answer instead of searching for it."""
        b0, b1 = int(self.krow[0]), int(self.krow[1])
        lo = b0 + np.searchsorted(self.krank[b0:b1], self.rlo)
        hi = b0 + np.searchsorted(self.krank[b0:b1], self.rhi)
        out = np.full(self.S, -np.inf, tab.dtype)
        ok = np.flatnonzero(lo < hi)
        k = np.floor(np.log2(hi[ok] - lo[ok])).astype(np.int64)
        out[ok] = np.maximum(tab[k, lo[ok]], tab[k, hi[ok] - (1 << k)])
        return out

    def range_max(self, tab, s, n):
        """E(s, n) from a `compile_host` table: two binary searches in row s of krank, two reads."""
        b0, b1 = int(self.krow[s]), int(self.krow[s + 1])
        lo = b0 + int(np.searchsorted(self.krank[b0:b1], self.rlo[n]))
        hi = b0 + int(np.searchsorted(self.krank[b0:b1], self.rhi[n]))
        if lo >= hi:
            return tab.dtype.type(-np.inf)
        k = (hi - lo).bit_length() - 1
        return max(tab[k, lo], tab[k, hi - (1 << k)])

    def compile(self, device, dtype, lm_weight=1.0, word_score=0.0):
        """The arrays on `device` for decoding in `dtype`, cached per (device, dtype, lm_weight, word_score) as `WordLM.compile`
        is: a dict of device tensors (rlo, rhi, la_state, krow, krank int32; tab, dense0) plus S, H, A, levels."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if dtype not in (torch.float32, torch.float64):
            raise RuntimeError("torch_asg_amd: expected scalar type Float or Double but found %s" % dtype)
        key = (device, dtype, float(lm_weight), float(word_score))
        hit = self._compiled.get(key)
        if hit is not None:
            return hit
        host = {n: getattr(self, n) for n in ("rlo", "rhi", "la_state", "krow", "krank")}
        host["tab"] = self.compile_host(np.float32 if dtype == torch.float32 else np.float64, lm_weight, word_score)
        host["dense0"] = self.dense_host(host["tab"])
        dev = {n: torch.from_numpy(np.ascontiguousarray(a)).to(device) for n, a in host.items()}
        dev["S"], dev["H"], dev["A"], dev["levels"], dev["dtype"] = self.S, self.H, self.A, self.levels, dtype
        self._compiled[key] = dev
        return dev


def check_lookahead(lookahead, lexicon, word_lm):
    """The argument checks of `lookahead=`: its type, and that it was built for this very lexicon and LM (its tables hold
    this LM's weights in this trie's ranks: another pair of equal shape would give wrong values without any error)."""
    if not isinstance(lookahead, WordLookahead):
        raise TypeError("torch_asg_amd: lookahead must be a torch_asg_amd.WordLookahead or None")
    if lookahead._lexicon is not lexicon or lookahead._lm is not word_lm:
        raise RuntimeError("torch_asg_amd: the look-ahead was built for another lexicon or word LM (%d lexicon states and %d LM "
                           "states; the call has %d and %d)" % (lookahead.S, lookahead.H, lexicon.graph.S, word_lm.H))


def abi_lookahead(la):
    """The asg_word_lookahead view of a `WordLookahead.compile` result (pointers into its tensors)."""
    s = _lib.AsgWordLookahead()
    s.S, s.H, s.A, s.levels = la["S"], la["H"], la["A"], la["levels"]
    s.dtype = _lib.ASG_DTYPE_F32 if la["dtype"] == torch.float32 else _lib.ASG_DTYPE_F64
    for name in ("rlo", "rhi", "la_state", "krow", "krank", "tab", "dense0"):
        t = la[name]
        setattr(s, name, ctypes.c_void_p(t.data_ptr() if t.numel() else None))
    return s


def abi_word_lm(lm, lex):
    """The asg_word_lm view of a `WordLM.compile` result and a `Lexicon.compile_words` result (pointers into their tensors)."""
    s = _lib.AsgWordLM()
    s.H, s.A, s.V, s.S = lm["H"], lm["A"], lm["V"], lex["word_of_state"].numel()
    s.start = lm["start"]
    s.dtype = _lib.ASG_DTYPE_F32 if lm["dtype"] == torch.float32 else _lib.ASG_DTYPE_F64
    for name in ("row", "word", "next", "backoff", "lw", "bw", "ew"):
        t = lm[name]
        setattr(s, name, ctypes.c_void_p(t.data_ptr() if t.numel() else None))
    s.word_of_state = ctypes.c_void_p(lex["word_of_state"].data_ptr())
    return s


def check_words(lexicon, word_lm):
    """The argument checks of a (lexicon, word LM) pair: their types, and that the LM knows every word of the lexicon.  Apart
    from `abi_words` because the callers report these before they look at the device."""
    if not isinstance(lexicon, Lexicon):
        raise TypeError("torch_asg_amd: lexicon must be a torch_asg_amd.Lexicon")
    if not isinstance(word_lm, WordLM):
        raise TypeError("torch_asg_amd: word_lm must be a torch_asg_amd.WordLM")
    wmax = int(lexicon.word_of_state.max(initial=-1))
    if wmax >= word_lm.V:
        raise RuntimeError("torch_asg_amd: the lexicon has word id %d but the word LM knows %d words" % (wmax, word_lm.V))


def abi_words(lexicon, word_lm, device, dtype, lm_weight, word_score, token_score):
    """A checked (`check_words`) pair compiled for (device, dtype) and the weights -> (the asg_token_graph_beam view of the
    lexicon, the asg_word_lm view, (the two compiled dicts the views point into: keep them alive with the views))."""
    lex = lexicon.compile_words(device, dtype, token_score)
    lm = word_lm.compile(device, dtype, lm_weight, word_score)
    w = abi_word_lm(lm, lex)
    w.separator = lexicon.separator
    return abi_graph_beam(lex), w, (lex, lm)
