"""Deterministic weighted automata over tokens, for Viterbi decoding of the ASG lattice composed with a token-level language
model (`torch_asg_amd.viterbi_decode_graph`, exact, and `torch_asg_amd.beam_decode_graph`, beam-pruned).

A `TokenGraph` is S states, a start state, next[S,N] (-1: no arc), weight[S,N] (log-score of emitting token i from state s;
-inf: no arc) and final[S] (-inf: not accepting).  `compile` folds the LM weight and the token insertion score into the arcs
in the decode dtype and builds the product graph the kernels read (include/asg_hip.h::asg_token_graph): the product states
q = (label i, state s') for which some arc s --i--> s' exists, sorted by (s', i), and per target q a CSR row of incoming edges
from every q' = (j, s) with j != i and next[s][i] == s', ascending by source index.
"""
import ctypes

import numpy as np
import torch

from . import _lib

_MAX_INDEX = (1 << 31) - 1


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.array(a, dtype=dtype)


class TokenGraph:
    """A deterministic weighted automaton over the N tokens of an ASG model; validated on the CPU when constructed."""

    def __init__(self, next, weight, final, start=0):
        nxt = _host(next, np.int64)
        w = _host(weight, np.float64)
        f = _host(final, np.float64)
        if nxt.ndim != 2 or nxt.shape[0] < 1 or nxt.shape[1] < 1:
            raise ValueError("TokenGraph: next must be [S,N] with S, N >= 1, got %s" % (nxt.shape,))
        S, N = nxt.shape
        if w.shape != (S, N):
            raise ValueError("TokenGraph: weight must be [%d,%d], got %s" % (S, N, w.shape))
        if f.shape != (S,):
            raise ValueError("TokenGraph: final must be [%d], got %s" % (S, f.shape))
        if N > (1 << 16) or S > _MAX_INDEX:
            raise ValueError("TokenGraph: at most 2^16 tokens and 2^31 - 1 states")
        if ((nxt < -1) | (nxt >= S)).any():
            raise ValueError("TokenGraph: next must hold states in [-1, %d)" % S)
        if np.isnan(w).any() or np.isnan(f).any():
            raise ValueError("TokenGraph: weight and final must not hold NaN")
        if (w == np.inf).any() or (f == np.inf).any():
            raise ValueError("TokenGraph: weight and final must not hold +inf")
        start = int(start)
        if not 0 <= start < S:
            raise ValueError("TokenGraph: start must be in [0, %d)" % S)
        self.next, self.weight, self.final, self.start = nxt, w, f, start
        self.S, self.N = S, N
        self._compiled = {}

    @classmethod
    def from_ngram(cls, logp):
        """An n-gram LM as an automaton.  logp is a dense table [N+1]*order (order 1..4): logp[c_1, .., c_{order-1}, x] is the
        log-probability of x after the context c_1 .. c_{order-1}.  Index N is sentence-start padding in the context axes
        and end-of-sentence in the last axis.  The states are the reachable contexts (the last order-1 tokens, padded on the
        left with N at the start): sum_{k<order} N^k of them, the all-padding one the start state.  final[ctx] =
        logp[ctx + (N,)]."""
        lp = _host(logp, np.float64)
        order = lp.ndim
        if not 1 <= order <= 4:
            raise ValueError("TokenGraph.from_ngram: order must be 1..4, got a %d-dimensional table" % order)
        N = lp.shape[0] - 1
        if N < 1 or any(d != N + 1 for d in lp.shape):
            raise ValueError("TokenGraph.from_ngram: logp must be [N+1]*order with N >= 1, got %s" % (lp.shape,))
        k = order - 1
        # reachable contexts: m padding symbols then k - m real tokens (m = k .. 0); a context is a tuple of k digits
        ctxs = []
        for m in range(k, -1, -1):
            real = np.indices((N,) * (k - m)).reshape(k - m, -1).T if k - m else np.zeros((1, 0), np.int64)
            pad = np.full((real.shape[0], m), N, np.int64)
            ctxs.append(np.concatenate([pad, real], axis=1))
        ctx = np.concatenate(ctxs, axis=0)                      # [S, k], the start context (all padding) first
        S = ctx.shape[0]
        base = (N + 1) ** np.arange(k - 1, -1, -1, dtype=np.int64) if k else np.zeros(0, np.int64)
        code = ctx @ base if k else np.zeros(1, np.int64)
        index = np.full((N + 1) ** k, -1, np.int64)
        index[code] = np.arange(S)
        tok = np.arange(N)
        if k:
            nctx = np.concatenate([np.repeat(ctx[:, 1:], N, axis=0), np.tile(tok, S)[:, None]], axis=1)
            nxt = index[nctx @ base].reshape(S, N)
        else:
            nxt = np.zeros((1, N), np.int64)
        flat = lp.reshape(-1, N + 1)                            # row = context code over (N+1)^k
        weight = flat[code][:, :N]
        final = flat[code][:, N]
        return cls(nxt, weight, final, 0)

    @classmethod
    def from_lexicon(cls, spellings, num_tokens, separator, word_scores=None):
        """A lexicon as an automaton: a trie of the spellings whose word ends return to the root on `separator`.  `spellings`
        is a list of non-empty token-id sequences without `separator`; `word_scores` one log-score per spelling (default 0;
        the largest one counts when a spelling occurs twice).  State 0 is the root and the start; the other trie nodes are
        numbered in order of first creation while the spellings are inserted in the given order; trie arcs weigh 0.  A node that
        ends a word has an arc on `separator` to the root that weighs the word's score, and is final with the same score; the
        root is final with 0 and has no `separator` arc; nothing else is final.  The lattice collapses repeated labels, so a
        spelling with two equal consecutive tokens raises ValueError (spell those with a repetition label)."""
        N, sep = int(num_tokens), int(separator)
        if N < 1 or not 0 <= sep < N:
            raise ValueError("TokenGraph.from_lexicon: separator must be in [0, %d)" % N)
        if word_scores is None:
            word_scores = [0.0] * len(spellings)
        if len(word_scores) != len(spellings):
            raise ValueError("TokenGraph.from_lexicon: %d scores for %d spellings" % (len(word_scores), len(spellings)))
        children = [{}]                 # per node: token -> node
        ends = {}                       # node -> score of the word that ends there
        for w, sc in zip(spellings, word_scores):
            toks = [int(x) for x in w]
            if not toks:
                raise ValueError("TokenGraph.from_lexicon: empty spelling")
            if any(x == sep or not 0 <= x < N for x in toks):
                raise ValueError("TokenGraph.from_lexicon: spelling %s has the separator or a token outside [0, %d)" % (toks, N))
            if any(a == b for a, b in zip(toks, toks[1:])):
                raise ValueError("TokenGraph.from_lexicon: spelling %s repeats a token; the lattice collapses repeats" % (toks,))
            node = 0
            for x in toks:
                nxt = children[node].get(x)
                if nxt is None:
                    nxt = len(children)
                    children[node][x] = nxt
                    children.append({})
                node = nxt
            sc = float(sc)
            ends[node] = max(ends[node], sc) if node in ends else sc
        S = len(children)
        nxt = np.full((S, N), -1, np.int64)
        weight = np.full((S, N), -np.inf)
        final = np.full(S, -np.inf)
        for s, ch in enumerate(children):
            for x, d in ch.items():
                nxt[s, x], weight[s, x] = d, 0.0
        for s, sc in ends.items():
            nxt[s, sep], weight[s, sep], final[s] = 0, sc, sc
        final[0] = 0.0
        return cls(nxt, weight, final, 0)

    def compile(self, device, dtype, lm_weight=1.0, token_score=0.0):
        """The product graph on `device` for decoding in `dtype` (float32 / float64), cached per
        (device, dtype, lm_weight, token_score).  A dict of device tensors plus Q and E; see the module docstring."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if dtype not in (torch.float32, torch.float64):
            raise RuntimeError("torch_asg_amd: expected scalar type Float or Double but found %s" % dtype)
        key = (device, dtype, float(lm_weight), float(token_score))
        hit = self._compiled.get(key)
        if hit is not None:
            return hit
        host = self.compile_host(np.float32 if dtype == torch.float32 else np.float64, lm_weight, token_score)
        dev = {n: torch.from_numpy(a).to(device) for n, a in host.items() if isinstance(a, np.ndarray)}
        dev["Q"], dev["E"], dev["N"] = host["Q"], host["E"], self.N
        dev["dtype"] = dtype
        self._compiled[key] = dev
        return dev

    def compile_host(self, dt, lm_weight=1.0, token_score=0.0):
        """The product graph as numpy arrays, weights folded in dtype `dt`:
        label, state, start_w, final_w [Q]; row [Q+1]; src, src_label, edge_w [E]."""
        dt = np.dtype(dt).type
        lw, ts = dt(lm_weight), dt(token_score)
        if not (np.isfinite(lw) and np.isfinite(ts)):
            raise ValueError("TokenGraph: lm_weight and token_score must be finite")
        S, N = self.S, self.N
        present = (self.next >= 0) & (self.weight != -np.inf)
        with np.errstate(invalid="ignore", over="ignore"):
            arcw = (lw * self.weight.astype(dt)).astype(dt) + ts        # two roundings in dt, no FMA
            finw = np.where(self.final == -np.inf, dt(-np.inf), lw * self.final.astype(dt)).astype(dt)
        s_a, i_a = np.nonzero(present)                                   # every arc s --i--> s'
        sp_a = self.next[s_a, i_a]
        qkey = np.unique(sp_a * N + i_a)                                 # product states, sorted by (s', i)
        Q = int(qkey.size)
        if Q > _MAX_INDEX:
            raise ValueError("TokenGraph: %d product states, at most 2^31 - 1" % Q)
        label = (qkey % N).astype(np.int64)
        state = (qkey // N).astype(np.int64)
        start_w = np.full(Q, -np.inf, dt)
        i0 = np.nonzero(present[self.start])[0]
        start_w[np.searchsorted(qkey, self.next[self.start, i0] * N + i0)] = arcw[self.start, i0]
        final_w = finw[state]
        # the product states of each automaton state form one contiguous range of q (sorted by state first)
        lo = np.searchsorted(state, np.arange(S), "left")
        hi = np.searchsorted(state, np.arange(S), "right")
        tgt_a = np.searchsorted(qkey, sp_a * N + i_a)                    # target of each arc
        cnt = hi[s_a] - lo[s_a]                                          # candidate sources of each arc: the q's of state s
        arc_of = np.repeat(np.arange(s_a.size), cnt)
        src = lo[s_a][arc_of] + (np.arange(arc_of.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        keep = label[src] != i_a[arc_of]                                 # j != i: a repeated label is a stay
        src, arc_of = src[keep], arc_of[keep]
        tgt = tgt_a[arc_of]
        order = np.lexsort((src, tgt))
        src, tgt, arc_of = src[order], tgt[order], arc_of[order]
        E = int(src.size)
        if E > _MAX_INDEX:
            raise ValueError("TokenGraph: %d product edges, at most 2^31 - 1" % E)
        row = np.zeros(Q + 1, np.int64)
        np.cumsum(np.bincount(tgt, minlength=Q), out=row[1:])
        i32 = np.int32
        return {"label": label.astype(i32), "state": state.astype(i32), "start_w": start_w, "final_w": final_w.astype(dt),
                "row": row.astype(i32), "src": src.astype(i32), "src_label": label[src].astype(i32),
                "edge_w": arcw[s_a[arc_of], i_a[arc_of]].astype(dt), "Q": Q, "E": E}

    def compile_loss(self, device, dtype, lm_weight=1.0, token_score=0.0):
        """What `compile` returns plus the arrays the loss kernels read (include/asg_hip.h::asg_token_graph_loss), cached apart
        from `compile`'s entry (which stays as it is, so the decoder pays nothing for them)."""
        base = self.compile(device, dtype, lm_weight, token_score)
        device = base["label"].device
        key = ("loss", device, dtype, float(lm_weight), float(token_score))
        hit = self._compiled.get(key)
        if hit is not None:
            return hit
        host = self.compile_loss_host(np.float32 if dtype == torch.float32 else np.float64, lm_weight, token_score)
        dev = dict(base)
        dev.update({n: torch.from_numpy(a).to(device) for n, a in host.items()})
        dev["S"], dev["start"] = self.S, self.start
        self._compiled[key] = dev
        return dev

    def compile_loss_host(self, dt, lm_weight=1.0, token_score=0.0):
        """The loss-only arrays as numpy arrays: tgt [E] (target of each incoming edge), orow [Q+1] and oedge [E] (the outgoing
        edges of each q as incoming-edge indices, ascending by (src, tgt)), lrow [N+1] and lq [Q] (the product states of each
        label, ascending), pkey int64 and pedge [E] (the edges sorted by label pair label[tgt] * N + src_label, stably), and the
        automaton for the target walk: next [S,N] (-1 where no arc), arcw [S,N] (-inf where no arc) and finw [S] in dtype dt."""
        h = self.compile_host(dt, lm_weight, token_score)
        dt = np.dtype(dt).type
        Q, N = h["Q"], self.N
        row = h["row"].astype(np.int64)
        src = h["src"].astype(np.int64)
        tgt = np.repeat(np.arange(Q, dtype=np.int64), np.diff(row))
        oedge = np.lexsort((tgt, src))
        orow = np.zeros(Q + 1, np.int64)
        np.cumsum(np.bincount(src, minlength=Q), out=orow[1:])
        label = h["label"].astype(np.int64)
        lq = np.argsort(label, kind="stable")
        lrow = np.zeros(N + 1, np.int64)
        np.cumsum(np.bincount(label, minlength=N), out=lrow[1:])
        pk = label[tgt] * N + h["src_label"].astype(np.int64)
        pedge = np.argsort(pk, kind="stable")
        lw, ts = dt(lm_weight), dt(token_score)
        present = (self.next >= 0) & (self.weight != -np.inf)
        with np.errstate(invalid="ignore", over="ignore"):
            arcw = (lw * self.weight.astype(dt)).astype(dt) + ts        # as compile_host folds them
            finw = np.where(self.final == -np.inf, dt(-np.inf), lw * self.final.astype(dt)).astype(dt)
        i32 = np.int32
        return {"tgt": tgt.astype(i32), "orow": orow.astype(i32), "oedge": oedge.astype(i32), "lrow": lrow.astype(i32),
                "lq": lq.astype(i32), "pkey": pk[pedge].astype(np.int64), "pedge": pedge.astype(i32),
                "next": np.where(present, self.next, -1).astype(i32), "arcw": np.where(present, arcw, dt(-np.inf)).astype(dt),
                "finw": finw}


    def compile_beam(self, device, dtype, lm_weight=1.0, token_score=0.0):
        """What `compile` returns plus the source-side arrays the beam decoder reads (include/asg_hip.h::asg_token_graph_beam),
        cached apart from `compile`'s entry (which stays as it is)."""
        base = self.compile(device, dtype, lm_weight, token_score)
        device = base["label"].device
        key = ("beam", device, dtype, float(lm_weight), float(token_score))
        hit = self._compiled.get(key)
        if hit is not None:
            return hit
        host = self.compile_beam_host(np.float32 if dtype == torch.float32 else np.float64, lm_weight, token_score)
        dev = dict(base)
        dev.update({n: torch.from_numpy(a).to(device) for n, a in host.items() if isinstance(a, np.ndarray)})
        dev["num_start"], dev["max_out"] = host["num_start"], host["max_out"]
        self._compiled[key] = dev
        return dev

    def compile_beam_host(self, dt, lm_weight=1.0, token_score=0.0):
        """The beam-only arrays as numpy arrays: orow [Q+1] (CSR offsets of the outgoing edges of each q), oarc [E,2] (target and
        the target's label of each outgoing edge, ascending by (source, target)), ow [E] (its folded weight, dtype dt), start_q
        (the q with start_w > -inf, ascending), and the integers num_start and max_out (the largest out-degree)."""
        h = self.compile_host(dt, lm_weight, token_score)
        Q = h["Q"]
        row = h["row"].astype(np.int64)
        src = h["src"].astype(np.int64)
        tgt = np.repeat(np.arange(Q, dtype=np.int64), np.diff(row))
        order = np.lexsort((tgt, src))
        deg = np.bincount(src, minlength=Q)
        orow = np.zeros(Q + 1, np.int64)
        np.cumsum(deg, out=orow[1:])
        otgt = tgt[order]
        oarc = np.stack([otgt, h["label"].astype(np.int64)[otgt]], axis=1) if Q else np.zeros((0, 2), np.int64)
        start_q = np.nonzero(h["start_w"] > -np.inf)[0]
        i32 = np.int32
        return {"orow": orow.astype(i32), "oarc": np.ascontiguousarray(oarc.astype(i32)), "ow": h["edge_w"][order],
                "start_q": start_q.astype(i32), "num_start": int(start_q.size), "max_out": int(deg.max(initial=0))}

    def compile_beam_loss(self, device, dtype, lm_weight=1.0, token_score=0.0):
        """What `compile_beam` returns plus the automaton's transition table for the target walk of the beam-pruned loss
        (include/asg_hip.h::asg_token_graph_beam_loss): next [S,N] int32, -1 where no arc.  Cached under its own key; the
        results of `compile`, `compile_loss` and `compile_beam` stay as they are."""
        base = self.compile_beam(device, dtype, lm_weight, token_score)
        device = base["label"].device
        key = ("beam_loss", device, dtype, float(lm_weight), float(token_score))
        hit = self._compiled.get(key)
        if hit is not None:
            return hit
        present = (self.next >= 0) & (self.weight != -np.inf)
        dev = dict(base)
        dev["next"] = torch.from_numpy(np.where(present, self.next, -1).astype(np.int32)).to(device)
        dev["S"], dev["start"] = self.S, self.start
        self._compiled[key] = dev
        return dev


def abi_graph(compiled):
    """The asg_token_graph view of a compiled graph (pointers into its device tensors)."""
    g = _lib.AsgTokenGraph()
    g.Q, g.E, g.N = compiled["Q"], compiled["E"], compiled["N"]
    g.dtype = _lib.ASG_DTYPE_F32 if compiled["dtype"] == torch.float32 else _lib.ASG_DTYPE_F64
    for name in ("label", "state", "row", "src", "src_label", "start_w", "final_w", "edge_w"):
        t = compiled[name]
        setattr(g, name, ctypes.c_void_p(t.data_ptr() if t.numel() else None))
    return g


def abi_graph_loss(compiled):
    """The asg_token_graph_loss view of a `compile_loss` result (it points at an asg_token_graph, which it keeps alive)."""
    g = abi_graph(compiled)
    gl = _lib.AsgTokenGraphLoss()
    gl.graph = ctypes.pointer(g)
    gl.S, gl.start = compiled["S"], compiled["start"]
    for name in ("tgt", "orow", "oedge", "lrow", "lq", "pkey", "pedge", "next", "arcw", "finw"):
        t = compiled[name]
        setattr(gl, name, ctypes.c_void_p(t.data_ptr() if t.numel() else None))
    return gl


def abi_graph_beam(compiled):
    """The asg_token_graph_beam view of a `compile_beam` result (it points at an asg_token_graph, which it keeps alive)."""
    g = abi_graph(compiled)
    gb = _lib.AsgTokenGraphBeam()
    gb.graph = ctypes.pointer(g)
    gb.num_start, gb.max_out = compiled["num_start"], compiled["max_out"]
    for name in ("orow", "oarc", "ow", "start_q"):
        t = compiled[name]
        setattr(gb, name, ctypes.c_void_p(t.data_ptr() if t.numel() else None))
    return gb


def abi_graph_beam_loss(compiled):
    """The asg_token_graph_beam_loss view of a `compile_beam_loss` result (it keeps the views it points at alive)."""
    gb = abi_graph_beam(compiled)
    gl = _lib.AsgTokenGraphBeamLoss()
    gl.beam = ctypes.pointer(gb)
    gl.S, gl.start = compiled["S"], compiled["start"]
    gl.next = ctypes.c_void_p(compiled["next"].data_ptr())
    return gl
