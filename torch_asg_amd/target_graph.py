"""Per-utterance target graphs: the transcript of an utterance as "one of these" (`torch_asg_amd.target_graph_score`,
`target_graph_asg_loss`, `ASGLoss.target_graph_loss`, `target_graph_viterbi`, `target_graph_confidence`).

A `TargetGraphs` is a batch of B small node-labelled graphs.  Node k of graph b carries a label in [0, N), a start weight and a
final weight (-inf: not a start / not a final); a directed edge src -> dst carries a weight (finite or -inf).  The stay on a
node is implicit and weighs nothing.  The score of utterance b is the log-sum over every path of graph b from a start to a
final, and over every alignment of that path's labels to the frames, of start + emissions + transitions + edge weights +
final -- for a chain, the force-aligned score.  Cycles are allowed (the recursion is time-synchronous).  The lattice collapses
repeated labels, so an edge between two nodes of the same label is refused: spell those with a repetition label, as
`TokenGraph.from_lexicon` asks.

`compile` packs the batch once into the padded device arrays the kernels read (include/asg_hip.h::asg_target_graphs).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .graph import _host

MAX_NODES = 1024


def _weights(a, what):
    w = np.array(_host(a, np.float64), dtype=np.float64).reshape(-1)
    if np.isnan(w).any() or (w == np.inf).any():
        raise ValueError("TargetGraphs: %s must not hold NaN or +inf" % what)
    return w


class TargetGraphs:
    """A batch of node-labelled target graphs, one per utterance; validated on the CPU when constructed.

    labels[b], start[b], final[b]: K_b labels and weights (K_b <= 1024, 0 allowed); edges[b]: a list of (src, dst, weight)."""

    def __init__(self, labels, start, final, edges, num_labels):
        N = int(num_labels)
        if N < 1:
            raise ValueError("TargetGraphs: num_labels must be >= 1")
        B = len(labels)
        if B < 1 or len(start) != B or len(final) != B or len(edges) != B:
            raise ValueError("TargetGraphs: labels, start, final and edges must list the same B >= 1 utterances")
        self.N, self.B = N, B
        self.graphs = []                # per utterance: label [K], start_w [K], final_w [K], src, dst [E] (incoming CSR order), edge_w [E]
        for b in range(B):
            lab = np.array(_host(labels[b], np.int64), dtype=np.int64).reshape(-1)
            K = lab.size
            if K > MAX_NODES:
                raise ValueError("TargetGraphs: graph %d has %d nodes, at most %d" % (b, K, MAX_NODES))
            if ((lab < 0) | (lab >= N)).any():
                raise ValueError("TargetGraphs: graph %d has a label outside [0, %d)" % (b, N))
            sw, fw = _weights(start[b], "start"), _weights(final[b], "final")
            if sw.size != K or fw.size != K:
                raise ValueError("TargetGraphs: graph %d has %d nodes but %d start and %d final weights" % (b, K, sw.size, fw.size))
            ed = list(edges[b])
            src = np.array([int(e[0]) for e in ed], dtype=np.int64)
            dst = np.array([int(e[1]) for e in ed], dtype=np.int64)
            ew = _weights([float(e[2]) for e in ed], "edge weights")
            if ((src < 0) | (src >= K) | (dst < 0) | (dst >= K)).any():
                raise ValueError("TargetGraphs: graph %d has an edge outside its %d nodes" % (b, K))
            if (src == dst).any():
                raise ValueError("TargetGraphs: graph %d has a self edge; the stay on a node is implicit" % b)
            if (lab[src] == lab[dst]).any():
                raise ValueError("TargetGraphs: graph %d has an edge between two nodes of the same label; the lattice collapses "
                                 "repeats (spell them with a repetition label)" % b)
            order = np.lexsort((src, dst))                          # incoming CSR: by target, ascending by source
            self.graphs.append((lab, sw, fw, src[order], dst[order], ew[order]))
        self.Kmax = max(g[0].size for g in self.graphs)
        self.Emax = max(g[3].size for g in self.graphs)
        if B * (self.Kmax + self.Emax) > (1 << 31) - 1:
            raise ValueError("TargetGraphs: B * (Kmax + Emax) must stay below 2^31")
        self._compiled = {}
        self.final_alternative = None   # from_alternatives: host [B,Kmax] int64, the index of the sequence that ends in a node, -1 elsewhere
        self.alternative_final = None   # from_alternatives: host [B,Amax] int64, its inverse: the node in which sequence a ends, -1 behind them
        self._maps = {}    # (name, device) -> tensor

    @classmethod
    def from_targets(cls, targets, target_lengths, num_labels):
        """A chain per utterance: targets [B,S] and target_lengths [B] (None: S) as `ASGLoss.forward` takes them.  Start weight
        0 on node 0, final weight 0 on the last node; length 0 gives an empty graph (score -inf).  Two equal consecutive
        labels raise ValueError, as any edge between nodes of one label does."""
        tg = _host(targets, np.int64)
        if tg.ndim != 2:
            raise ValueError("TargetGraphs.from_targets: targets must be [B,S]")
        B, S = tg.shape
        tl = np.full(B, S, np.int64) if target_lengths is None else _host(target_lengths, np.int64).reshape(-1)
        if tl.size != B:
            raise ValueError("TargetGraphs.from_targets: target_lengths must be [%d]" % B)
        tl = np.clip(tl, 0, S)
        return cls.from_alternatives([[tg[b, :tl[b]]] if tl[b] else [] for b in range(B)], num_labels)

    @classmethod
    def from_alternatives(cls, alternatives, num_labels, weights=None):
        """Per utterance a list of label sequences, any of which is the transcript: the prefix tree of the sequences, its
        nodes numbered in order of first creation while the sequences are inserted in the given order.  The first nodes are
        starts with weight 0, every sequence end is final with that sequence's weight (weights[b][n], default 0), edges
        weigh 0.  `final_alternative[b, k]` records which sequence ends in node k.  An empty sequence, two equal consecutive labels and the same sequence given twice (the log semiring would
        count it once) raise ValueError."""
        labels, start, final, edges, ends = [], [], [], [], []
        for b, seqs in enumerate(alternatives):
            ends.append([])
            ws = [0.0] * len(seqs) if weights is None else list(weights[b])
            if len(ws) != len(seqs):
                raise ValueError("TargetGraphs.from_alternatives: %d weights for %d sequences of utterance %d" % (len(ws), len(seqs), b))
            lab, sw, fw, ed = [], [], [], []
            children = [{}]                                         # children[0]: the virtual root; node k is children[k + 1]
            for seq, w in zip(seqs, ws):
                seq = [int(x) for x in _host(seq, np.int64).reshape(-1)]
                if not seq:
                    raise ValueError("TargetGraphs.from_alternatives: empty sequence in utterance %d" % b)
                if any(x == y for x, y in zip(seq, seq[1:])):
                    raise ValueError("TargetGraphs.from_alternatives: sequence %s repeats a label; the lattice collapses repeats" % (seq,))
                at = -1
                for x in seq:
                    nxt = children[at + 1].get(x)
                    if nxt is None:
                        nxt = len(lab)
                        children[at + 1][x] = nxt
                        children.append({})
                        lab.append(x)
                        sw.append(0.0 if at < 0 else -np.inf)
                        fw.append(-np.inf)
                        if at >= 0:
                            ed.append((at, nxt, 0.0))
                    at = nxt
                if fw[at] != -np.inf:
                    raise ValueError("TargetGraphs.from_alternatives: sequence %s is given twice in utterance %d" % (seq, b))
                fw[at] = float(w)
                if fw[at] == -np.inf:
                    raise ValueError("TargetGraphs.from_alternatives: a sequence weight must be finite")
                ends[-1].append(at)
            labels.append(lab); start.append(sw); final.append(fw); edges.append(ed)
        self = cls(labels, start, final, edges, num_labels)
        self.final_alternative = np.full((self.B, self.Kmax), -1, np.int64)
        self.alternative_final = np.full((self.B, max(len(at) for at in ends)), -1, np.int64)
        for b, at in enumerate(ends):
            self.final_alternative[b, at] = np.arange(len(at))
            self.alternative_final[b, :len(at)] = at
        return self

    def final_alternative_on(self, device):
        """`final_alternative` as a tensor on `device` (cached), or None for graphs built from arrays."""
        return self._map_on("final_alternative", device)

    def alternative_final_on(self, device):
        """`alternative_final` as a tensor on `device` (cached), or None for graphs built from arrays."""
        return self._map_on("alternative_final", device)

    def _map_on(self, name, device):
        host = getattr(self, name)
        if host is None:
            return None
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        hit = self._maps.get((name, device))
        if hit is None:
            hit = self._maps[(name, device)] = torch.from_numpy(host).to(device)
        return hit

    def compile_host(self, dt):
        """The padded arrays as numpy arrays, weights in dtype `dt`; integer arrays int32 (pkey int64):
        nk [B]; label, start_w, final_w [B,Kmax]; row [B,Kmax+1]; src, tgt, edge_w [B,Emax] (incoming CSR); orow [B,Kmax+1] and
        oedge [B,Emax] (the outgoing edges of each node as incoming-edge indices, ascending by (src, tgt)); nlab [B], lab
        [B,Kmax], lrow [B,Kmax+1], lnode [B,Kmax] (the distinct labels ascending and their nodes ascending); and the batch-wide
        list for the transition gradient: every stay (slot k) and edge (slot Kmax + e) keyed by l_dst * N + l_src, sorted
        stably by key, then b, then slot -- pslot = b * (Kmax + Emax) + slot, pkey the distinct keys, pseg their offsets."""
        dt = np.dtype(dt).type
        B, N, Kmax, Emax = self.B, self.N, self.Kmax, self.Emax
        i32 = np.int32
        h = {n: np.zeros((B, Kmax), i32) for n in ("label", "lab", "lnode")}
        h.update({n: np.zeros((B, Kmax + 1), i32) for n in ("row", "orow", "lrow")})
        h.update({n: np.zeros((B, Emax), i32) for n in ("src", "tgt", "oedge")})
        h.update({n: np.full((B, Kmax), -np.inf, dt) for n in ("start_w", "final_w")})
        h["edge_w"] = np.full((B, Emax), -np.inf, dt)
        h["nk"], h["nlab"] = np.zeros(B, i32), np.zeros(B, i32)
        keys, slots = [], []
        for b, (lab, sw, fw, src, dst, ew) in enumerate(self.graphs):
            K, E = lab.size, src.size
            h["nk"][b] = K
            h["label"][b, :K], h["start_w"][b, :K], h["final_w"][b, :K] = lab, sw.astype(dt), fw.astype(dt)
            h["row"][b, 1:K + 1] = np.cumsum(np.bincount(dst, minlength=K))
            h["row"][b, K + 1:] = E
            h["src"][b, :E], h["tgt"][b, :E], h["edge_w"][b, :E] = src, dst, ew.astype(dt)
            h["oedge"][b, :E] = np.lexsort((dst, src))
            h["orow"][b, 1:K + 1] = np.cumsum(np.bincount(src, minlength=K))
            h["orow"][b, K + 1:] = E
            distinct, counts = np.unique(lab, return_counts=True)
            h["nlab"][b] = distinct.size
            h["lab"][b, :distinct.size] = distinct
            h["lrow"][b, 1:distinct.size + 1] = np.cumsum(counts)
            h["lrow"][b, distinct.size + 1:] = K
            h["lnode"][b, :K] = np.argsort(lab, kind="stable")
            keys += [lab * N + lab, lab[dst] * N + lab[src]]
            slots += [b * (Kmax + Emax) + np.arange(K), b * (Kmax + Emax) + Kmax + np.arange(E)]
        keys, slots = np.concatenate(keys).astype(np.int64), np.concatenate(slots).astype(np.int64)
        order = np.argsort(keys, kind="stable")
        pkey, first = np.unique(keys[order], return_index=True)
        h["pkey"], h["pslot"] = pkey.astype(np.int64), slots[order].astype(i32)
        h["pseg"] = np.append(first, keys.size).astype(i32)
        return h

    def compile(self, device, dtype):
        """The padded arrays on `device` with weights in `dtype` (float32 / float64), cached per (device, dtype): a dict of
        device tensors plus B, Kmax, Emax, N, npairs and dtype."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if dtype not in (torch.float32, torch.float64):
            raise RuntimeError("torch_asg_amd: expected scalar type Float or Double but found %s" % dtype)
        hit = self._compiled.get((device, dtype))
        if hit is not None:
            return hit
        host = self.compile_host(np.float32 if dtype == torch.float32 else np.float64)
        dev = {n: torch.from_numpy(a).to(device) for n, a in host.items()}
        dev.update(B=self.B, Kmax=self.Kmax, Emax=self.Emax, N=self.N, npairs=int(host["pkey"].size), dtype=dtype)
        self._compiled[(device, dtype)] = dev
        return dev


def abi_target_graphs(compiled):
    """The asg_target_graphs view of a compiled batch (pointers into its device tensors)."""
    g = _lib.AsgTargetGraphs()
    g.B, g.Kmax, g.Emax, g.npairs, g.N = (compiled[n] for n in ("B", "Kmax", "Emax", "npairs", "N"))
    g.dtype = _lib.ASG_DTYPE_F32 if compiled["dtype"] == torch.float32 else _lib.ASG_DTYPE_F64
    for name in _lib.TARGET_GRAPH_ARRAYS:
        t = compiled[name]
        setattr(g, name, ctypes.c_void_p(t.data_ptr() if t.numel() else None))
    return g
