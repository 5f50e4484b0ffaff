"""Test-only helpers shared by tests/test_hip_graph_regimes.py (GPU) and tests/test_graph_regimes_cpu.py: the automata, the
inputs and the cached references of the cases that put the exact graph decoder (csrc/asg_decode_graph.hip) and the
exact graph loss (csrc/asg_graph_loss.hip, 5h) at the sizes where their kernels change shape, plus the routing rules of
include/asg_hip.h restated so that a case can assert the regime it names.  Nothing here needs a GPU.

Lengths.  A batch of four or more utterances holds the lengths T, 0 and 1 in its first three places and again from utterance 64
on (the second 64-lane block of the streaming kernels) as far as that block has places; a batch of three holds T, 0 and T - 1,
a batch of two T and T - 1 (the big graphs, where the reference is the cost and the full-length work is what the case is for).
"""
import functools

import numpy as np
import torch

from graph_decode_ref import decode_graph_ref, fold, product
from graph_loss_ref import Composed, full_graph_ref

F32, F64 = torch.float32, torch.float64

# ---- the routing of include/asg_hip.h (csrc/asg_decode_graph.hip, csrc/asg_graph_loss.hip), restated -------------------------
LOSS_STREAM, LOSS_RESIDENT = 128, 256        # ASG_FLAG_GRAPH_LOSS_STREAMING, ASG_FLAG_GRAPH_LOSS_RESIDENT
DEC_STREAM, DEC_RESIDENT = 16, 32            # ASG_FLAG_DECODE_GRAPH_STREAMING, ASG_FLAG_DECODE_GRAPH_RESIDENT
VEC_BYTES = 128 * 1024                       # both vectors (and the decoder's emissions) of a resident workgroup, at most
LDS_PLAIN = 64 * 1024                        # above this a launch has to ask for its dynamic LDS
LOSS_EDGES = 4096                            # kLossResidentEdges
DEC_EDGES = 32768                            # kResidentEdges
WG = 1024                                    # kLT, kRT: threads of a resident workgroup


def esize(dtype):
    return 8 if dtype == F64 else 4


def loss_fits(e, Q):
    return 2 * Q * e <= VEC_BYTES


def loss_resident(flags, e, Q, E):
    """Does asg_graph_full_forward / _backward take the resident route?"""
    if Q == 0:
        return True
    if flags & LOSS_STREAM:
        return False
    if flags & LOSS_RESIDENT:
        return loss_fits(e, Q)
    return loss_fits(e, Q) and E <= LOSS_EDGES


def loss_lds(e, Q):
    return 256 + 2 * Q * e


def dec_fits(e, N, Q):
    return N <= WG and 2 * (Q + N) * e <= VEC_BYTES


def dec_resident(flags, e, N, Q, E):
    """Does asg_viterbi_decode_graph take the resident route?"""
    if Q == 0 or flags & DEC_STREAM:
        return False
    if flags & DEC_RESIDENT:
        return dec_fits(e, N, Q)
    return dec_fits(e, N, Q) and E <= DEC_EDGES


def dec_lds(e, N, Q):
    """Dynamic LDS of the resident decoder: the transition matrix comes along when everything stays under 160 KiB."""
    base = 512 + (2 * Q + 2 * N) * e
    return base + N * N * e if base + N * N * e <= 160 * 1024 else base


def dec_stage_frames(e, N, Q):
    """Frames of back-pointer rows the resident backtrace stages at a time."""
    return min(64, (dec_lds(e, N, Q) - 512) // (Q * 4))


def dec_subgroup(Q, E):
    """Lanes per target of the resident decoder."""
    avg = (E + Q - 1) // Q
    fill = 1
    while fill * 2 <= max(WG // Q, 1):
        fill *= 2
    want = min(fill, max(avg // 2, 1))
    return 64 if want >= 64 else (16 if want >= 16 else 4)


# ---- automata ------------------------------------------------------------------------------------------------------------------

def _asg():
    import torch_asg_amd
    return torch_asg_amd


# (_ngram and _one_state are shared with tests/test_hip_graph_loss.py, which imports them from here)
def _ngram(N, order, seed, holes=False):
    rng = np.random.default_rng(seed)
    lp = np.log(rng.dirichlet(np.ones(N + 1), size=(N + 1,) * (order - 1))) if order > 1 else np.log(rng.dirichlet(np.ones(N + 1)))
    if holes:
        lp[rng.random(size=lp.shape) < 0.2] = -np.inf
    return _asg().TokenGraph.from_ngram(lp)


def _enterable(S, N, seed):
    """A random automaton every state of which can be entered: 30 % of the arcs missing, 30 % of the states not accepting."""
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, S, size=(S, N))
    nxt[rng.random(size=(S, N)) < 0.3] = -1
    w = rng.normal(size=(S, N))
    f = rng.normal(size=S)
    f[rng.random(size=S) < 0.3] = -np.inf
    return _asg().TokenGraph(nxt, w, f, start=0)


def _shift(S, drop, seed=5):
    """next[s][i] = (s + stride[i]) % S over 4 tokens: every column is a permutation of the states, so each arc reaches a product
    state of its own and Q = 4 * S - drop once `drop` arcs are removed (the last tokens of the highest states).  Every state
    accepts.  The strides 1, S // 3, S // 2 + 1 and S - 5 spread the states a few frames reach over the whole range, so the live
    values of a short utterance lie at the bottom, in the middle and at the top of the kernels' state vectors."""
    N = 4
    rng = np.random.default_rng(seed)
    nxt = (np.arange(S)[:, None] + np.array([1, S // 3, S // 2 + 1, S - 5])[None, :]) % S
    for k in range(drop):
        nxt[S - 1 - k, N - 1] = -1
    return _asg().TokenGraph(nxt, rng.normal(size=(S, N)), rng.normal(size=S), start=0)


def _one_state(N):
    return _asg().TokenGraph(np.zeros((1, N), np.int64), np.zeros((1, N)), np.zeros(1))


def _cycle3(N=12, tokens=(0, 1, 2), seed=6):
    """Three states in a cycle that moves on three tokens only: the other labels have no product state."""
    rng = np.random.default_rng(seed)
    nxt = np.full((3, N), -1, np.int64)
    nxt[:, list(tokens)] = ((np.arange(3) + 1) % 3)[:, None]
    return _asg().TokenGraph(nxt, rng.normal(size=(3, N)), rng.normal(size=3), start=0)


def _dead(which):
    """The three automata without any accepted path of tests/test_hip_graph_decode.py::test_edge_cases."""
    g = _ngram(6, 2, 7)
    if which == 0:
        return _asg().TokenGraph(g.next, g.weight, np.full(g.S, -np.inf))                      # no accepting state
    if which == 1:
        return _asg().TokenGraph(np.where(np.arange(g.S)[:, None] == 0, -1, g.next), g.weight, g.final)   # no arc at the start
    return _asg().TokenGraph(np.full((2, 6), -1), np.zeros((2, 6)), np.zeros(2))              # no arc at all (Q = 0)


CYCLE_TOKENS = {"cycle3": (0, 1, 2), "cycle3_n14": (0, 1, 13)}     # the tokens the 3-state cycles move on

# name -> (builder, N, Q, E): Q and E are asserted by both test modules, never trusted
GRAPHS = {
    "bigram65": (lambda: _ngram(65, 2, 21), 65, 65, 4160),
    "bigram64": (lambda: _ngram(64, 2, 22), 64, 64, 4032),
    "bigram10": (lambda: _ngram(10, 2, 2), 10, 10, 90),
    "trigram40_holes": (lambda: _ngram(40, 3, 3, holes=True), 40, 1633, 51081),
    "enterable600": (lambda: _enterable(600, 20, 31), 20, 6059, 80948),
    "enterable1000": (lambda: _enterable(1000, 20, 32), 20, 10093, 134584),
    # the fit limits 2 * Q * e <= 128 KiB of the loss: float32 16384 | 16385, float64 8192 | 8193
    "shift16384": (lambda: _shift(4096, 0), 4, 16384, 49152),
    "shift16385": (lambda: _shift(4097, 3), 4, 16385, 49146),
    "shift8192": (lambda: _shift(2048, 0), 4, 8192, 24576),
    "shift8193": (lambda: _shift(2049, 3), 4, 8193, 24570),
    # the fit limits 2 * (Q + N) * e <= 128 KiB of the decoder, N = 4: float32 16380 | 16381, float64 8188 | 8189
    "shift16380": (lambda: _shift(4095, 0), 4, 16380, 49140),
    "shift16381": (lambda: _shift(4096, 3), 4, 16381, 49134),
    "shift8188": (lambda: _shift(2047, 0), 4, 8188, 24564),
    "shift8189": (lambda: _shift(2048, 3), 4, 8189, 24558),
    "one_state1024": (lambda: _one_state(1024), 1024, 1024, 1024 * 1023),
    "one_state1025": (lambda: _one_state(1025), 1025, 1025, 1025 * 1024),
    "cycle3": (_cycle3, 12, 9, 18),
    # (N = 12 fits the ceil(Q / 4) * 4 = 12 wavefronts of a backward grid sized by Q alone; with N = 14 and the cycle on the
    # tokens 0, 1 and 13, label 13 lies beyond them and has a gradient that is not zero)
    "cycle3_n14": (lambda: _cycle3(14, CYCLE_TOKENS["cycle3_n14"]), 14, 9, 18),
    "dead_final": (lambda: _dead(0), 6, 6, 30),
    "dead_start": (lambda: _dead(1), 6, 6, 30),
    "dead_empty": (lambda: _dead(2), 6, 0, 0),
}


@functools.lru_cache(maxsize=None)
def graph(name):
    return GRAPHS[name][0]()


@functools.lru_cache(maxsize=None)
def facts(name):
    """(Q, E) of the product graph, from the restatement (tests/graph_decode_ref.py::product), not from torch_asg_amd/graph.py."""
    g = graph(name)
    present = fold(g.next, g.weight, g.final, np.float64, 1.0, 0.0)[0]
    _, _, src, _, Q = product(g.next, present)
    return int(Q), int(src.size)


def expected(name):
    """(Q, E) the table states."""
    return GRAPHS[name][2], GRAPHS[name][3]


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def lengths(T, B, seed):
    g = torch.Generator().manual_seed(seed)
    il = torch.randint(0, T + 1, (B,), generator=g)
    if B == 2:
        il[:] = torch.tensor([T, T - 1])
    elif B == 3:
        il[:] = torch.tensor([T, 0, T - 1])
    else:
        il[:3] = torch.tensor([T, 0, 1])
        for k, v in enumerate((1, T, 0)):                  # the second 64-lane block
            if 64 + k < B:
                il[64 + k] = v
        if B >= 130:                                        # ... and the partial third one
            il[128], il[129] = 0, T
    return il


@functools.lru_cache(maxsize=None)
def inputs(T, B, N, seed, f64):
    """-> (x [T,B,N], tr [N,N], il [B], grad_scores [B] float64): values drawn in float64, rounded to the dtype once."""
    dtype = F64 if f64 else F32
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g, dtype=F64), -1).to(dtype)
    tr = (0.5 * torch.randn(N, N, generator=g, dtype=F64)).to(dtype)
    gs = torch.linspace(-1.0, 2.0, B, dtype=F64) if B > 1 else torch.tensor([1.5], dtype=F64)
    return x, tr, lengths(T, B, seed + 1000), gs


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def loss_reference(name, T, B, seed, f64, with_lengths=True):
    """(Z, grad_inputs, grad_transition) of tests/graph_loss_ref.py for inputs(T, B, N, seed, f64); computed once, read-only."""
    g = graph(name)
    x, tr, il, gs = inputs(T, B, g.N, seed, f64)
    return _frozen(list(full_graph_ref(x.double().numpy(), tr.double().numpy(), g.next, g.weight, g.final, g.start,
                                       il.numpy() if with_lengths else None, 1.0, 0.0, gs.numpy(),
                                       fold_dt=np.float64 if f64 else np.float32)))


@functools.lru_cache(maxsize=None)
def decode_reference(name, T, B, seed, f64, with_lengths=True):
    """The five outputs of tests/graph_decode_ref.py for the same inputs; computed once, read-only."""
    g = graph(name)
    x, tr, il, _ = inputs(T, B, g.N, seed, f64)
    return _frozen(list(decode_graph_ref(x.numpy(), tr.numpy(), g.next, g.weight, g.final, g.start,
                                         il.numpy() if with_lengths else None, 1.0, 0.0)))


def finite_mask(name, frames):
    """Which product states have a finite alpha after `frames` frames of finite emissions: those a path from the start reaches
    (the weights of present arcs are finite, so -inf is structural)."""
    g = graph(name)
    c = Composed(g.next, g.weight, g.final, g.start)
    reach = c.start_w > -np.inf
    for _ in range(1, frames):
        nxt = reach.copy()
        nxt[c.tgt[reach[c.src]]] = True
        reach = nxt
    return reach


def finite_states(name, frames):
    """How many they are."""
    return int(finite_mask(name, frames).sum())


def mixed_parity(il):
    """Lengths >= 1 of both parities (the ping-pong rows of the streaming routes)."""
    l = np.asarray(il)
    l = l[l >= 1]
    return bool((l % 2 == 0).any() and (l % 2 == 1).any())
