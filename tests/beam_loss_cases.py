"""Test-only helpers shared by the GPU tests of the beam-pruned ASG loss (tests/test_hip_beam_loss.py and
tests/test_hip_beam_loss_regimes.py): the automata, the random cases, the call through `BeamGraphFullScore`, the call of the numpy
restatement tests/beam_loss_ref.py and the comparison under the project's parity rule (util.assert_close, scaled 1e-4 in float32;
1e-9 in float64 -- BASELINE.md section 2)."""
import numpy as np
import torch

from beam_loss_ref import beam_loss_ref
from util import assert_close

DEV = "cuda:0"
INF = float("inf")


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _ngram(N, order, seed, holes=False):
    rng = np.random.default_rng(seed)
    lp = np.log(rng.dirichlet(np.ones(N + 1), size=(N + 1,) * (order - 1))) if order > 1 else np.log(rng.dirichlet(np.ones(N + 1)))
    if holes:
        lp[rng.random(size=lp.shape) < 0.2] = -np.inf
    return _asg().TokenGraph.from_ngram(lp)


def _random_graph(S, N, seed):
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, S // 2, size=(S, N))
    nxt[rng.random(size=(S, N)) < 0.3] = -1
    w = rng.normal(size=(S, N))
    f = rng.normal(size=S)
    f[rng.random(size=S) < 0.3] = -np.inf
    return _asg().TokenGraph(nxt, w, f, start=0)


def _lexicon(N, words, seed, maxlen=4):
    """A trie over tokens 1 .. N-1 with separator 0; with many words the root's in-degree (one per word end) exceeds a beam."""
    rng = np.random.default_rng(seed)
    sp = []
    for _ in range(words):
        L = int(rng.integers(1, maxlen + 1))
        w = [int(rng.integers(1, N))]
        while len(w) < L:
            v = int(rng.integers(1, N))
            if v != w[-1]:
                w.append(v)
        sp.append(w)
    return _asg().TokenGraph.from_lexicon(sp, N, 0, list(rng.normal(size=words)))


def _one_state(N):
    return _asg().TokenGraph(np.zeros((1, N), np.int64), np.zeros((1, N)), np.zeros(1))


GRAPHS = {
    "unigram": lambda: _ngram(10, 1, 1),
    "bigram": lambda: _ngram(10, 2, 2),
    "trigram_holes": lambda: _ngram(6, 3, 3, holes=True),
    "random": lambda: _random_graph(12, 7, 4),
    "lexicon": lambda: _lexicon(8, 60, 5),
}


def _case(T, B, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g, dtype=torch.float64), -1).to(dtype)
    tr = (0.5 * torch.randn(N, N, generator=g, dtype=torch.float64)).to(dtype)
    il = torch.randint(0, T + 1, (B,), generator=g)
    il[0] = T
    if B > 1:
        il[1] = 0
    if B > 2:
        il[2] = 1
    return x, tr, il


def _targets(B, S, N, il, seed):
    g = torch.Generator().manual_seed(seed)
    tg = torch.randint(0, N, (B, S), generator=g)
    tl = torch.randint(0, S + 1, (B,), generator=g)
    tl[0] = min(S, int(il[0]))
    if S >= 2:
        tg[0, 1] = tg[0, 0]                                # a repeat in the target
    return tg, tl


def _full(x, tr, graph, il, K, th=INF, lw=1.0, ts=0.0, gs=None, tg=None, tl=None, max_work_bytes=1 << 30):
    xd = x.to(DEV).requires_grad_(True)
    td = tr.to(DEV).requires_grad_(True)
    dv = lambda t: None if t is None else t.to(DEV)
    Z = _asg().BeamGraphFullScore.apply(xd, td, graph, dv(il), K, th, lw, ts, dv(tg), dv(tl), max_work_bytes)
    g = torch.ones_like(Z) if gs is None else gs.to(DEV, Z.dtype)
    Z.backward(g)
    torch.cuda.synchronize()
    return Z.detach().cpu(), xd.grad.cpu(), td.grad.cpu()


def _ref(x, tr, graph, il, K, th=INF, lw=1.0, ts=0.0, gs=None, tg=None, tl=None, info=None):
    np_ = lambda t: None if t is None else t.numpy()
    return beam_loss_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start, np_(il), K, th, lw, ts,
                         np_(tg), np_(tl), np_(gs), info)[:3]


def _compare(got, want, dtype, what):
    Z, gx, gtr = got
    Zr, gxr, gtrr = want
    fin = np.isfinite(Zr)
    assert (np.isfinite(Z.numpy()) == fin).all(), what
    assert (Z.numpy()[~fin] == -np.inf).all(), what
    assert not torch.isnan(gx).any() and not torch.isnan(gtr).any(), what
    if dtype == torch.float64:
        assert np.allclose(Z.numpy()[fin], Zr[fin], rtol=1e-9, atol=1e-9), what
        assert np.allclose(gx.numpy(), gxr, rtol=1e-9, atol=1e-9), what
        assert np.allclose(gtr.numpy(), gtrr, rtol=1e-9, atol=1e-9), what
    else:
        assert_close(Z.numpy()[fin], Zr[fin], what=what + " Z")
        assert_close(gx.numpy(), gxr, what=what + " grad_inputs")
        assert_close(gtr.numpy(), gtrr, what=what + " grad_transition")
