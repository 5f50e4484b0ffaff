"""GPU tests (-m gpu) of the utterance groups under `max_work_bytes` when the last group is ragged: five utterances in groups of
2, 2 and 1 through each of the six grouped entry points (`HipBackend._groups`), against the same call in one group.  The
neighbouring grouping tests use B = 6 in groups of 2, which never leaves a short last group."""
import pytest
import torch

from beam_loss_cases import _ngram
from beam_word_cases import SMALL_WORDS, arpa_lm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, B, N, S = 12, 5, 6, 3
LENGTHS = (12, 3, 0, 7, 12)
TARGET_LENGTHS = (3, 1, 0, 2, 3)


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _inputs(dtype):
    g = torch.Generator().manual_seed(17)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g, dtype=torch.float64), -1).to(dtype)
    tr = (0.5 * torch.randn(N, N, generator=g, dtype=torch.float64)).to(dtype)
    tg = torch.randint(0, N, (B, S), generator=g)
    return x.to(DEV), tr.to(DEV), tg.to(DEV), torch.tensor(TARGET_LENGTHS, device=DEV)


def _loss(fn, x, tr, tg, tl, graph, il, *args, **kw):
    """(loss [B], inputs.grad, transition.grad) of a graph loss for an upstream gradient of ones."""
    xd, td = x.clone().requires_grad_(True), tr.clone().requires_grad_(True)
    loss = fn(xd, tg, td, graph, il, tl, *args, **kw)
    loss.backward(torch.ones_like(loss))
    return loss.detach(), xd.grad, td.grad


def _entry(name, dtype, il, nb=B):
    """name -> call(**kw) of that entry point on the first `nb` utterances of the shared case, kw = {} or
    {"max_work_bytes": n}."""
    A = _asg()
    x, tr, tg, tl = _inputs(dtype)
    x, tg, tl, il = x[:, :nb], tg[:nb], tl[:nb], None if il is None else il[:nb]
    graph = _ngram(N, 2, 3)
    if name == "viterbi_decode_graph":
        return lambda **kw: A.viterbi_decode_graph(x, tr, graph, il, 0.6, 0.1, **kw)
    if name == "beam_decode_graph":
        return lambda **kw: A.beam_decode_graph(x, tr, graph, il, 4, 8.0, 0.6, 0.1, **kw)
    if name == "beam_decode_graph_nbest":
        return lambda **kw: A.beam_decode_graph_nbest(x, tr, graph, il, 4, 3, 8.0, 0.6, 0.1, True, **kw)
    if name == "beam_decode_words":
        lex, lm = A.Lexicon(SMALL_WORDS, N, N - 1), arpa_lm(len(SMALL_WORDS), 1, 5)
        return lambda **kw: A.beam_decode_words(x, tr, lex, lm, il, 4, 8.0, 0.5, -0.2, 0.1, **kw)
    if name == "graph_asg_loss":
        return lambda **kw: _loss(A.graph_asg_loss, x, tr, tg, tl, graph, il, 0.6, 0.1, **kw)
    assert name == "beam_graph_asg_loss"
    return lambda **kw: _loss(A.beam_graph_asg_loss, x, tr, tg, tl, graph, il, 4, 8.0, 0.6, 0.1, **kw)


ENTRIES = ("viterbi_decode_graph", "beam_decode_graph", "beam_decode_graph_nbest", "beam_decode_words", "graph_asg_loss",
           "beam_graph_asg_loss")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("lengths", ["lengths", "none"])
@pytest.mark.parametrize("name", ENTRIES)
def test_a_ragged_last_group_changes_nothing(name, lengths, dtype):
    """`per`, the workspace of one utterance, is the first workspace of the call in one group divided by B (what the
    neighbouring grouping tests do) -- or, where it is larger, the workspace of the call on one utterance alone: the exact
    decoder and n-best round parts of their workspace up to 256 bytes, which at T = 12 makes one utterance cost more than a
    fifth of five, and the group size starts from max_work_bytes // (the size for one utterance).  max_work_bytes = 2.5 per
    then gives the groups (0, 2), (2, 4), (4, 5).  Decoders and n-best: every output bit for bit.  Beam loss: loss,
    inputs.grad and transition.grad bit for bit (its groups add into one transition.grad in batch order).  Exact graph loss:
    the loss bit for bit, the gradients as tests/test_hip_graph_loss.py::test_small_work_budget_groups_utterances compares
    them (transition.grad is a sum over the groups)."""
    from torch_asg_amd.asg import native
    il = torch.tensor(LENGTHS, device=DEV) if lengths == "lengths" else None
    call, call_one = _entry(name, dtype, il), _entry(name, dtype, il, 1)
    be = native()
    seen, spans = [], []
    buf, point = be._buf, be._group_problem
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    be._group_problem = lambda p, b0, b1, *a: (spans.append((b0, b1)), point(p, b0, b1, *a))[1]
    try:
        one = call()
        per = seen[0] // B
        del seen[:], spans[:]
        call_one()
        per = max(per, seen[0])
        del spans[:]
        small = call(max_work_bytes=2 * per + per // 2)
    finally:
        del be._buf, be._group_problem
    print(name, lengths, dtype, "per", per, "spans", spans)
    assert per > 0 and spans[:3] == [(0, 2), (2, 4), (4, 5)]
    exact = name != "graph_asg_loss"
    for k, (u, v) in enumerate(zip(small, one)):
        if u is None or v is None:
            assert u is None and v is None
            continue
        if not torch.equal(u, v):
            print(name, lengths, dtype, "output", k, "max |difference|", float((u - v).abs().nan_to_num(0.0).max()))
        if exact or k == 0:
            assert torch.equal(u, v), k
        else:
            assert torch.allclose(u, v, rtol=1e-12, atol=1e-12, equal_nan=True), k
