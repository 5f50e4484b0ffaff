"""GPU tests (-m gpu) of LM look-ahead in the lexicon + word-LM beam decoder (`beam_decode_words(..., lookahead=)`,
csrc/asg_beam_word_la.hip): all eight outputs bit-identical to the test-side numpy restatement (tests/beam_word_la_ref.py, pinned
on the CPU by tests/test_beam_word_la_cpu.py).  Every case first asserts, from the restatement's own sets, that its input is in
the regime it names."""
import numpy as np
import pytest
import torch

from beam_word_la_ref import beam_word_la_ref
from beam_word_ref import beam_word_ref
from test_beam_word_la_cpu import hand_case, rescue_case
from test_hip_beam_word import grid_case, ties_case, wide_lexicon_and_lm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
NAMES = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths")
ALL = 1024
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _gpu(x, tr, lex, lm, il, K, theta=INF, lw=1.0, ws=0.0, ts=0.0, **kw):
    out = _asg().beam_decode_words(x.to(DEV), tr.to(DEV), lex, lm, None if il is None else il.to(DEV), K, theta, lw, ws, ts, **kw)
    torch.cuda.synchronize()
    assert out._fields == NAMES
    assert out.scores.dtype == x.dtype and all(o.dtype == torch.int64 for o in out[1:])
    return {n: o.cpu().numpy() for n, o in zip(NAMES, out)}


def _check(x, tr, lex, lm, la, il, K, theta=INF, lw=1.0, ws=0.0, ts=0.0, info=None, what=""):
    got = _gpu(x, tr, lex, lm, il, K, theta, lw, ws, ts, lookahead=la)
    want = beam_word_la_ref(x.numpy(), tr.numpy(), lex, lm, la.order, None if il is None else il.numpy(), K, theta, lw, ws, ts,
                            info=info)
    for n in NAMES:
        assert got[n].tobytes() == want[n].tobytes(), "%s %s K=%d theta=%s order=%d" % (n, what, K, theta, la.order)
    return got


def _normal(T, B, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, B, N, generator=g, dtype=torch.float64).to(dtype), torch.randn(N, N, generator=g, dtype=torch.float64).to(dtype)


# ---------------------------------------------------------------------------------------------------------------- grid
@DTYPES
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("lm_order", [2, 3], ids=["bigram", "trigram"])
def test_grid_of_beams_thresholds_and_orders(lm_order, order, dtype):
    A = _asg()
    lex, lm, x, tr, il = grid_case(lm_order, dtype)
    la = A.WordLookahead(lex, lm, order)
    LW, WS, TS = 0.7, -0.4, 0.3
    changed = 0
    for K in (1, 2, 3, 8, 64, ALL):
        for theta in (INF, 2.0, 0.0):
            info = {}
            _check(x, tr, lex, lm, la, il, K, theta, LW, WS, TS, info, "grid")
            if K == ALL and theta == INF:
                assert max(max(s) for s in info["sizes"] if s) < ALL
            if K <= 3 and theta == INF:
                plain = {}
                beam_word_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), K, theta, LW, WS, TS, info=plain)
                changed += plain["kept"] != info["kept"]
    assert changed > 0                                     # the look-ahead changed what a narrow beam keeps


# ---------------------------------------------------------------------------------------------------------------- ties
@DTYPES
def test_ties_at_the_last_rank_and_between_sources(dtype):
    A = _asg()
    lex, lm, x, tr, il = ties_case(dtype)
    cuts = srcs = 0
    for order in (1, 2):
        la = A.WordLookahead(lex, lm, order)
        for K in (1, 2, 3, 5, 8):
            for theta in (INF, 1.0, 0.0):
                info = {}
                _check(x, tr, lex, lm, la, il, K, theta, 1.0, 1.0, 0.0, info, "ties")
                cuts += info["tie_cuts"]
                srcs += info["src_ties"]
    assert cuts > 0 and srcs > 0


# ---------------------------------------------------------------------------------------------------------------- rescue
@DTYPES
def test_look_ahead_rescues_the_word_a_beam_of_one_prunes(dtype):
    A = _asg()
    lex, lm, x, tr = rescue_case(np.float32 if dtype == torch.float32 else np.float64)
    x, tr = torch.from_numpy(x), torch.from_numpy(tr)
    best = _gpu(x, tr, lex, lm, None, ALL)
    plain = _gpu(x, tr, lex, lm, None, 1)
    assert best["words"][0, 0] == 1 and plain["words"][0, 0] == 0 and plain["scores"][0] < best["scores"][0]
    for order in (1, 2):
        got = _check(x, tr, lex, lm, A.WordLookahead(lex, lm, order), None, 1, what="rescue")
        for n in NAMES:
            assert got[n].tobytes() == best[n].tobytes(), n


# ---------------------------------------------------------------------------------------------------------------- ends
@DTYPES
def test_dead_ends_are_pruned_and_every_kind_of_end(dtype):
    A = _asg()
    # the nodes [3] and [3, 0] have no word below them that the LM knows: edges into [3] are no candidates
    lex, lm = hand_case()
    x, tr = _normal(7, 4, 5, 37, dtype)
    x[:, :, 3] += 2.0                                      # acoustics like the dead branch
    il = torch.tensor([7, 4, 1, 0])
    for order in (1, 2, 3):
        for K in (2, 8, ALL):
            info = {}
            got = _check(x, tr, lex, lm, A.WordLookahead(lex, lm, order), il, K, INF, 0.7, -0.4, 0.3, info, "dead")
            assert info["dead"] > 0 and (got["states"] < 5).all()          # (the trie nodes 5 and 6 are [3] and [3, 0])
    assert [int(s) for s in np.flatnonzero(lex.word_of_state == 4)] == [6]
    # word 0 = [0] is unknown to the LM, word 1 = [0, 1] known: the node of word 0 lives (word 1 is below it), its end is
    # rejected; utterance 1 ends in the node of word 1 without a separator
    lex2 = A.Lexicon([[0], [0, 1]], 3, 2)
    lm2 = A.WordLM(2, [0, 1], [1], [-0.5], [0], [-1], [0.0], 0, [-1.0])
    tr2 = torch.zeros(3, 3, dtype=dtype)
    x2 = torch.full((5, 3, 3), -9.0, dtype=dtype)
    for t, lab in enumerate([0, 0, 0, 0, 0]):              # stays in the node of word 0: its end is rejected
        x2[t, 0, lab] = 0.0
    for t, lab in enumerate([0, 1, 2, 0, 0]):              # word 1, the separator, then the node of word 0 again: rejected
        x2[t, 1, lab] = 0.0
    for t, lab in enumerate([0, 1, 2, 0, 1]):              # ... and on into the node of word 1: an end in a word-end node
        x2[t, 2, lab] = 0.0
    info = {}
    got = _check(x2, tr2, lex2, lm2, A.WordLookahead(lex2, lm2, 2), None, 1, info=info, what="ends")
    assert [len(k[-1]) for k in info["kept"]] == [1, 1, 1]
    assert got["scores"][0] == -np.inf and got["scores"][1] == -np.inf and got["scores"][2] > -np.inf
    assert got["words"][2].tolist() == [1, 1, -1, -1, -1] and got["states"][2, -1] == 2
    got = _check(x2, tr2, lex2, lm2, A.WordLookahead(lex2, lm2, 1), None, 8, what="ends")
    assert (got["words"] != 0).all()


# ---------------------------------------------------------------------------------------------------------------- range query
@DTYPES
def test_a_range_query_over_every_level_of_the_table(dtype):
    A = _asg()
    words = [[0, 1 + i] for i in range(70)] + [[1], [1, 2], [1, 3], [2], [2, 3], [3]] + [[4, 5 + i] for i in range(5)]
    V = len(words)
    lex = A.Lexicon(words, 80, 79)
    rng = np.random.default_rng(12)
    sub = np.sort(rng.choice(V, 75, replace=False))
    lm = A.WordLM(V, [0, V, V + 75], np.concatenate([np.arange(V), sub]), -rng.uniform(0.1, 5.0, V + 75),
                  rng.integers(0, 2, V + 75), [-1, 0], [0.0, -0.3], 1, [-1.0, -2.0])
    la = A.WordLookahead(lex, lm, 2)
    assert np.diff(la.krow).max() > 64 and la.levels == 7 and {1, 2, 3, 5, 70} <= set((la.rhi - la.rlo).tolist())
    x, tr = _normal(6, 3, 80, 38, dtype)
    for K in (4, 64):
        info = {}
        _check(x * 0.5, tr * 0.25, lex, lm, la, torch.tensor([6, 5, 2]), K, INF, 0.8, -0.1, 0.2, info, "levels")
        assert {h for kl in info["kept"] for kept in kl for h, _ in kept} == {0, 1}        # both rows were read


# ---------------------------------------------------------------------------------------------------------------- wide
def test_wide_beam_strips_the_workgroup_and_loads_the_table():
    A = _asg()
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(6, 2, 40, 33, torch.float32)
    info = {}
    _check(x * 0.25, tr * 0.25, lex, lm, A.WordLookahead(lex, lm, 2), torch.tensor([6, 5]), 1200, INF, 0.5, -0.2, 0.1, info, "wide")
    assert max(max(c) for c in info["cands"]) > 1024 and max(max(s) for s in info["sizes"]) > 1024


# ---------------------------------------------------------------------------------------------------------------- plumbing
@DTYPES
def test_no_look_ahead_is_the_call_as_it_was(dtype):
    lex, lm, x, tr, il = grid_case(3, dtype)
    for K, theta in ((2, INF), (16, 3.0)):
        a = _gpu(x, tr, lex, lm, il, K, theta, 0.7, -0.4, 0.3)
        b = _gpu(x, tr, lex, lm, il, K, theta, 0.7, -0.4, 0.3, lookahead=None)
        want = beam_word_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), K, theta, 0.7, -0.4, 0.3)
        for n in NAMES:
            assert a[n].tobytes() == b[n].tobytes() == want[n].tobytes(), n


def test_capture_and_replay_with_new_emissions_and_lengths():
    A = _asg()
    lex, lm, x0, tr, _ = grid_case(3, torch.float32)
    la = A.WordLookahead(lex, lm, 2)
    T, B, N = 7, 4, 5
    x = torch.zeros(T, B, N, device=DEV)
    tr = tr.to(DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)
    args = (4, 3.0, 0.7, -0.4, 0.3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.beam_decode_words(x, tr, lex, lm, il, *args, lookahead=la)       # warm-up: compiles and caches lexicon, LM, look-ahead
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert la.compile(DEV, torch.float32, 0.7, -0.4) is la.compile(DEV, torch.float32, 0.7, -0.4)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = A.beam_decode_words(x, tr, lex, lm, il, *args, lookahead=la)
    for seed in (1, 2, 3):
        gen = torch.Generator().manual_seed(seed)
        x.copy_(torch.randn(T, B, N, generator=gen))
        il.copy_(torch.tensor([T, seed, 0, T - seed]))
        gr.replay()
        torch.cuda.synchronize()
        want = beam_word_la_ref(x.cpu().numpy(), tr.cpu().numpy(), lex, lm, 2, il.cpu().numpy(), *args)
        for n, u in zip(NAMES, out):
            assert u.cpu().numpy().tobytes() == want[n].tobytes(), n


def test_determinism_groups_strides_and_the_neighbours():
    A = _asg()
    lex, lm = wide_lexicon_and_lm()
    la = A.WordLookahead(lex, lm, 2)
    x, tr = _normal(12, 6, 40, 36, torch.float32)
    xd, trd = (x * 0.25).to(DEV), tr.to(DEV)
    ild = torch.tensor([12, 3, 0, 1, 11, 7], device=DEV)
    args = (100, 6.0, 0.5, -0.2, 0.1)
    plain_before = [o.cpu() for o in A.beam_decode_words(xd, trd, lex, lm, ild, *args)]
    graph_before = [o.cpu() for o in A.beam_decode_graph(xd, trd, lex.graph, ild, 6, 4.0, 0.8, -0.5)]
    a = A.beam_decode_words(xd, trd, lex, lm, ild, *args, lookahead=la)
    plain_after = [o.cpu() for o in A.beam_decode_words(xd, trd, lex, lm, ild, *args)]       # right after a look-ahead call
    graph_after = [o.cpu() for o in A.beam_decode_graph(xd, trd, lex.graph, ild, 6, 4.0, 0.8, -0.5)]
    for u, v in zip(plain_before + graph_before, plain_after + graph_after):
        assert torch.equal(u, v)
    assert any(not torch.equal(u.cpu(), v) for u, v in zip(a, plain_before))                 # it is another search
    for _ in range(2):
        b = A.beam_decode_words(xd, trd, lex, lm, ild, *args, lookahead=la)
        for u, v in zip(a, b):
            assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    from torch_asg_amd.asg import native
    be = native()
    seen = []
    buf = be._buf
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    try:
        A.beam_decode_words(xd, trd, lex, lm, ild, *args)
        plain_bytes = seen[-1]
        A.beam_decode_words(xd, trd, lex, lm, ild, *args, lookahead=la)
        assert seen[-1] == plain_bytes                     # no workspace of its own
        per = seen[-1] // 6
        small = A.beam_decode_words(xd, trd, lex, lm, ild, *args, max_work_bytes=2 * per + per // 2, lookahead=la)
        assert seen[-1] == 2 * per
    finally:
        del be._buf
    for u, v in zip(small, a):
        assert torch.equal(u, v)
    xt = xd.transpose(0, 1).contiguous().transpose(0, 1)                   # a strided [T,B,N] view
    for u, v in zip(A.beam_decode_words(xt, trd, lex, lm, ild, *args, lookahead=la), a):
        assert torch.equal(u, v)
    loss = A.ASGLoss(40).to(DEV)
    with torch.no_grad():
        loss.transition.copy_(trd)
    for u, v in zip(loss.beam_decode_words(xd, lex, lm, ild, *args, lookahead=la), a):
        assert torch.equal(u, v)
    xh = xd.to(torch.bfloat16)                                             # half precision is its widening
    for u, v in zip(A.beam_decode_words(xh, trd, lex, lm, ild, 50, lookahead=la),
                    A.beam_decode_words(xh.float(), trd, lex, lm, ild, 50, lookahead=la)):
        assert torch.equal(u, v)
