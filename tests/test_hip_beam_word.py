"""GPU tests (-m gpu) of beam decoding with a lexicon and a word LM composed on the fly (`torch_asg_amd.beam_decode_words`,
csrc/asg_beam_word.hip): every output bit-identical to the test-side numpy restatement (tests/beam_word_ref.py, pinned on the
CPU by tests/test_beam_word_cpu.py).  Every case first asserts, from the restatement's own sets, that its input is in the regime
it names: two histories on one product state, ties cut at the K-th value and decided by source-pair order, more candidates and
kept pairs than the workgroup has threads, the largest beam the LDS holds, every kind of end; then the equivalences with the
token-automaton decoders on the device, capture, determinism, grouping and errors."""
import functools

import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, compose_static, eighths, integers, small_lexicon, without_unigrams
from beam_word_ref import beam_word_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
NAMES = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths")
ALL = 1024                                                 # more than every pair of the small cases
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


def _check(x, tr, lex, lm, il, K, theta=INF, lw=1.0, ws=0.0, ts=0.0, info=None, what=""):
    got = _gpu(x, tr, lex, lm, il, K, theta, lw, ws, ts)
    want = beam_word_ref(x.numpy(), tr.numpy(), lex, lm, None if il is None else il.numpy(), K, theta, lw, ws, ts, info=info)
    for n in NAMES:
        assert np.array_equal(got[n], want[n]), "%s %s K=%d theta=%s" % (n, what, K, theta)
    return got


def _normal(T, B, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, B, N, generator=g, dtype=torch.float64).to(dtype), torch.randn(N, N, generator=g, dtype=torch.float64).to(dtype)


# ---------------------------------------------------------------------------------------------------------------- grid
def grid_case(order, dtype):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, order, 60 + order, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(7, 4, 5, 31, dtype)
    return lex, lm, x, tr, torch.tensor([7, 4, 1, 0])


@DTYPES
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_grid_of_beams_and_thresholds(order, dtype):
    A = _asg()
    lex, lm, x, tr, il = grid_case(order, dtype)
    LW, WS, TS = 0.7, -0.4, 0.3
    if order == 3:                                         # the trigram has histories that back off twice
        assert (lm.backoff[lm.backoff[lm.backoff >= 0]] >= 0).any()
    shared = 0
    for K in (1, 2, 3, 8, 64, ALL):
        for theta in (INF, 2.0, 0.0):
            info = {}
            got = _check(x, tr, lex, lm, il, K, theta, LW, WS, TS, info, "grid")
            shared += sum(len({q for _, q in kept}) < len(kept) for kl in info["kept"] for kept in kl)
            if K == ALL and theta == INF:
                assert max(max(s) for s in info["sizes"] if s) < ALL
                plain = A.beam_decode_graph(x.to(DEV), tr.to(DEV), lex.graph, il.to(DEV), ALL, INF, 1.0, TS)
                differs = not np.array_equal(plain[1].cpu().numpy(), got["path"])
    assert shared > 0                                      # some frame kept two pairs with one q and different h
    assert differs                                         # the LM changed a best path: ignoring it cannot pass


# ---------------------------------------------------------------------------------------------------------------- ties
def ties_case(dtype):
    lex = small_lexicon()
    lm = integers(arpa_lm(5, 2, 71, keep=(1.0, 0.6, 0.5)))
    g = torch.Generator().manual_seed(32)
    x = torch.randint(-2, 3, (8, 5, 5), generator=g).to(dtype)
    return lex, lm, x, torch.zeros(5, 5, dtype=dtype), torch.tensor([8, 8, 5, 1, 0])


@DTYPES
def test_ties_at_the_last_rank_and_between_sources(dtype):
    lex, lm, x, tr, il = ties_case(dtype)
    cuts = srcs = 0
    for K in (1, 2, 3, 5, 8):
        for theta in (INF, 1.0, 0.0):
            info = {}
            _check(x, tr, lex, lm, il, K, theta, 1.0, 1.0, 0.0, info, "ties")
            cuts += info["tie_cuts"]
            srcs += info["src_ties"]
    assert cuts > 0 and srcs > 0


# ---------------------------------------------------------------------------------------------------------------- wide
@functools.lru_cache(maxsize=None)
def wide_lexicon_and_lm():
    from torch_asg_amd import Lexicon
    rng = np.random.default_rng(5)
    words, seen = [], set()
    while len(words) < 300:
        n = int(rng.integers(1, 4))
        w = tuple(int(t) for t in rng.integers(0, 39, n))
        if w in seen or any(a == b for a, b in zip(w, w[1:])):
            continue
        seen.add(w)
        words.append(list(w))
    return Lexicon(words, 40, 39), arpa_lm(300, 2, 72, keep=(1.0, 0.03))


def test_wide_beam_strips_the_workgroup_and_loads_the_table():
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(6, 2, 40, 33, torch.float32)
    x = x * 0.25                                           # flat emissions: many pairs stay close
    info = {}
    _check(x, tr * 0.25, lex, lm, torch.tensor([6, 5]), 1200, INF, 0.5, -0.2, 0.1, info, "wide")
    assert max(max(c) for c in info["cands"]) > 1024 and max(max(s) for s in info["sizes"]) > 1024


# ---------------------------------------------------------------------------------------------------------------- large LDS
@DTYPES
def test_the_largest_beam_the_lds_holds(dtype):
    A = _asg()
    lex, lm, x, tr, il = grid_case(2, dtype)
    _check(x[:4], tr, lex, lm, torch.tensor([4, 3, 1, 0]), 8192, INF, 0.7, -0.4, 0.3, what="K=8192")
    with pytest.raises(RuntimeError, match="unsupported|limit|support"):
        A.beam_decode_words(x.to(DEV), tr.to(DEV), lex, lm, il.to(DEV), 8193)


# ---------------------------------------------------------------------------------------------------------------- ends
@DTYPES
def test_every_kind_of_end(dtype):
    from torch_asg_amd import Lexicon, WordLM
    lex = Lexicon([[0], [0, 1]], 3, 2)                     # nodes: 0 root, 1 "0" (word 0), 2 "01" (word 1)
    tr = torch.zeros(3, 3, dtype=dtype)
    x = torch.full((5, 3, 3), -9.0, dtype=dtype)
    for t, lab in enumerate([0, 2, 0, 1, 2]):              # ends at the root
        x[t, 0, lab] = 0.0
    for t, lab in enumerate([0, 1, 2, 0, 1]):              # ends in a word-end node
        x[t, 1, lab] = 0.0
    il = torch.tensor([5, 5, 5])
    lm = WordLM(2, [0, 2, 3], [0, 1, 0], [-0.5, -1.0, -0.25], [1, 1, 0], [-1, 0], [0.0, -0.125], 0, [-2.0, -0.75])
    got = _check(x, tr, lex, lm, il, 8, what="ends")
    assert got["words"][0].tolist() == [0, 1, -1, -1, -1] and got["path"][0].tolist() == [0, 2, 0, 1, 2]
    assert got["words"][1].tolist() == [1, 1, -1, -1, -1] and got["word_lengths"].tolist()[:2] == [2, 2]
    # an LM that knows word 0 only: the step of word 1 is rejected on its separator edge and at the end
    rej = WordLM(2, [0, 1], [0], [-0.5], [0], [-1], [0.0], 0, [-1.0])
    got = _check(x, tr, lex, rej, il, 8, what="rejected")
    assert (got["words"] != 1).all() and (got["scores"] > -np.inf).all()
    # every path ends mid-word: no hypothesis
    long = Lexicon([[0, 1, 0]], 3, 2)
    got = _check(x[:2], tr, long, WordLM.null(1), None, 8, what="mid-word")
    assert (got["scores"] == -np.inf).all()
    for n in NAMES[1:]:
        assert (got[n] == (0 if n.endswith("lengths") else -1)).all(), n


# ---------------------------------------------------------------------------------------------------------------- equivalences
@DTYPES
def test_the_null_lm_equals_the_token_automaton_beam_decoder(dtype):
    A = _asg()
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    x, tr = _normal(9, 4, 5, 34, dtype)
    il = torch.tensor([9, 6, 1, 0])
    for K in (1, 3, 7, 12):
        for theta in (INF, 1.5):
            got = _gpu(x, tr, lex, A.WordLM.null(5), il, K, theta, ts=-0.3)
            want = A.beam_decode_graph(x.to(DEV), tr.to(DEV), lex.graph, il.to(DEV), K, theta, 1.0, -0.3)
            for n, w in zip(NAMES[:5], want):
                assert np.array_equal(got[n], w.cpu().numpy()), (n, K, theta)


@DTYPES
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_a_static_composition_in_eighths_equals_the_token_automaton_decoders(order, dtype):
    A = _asg()
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = without_unigrams(eighths(arpa_lm(5, order, 40 + order)), {3})
    static = A.TokenGraph(*compose_static(lex, lm))
    S = lex.graph.S
    g = torch.Generator().manual_seed(35)
    x = (torch.randint(-32, 32, (8, 4, 5), generator=g) / 8.0).to(dtype)
    tr = (torch.randint(-16, 16, (5, 5), generator=g) / 8.0).to(dtype)
    il = torch.tensor([8, 5, 1, 0])
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    for K in (1, 2, 3, 8, 64, ALL):
        for theta in (INF, 2.0, 0.0):
            got = _gpu(x, tr, lex, lm, il, K, theta, ts=0.125)
            want = [o.cpu().numpy() for o in A.beam_decode_graph(xd, trd, static, ild, K, theta, 1.0, 0.125)]
            for n, w in zip(NAMES[:4], want):
                assert np.array_equal(got[n], w), (n, K, theta)
            assert np.array_equal(np.where(got["path"] >= 0, got["lm_states"] * S + got["states"], -1), want[4])
    exact = [o.cpu().numpy() for o in A.viterbi_decode_graph(xd, trd, static, ild, 1.0, 0.125)]
    got = _gpu(x, tr, lex, lm, il, ALL, INF, ts=0.125)
    for n, w in zip(NAMES[:4], exact):
        assert np.array_equal(got[n], w), n


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_capture_and_replay_with_new_emissions_and_lengths():
    A = _asg()
    lex, lm, x0, tr, _ = grid_case(3, torch.float32)
    T, B, N = 7, 4, 5
    x = torch.zeros(T, B, N, device=DEV)
    tr = tr.to(DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)
    args = (16, 3.0, 0.7, -0.4, 0.3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.beam_decode_words(x, tr, lex, lm, il, *args)     # warm-up: compiles and caches lexicon and LM
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = A.beam_decode_words(x, tr, lex, lm, il, *args)
    for seed in (1, 2, 3):
        gen = torch.Generator().manual_seed(seed)
        x.copy_(torch.randn(T, B, N, generator=gen))
        il.copy_(torch.tensor([T, seed, 0, T - seed]))
        gr.replay()
        torch.cuda.synchronize()
        eager = A.beam_decode_words(x, tr, lex, lm, il, *args)
        for u, v in zip(out, eager):
            assert torch.equal(u, v)
        want = beam_word_ref(x.cpu().numpy(), tr.cpu().numpy(), lex, lm, il.cpu().numpy(), *args)
        for n, u in zip(NAMES, out):
            assert np.array_equal(u.cpu().numpy(), want[n]), n


def test_two_runs_give_identical_bits_and_groups_equal_one_call():
    A = _asg()
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(12, 6, 40, 36, torch.float32)
    xd, trd = (x * 0.25).to(DEV), tr.to(DEV)
    ild = torch.tensor([12, 3, 0, 1, 11, 7], device=DEV)
    args = (300, 6.0, 0.5, -0.2, 0.1)
    a = A.beam_decode_words(xd, trd, lex, lm, ild, *args)
    for _ in range(2):
        b = A.beam_decode_words(xd, trd, lex, lm, ild, *args)
        for u, v in zip(a, b):
            assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    from torch_asg_amd.asg import native
    be = native()
    seen = []
    buf = be._buf
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    try:
        A.beam_decode_words(xd, trd, lex, lm, ild, *args)
        per = seen[-1] // 6
        small = A.beam_decode_words(xd, trd, lex, lm, ild, *args, max_work_bytes=2 * per + per // 2)
        assert seen[-1] == 2 * per
    finally:
        del be._buf
    for u, v in zip(small, a):
        assert torch.equal(u, v)
    # a strided [T,B,N] view, the module method, and half precision as its widening
    xt = xd.transpose(0, 1).contiguous().transpose(0, 1)
    for u, v in zip(A.beam_decode_words(xt, trd, lex, lm, ild, *args), a):
        assert torch.equal(u, v)
    loss = A.ASGLoss(40).to(DEV)
    with torch.no_grad():
        loss.transition.copy_(trd)
    for u, v in zip(loss.beam_decode_words(xd, lex, lm, ild, *args), a):
        assert torch.equal(u, v)
    for hd in (torch.float16, torch.bfloat16):
        xh = xd.to(hd)
        for u, v in zip(A.beam_decode_words(xh, trd, lex, lm, ild, 50), A.beam_decode_words(xh.float(), trd, lex, lm, ild, 50)):
            assert torch.equal(u, v)
    # compiled once per (device, dtype, weights)
    assert lm.compile(DEV, torch.float32, 0.5, -0.2) is lm.compile(DEV, torch.float32, 0.5, -0.2)
    assert lex.compile_words(DEV, torch.float32, 0.1) is lex.compile_words(DEV, torch.float32, 0.1)


def test_the_token_automaton_decoders_are_undisturbed_by_a_call():
    A = _asg()
    lex, lm, x, tr, il = grid_case(3, torch.float32)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    before = [o.cpu() for o in A.beam_decode_graph(xd, trd, lex.graph, ild, 6, 4.0, 0.8, -0.5)]
    nb_before = A.beam_decode_graph_nbest(xd, trd, lex.graph, ild, 6, 3, 4.0, 0.8, -0.5)
    nb_before = [o.cpu() for o in nb_before if o is not None]
    A.beam_decode_words(xd, trd, lex, lm, ild, 64, 4.0, 0.7, -0.4, 0.3)
    after = [o.cpu() for o in A.beam_decode_graph(xd, trd, lex.graph, ild, 6, 4.0, 0.8, -0.5)]
    A.beam_decode_words(xd, trd, lex, lm, ild, 64, 4.0, 0.7, -0.4, 0.3)
    nb_after = [o.cpu() for o in A.beam_decode_graph_nbest(xd, trd, lex.graph, ild, 6, 3, 4.0, 0.8, -0.5) if o is not None]
    for u, v in zip(before + nb_before, after + nb_after):
        assert torch.equal(u, v)


def test_errors():
    A = _asg()
    lex, lm, x, tr, il = grid_case(2, torch.float32)
    xd, trd = x.to(DEV), tr.to(DEV)
    with pytest.raises(RuntimeError):
        A.beam_decode_words(x, tr, lex, lm, beam_size=4)                   # CPU tensors
    with pytest.raises(RuntimeError, match="tokens"):
        A.beam_decode_words(torch.randn(4, 2, 6, device=DEV), torch.randn(6, 6, device=DEV), lex, lm, beam_size=4)
    with pytest.raises(RuntimeError):
        A.beam_decode_words(xd, trd.double(), lex, lm, beam_size=4)
    with pytest.raises(RuntimeError):
        A.beam_decode_words(xd, trd, lex, lm, torch.tensor([4, 4], device=DEV), beam_size=4)
    with pytest.raises(TypeError):
        A.beam_decode_words(xd, trd, lex.graph, lm, beam_size=4)
    with pytest.raises(RuntimeError, match="knows"):
        A.beam_decode_words(xd, trd, lex, A.WordLM.null(2), beam_size=4)
    for kw in (dict(beam_size=0), dict(beam_size=4, beam_threshold=-1.0), dict(beam_size=4, beam_threshold=float("nan"))):
        with pytest.raises(ValueError):
            A.beam_decode_words(xd, trd, lex, lm, **kw)
