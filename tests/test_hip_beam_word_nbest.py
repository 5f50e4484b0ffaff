"""GPU tests (-m gpu) of the n best hypotheses of beam decoding with a lexicon and a word LM
(`torch_asg_amd.beam_decode_words_nbest`, `BeamWordStream.result_nbest`, csrc/asg_beam_word_nbest.hip): the bytes of every output
against the test-side numpy restatement (tests/beam_word_nbest_ref.py, pinned on the CPU by tests/test_beam_word_nbest_cpu.py).
Every case first asserts from the restatement that its input is in the regime it names; then the equivalences with the decoders
on the device, capture, determinism, grouping, the stream and errors."""
import functools

import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, compose_static, eighths, integers, small_lexicon, without_unigrams
from beam_word_nbest_cases import split_bound
from beam_word_nbest_ref import NAMES, BeamWordNbestStreamRef, beam_word_nbest_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
ALL = 1024                                                 # more than every pair of the small cases
ALIGN = ("path", "states", "lm_states")
STREAM_NAMES = ("scores", "graph_scores", "lm_scores", "tokens", "token_lengths", "words", "word_lengths", "num_hyps", "path",
                "states", "lm_states", "frames", "status")
ONE_BEST = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _np(out, names):
    assert out._fields == names
    return {n: (None if o is None else o.cpu().numpy()) for n, o in zip(names, out)}


def _gpu(x, tr, lex, lm, il, K, nbest, theta=INF, lw=1.0, ws=0.0, ts=0.0, align=True, **kw):
    out = _asg().beam_decode_words_nbest(x.to(DEV), tr.to(DEV), lex, lm, None if il is None else il.to(DEV), K, nbest, theta, lw, ws,
                                         ts, align, **kw)
    torch.cuda.synchronize()
    assert all(o.dtype == x.dtype for o in out[:4]) and all(o.dtype == torch.int64 for o in out[4:] if o is not None)
    return _np(out, NAMES)


def _first(want, nbest):
    """The restatement for a smaller nbest: its first rows (the order does not depend on nbest)."""
    res = {n: (v if n in ("num_hyps", "num_cands") else v[:, :nbest]) for n, v in want.items()}
    res["num_hyps"] = np.minimum(want["num_cands"], nbest)
    return res


def _same(got, want, names, what=""):
    for n in names:
        if got[n] is None:
            assert n in ALIGN
            continue
        assert got[n].shape == want[n].shape and got[n].dtype == want[n].dtype, (n, what)
        assert got[n].tobytes() == want[n].tobytes(), "%s %s" % (n, what)


def _check(x, tr, lex, lm, il, K, nbest, theta=INF, lw=1.0, ws=0.0, ts=0.0, align=True, info=None, what=""):
    got = _gpu(x, tr, lex, lm, il, K, nbest, theta, lw, ws, ts, align)
    want = beam_word_nbest_ref(x.numpy(), tr.numpy(), lex, lm, None if il is None else il.numpy(), K, nbest, theta, lw, ws, ts, info)
    _same(got, want, NAMES, "%s K=%d nbest=%d theta=%s" % (what, K, nbest, theta))
    return got, want


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
def test_grid_of_beams_thresholds_and_nbest(order, dtype):
    A = _asg()
    lex, lm, x, tr, il = grid_case(order, dtype)
    LW, WS, TS = 0.7, -0.4, 0.3
    padded = several = 0
    for K in (1, 2, 3, 8, 64, ALL):
        for theta in (INF, 2.0, 0.0):
            want = beam_word_nbest_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), K, K + 5, theta, LW, WS, TS)
            assert (want["num_cands"] <= K).all() and want["num_cands"][3] == 0
            several += int((want["num_cands"] > 1).sum())
            one = _np(A.beam_decode_words(x.to(DEV), tr.to(DEV), lex, lm, il.to(DEV), K, theta, LW, WS, TS), ONE_BEST)
            for nbest in (1, 2, K, K + 5):
                w = _first(want, nbest)
                padded += int((w["num_hyps"] < nbest).sum())
                for align in (False, True):
                    got = _gpu(x, tr, lex, lm, il, K, nbest, theta, LW, WS, TS, align)
                    _same(got, w, NAMES, "grid K=%d nbest=%d theta=%s" % (K, nbest, theta))
                    assert all((got[n] is None) != align for n in ALIGN)
                for n in ONE_BEST:                         # row 0 is the decoder's result, bit for bit
                    assert got[n][:, 0].tobytes() == one[n].tobytes(), (n, K, theta)
            diff, bound, fin = split_bound(want, x.numpy().dtype.type)
            assert (diff[fin] <= bound[fin]).all()
    assert padded > 0 and several > 0


# ---------------------------------------------------------------------------------------------------------------- ties
@DTYPES
def test_ties_between_ends_are_broken_by_h_then_q(dtype):
    lex = small_lexicon()
    lm = integers(arpa_lm(5, 2, 71, keep=(1.0, 0.6, 0.5)))
    g = torch.Generator().manual_seed(32)
    x = torch.randint(-2, 3, (8, 5, 5), generator=g).to(dtype)
    tr = torch.zeros(5, 5, dtype=dtype)
    il = torch.tensor([8, 8, 5, 1, 0])
    tied = same_q = 0
    for K in (3, 8, 64):
        for theta in (INF, 1.0):
            _, want = _check(x, tr, lex, lm, il, K, K, theta, 1.0, 1.0, 0.0, what="ties")
            for b in range(5):
                nh = int(want["num_hyps"][b])
                L = int(il[b])
                sc = want["scores"][b, :nh]
                tied += int((sc[1:] == sc[:-1]).sum())
                ends = [(int(want["lm_states"][b, r, L - 1]), int(want["states"][b, r, L - 1]), int(want["path"][b, r, L - 1]))
                        for r in range(nh)]
                for r in range(1, nh):
                    if sc[r] == sc[r - 1]:
                        assert ends[r - 1] < ends[r]       # pair order: h, then q (state and label ascend with q)
                qs = [e[1:] for e in ends]
                same_q += len(qs) - len(set(qs))
    assert tied > 0 and same_q > 0                         # two candidates on one q with different h among them


# ---------------------------------------------------------------------------------------------------------------- the sort's edges
@functools.lru_cache(maxsize=None)
def every_node_ends_a_word(N, two):
    """A lexicon whose every node is the root or a word end -- all one-token words and `two` two-token words -- and a bigram LM
    with every unigram: every kept pair has an end, so the candidates are the last set."""
    from torch_asg_amd import Lexicon
    rng = np.random.default_rng(7)
    words = [[i] for i in range(N - 1)]
    seen = set()
    while len(seen) < two:
        a, b = (int(v) for v in rng.integers(0, N - 1, 2))
        if a != b and (a, b) not in seen:
            seen.add((a, b))
            words.append([a, b])
    return Lexicon(words, N, N - 1), arpa_lm(len(words), 2, 73, keep=(1.0, 0.3))


@pytest.mark.parametrize("K", [63, 64, 65])
def test_63_64_65_candidates(K):
    lex, lm = every_node_ends_a_word(10, 0)
    x, tr = _normal(5, 2, 10, 37, torch.float32)
    _, want = _check(x * 0.25, tr * 0.25, lex, lm, None, K, K + 1, INF, 0.5, -0.2, 0.1, what="edge")
    assert (want["num_cands"] == K).all() and (want["num_hyps"] == K).all()


def test_more_than_1024_hypotheses_strip_the_lanes_and_the_workgroup():
    lex, lm = every_node_ends_a_word(40, 261)
    x, tr = _normal(5, 2, 40, 33, torch.float32)
    info = {}
    _, want = _check(x * 0.25, tr * 0.25, lex, lm, torch.tensor([5, 4]), 1200, 1200, INF, 0.5, -0.2, 0.1, info=info, what="wide")
    assert (want["num_hyps"] > 1024).all() and max(info["sizes"][0]) > 1024


@DTYPES
def test_the_largest_beam_the_lds_holds(dtype):
    A = _asg()
    lex, lm, x, tr, il = grid_case(2, dtype)
    _, want = _check(x[:4], tr, lex, lm, torch.tensor([4, 3, 1, 0]), 8192, 8192, INF, 0.7, -0.4, 0.3, what="K=8192")
    assert want["num_hyps"][0] > 8
    with pytest.raises(RuntimeError, match="unsupported|limit|support"):
        A.beam_decode_words_nbest(x.to(DEV), tr.to(DEV), lex, lm, il.to(DEV), 8193, 4)
    with pytest.raises(RuntimeError, match="unsupported|limit|support"):
        A.beam_decode_words_nbest(x.to(DEV), tr.to(DEV), lex, lm, il.to(DEV), 16, 8193)


@DTYPES
def test_the_64_frame_blocks_of_the_collapse(dtype):
    lex, lm, _, _, _ = grid_case(3, dtype)
    x, tr = _normal(130, 4, 5, 38, dtype)
    il = torch.tensor([63, 64, 65, 129])
    for align in (True, False):
        _, want = _check(x, tr, lex, lm, il, 8, 6, INF, 0.7, -0.4, 0.3, align, what="T=130")
    assert (want["num_hyps"] >= 2).all() and (want["token_lengths"][:, 0] > 8).all() and (want["word_lengths"][:, 0] > 4).all()


# ---------------------------------------------------------------------------------------------------------------- ends
@DTYPES
def test_every_kind_of_end_among_the_rows(dtype):
    from torch_asg_amd import Lexicon, WordLM
    lex = Lexicon([[0], [0, 1]], 3, 2)                     # nodes: 0 root, 1 "0" (word 0), 2 "01" (word 1)
    tr = torch.zeros(3, 3, dtype=dtype)
    x, _ = _normal(5, 3, 3, 39, dtype)
    lm = WordLM(2, [0, 2, 3], [0, 1, 0], [-0.5, -1.0, -0.25], [1, 1, 0], [-1, 0], [0.0, -0.125], 0, [-2.0, -0.75])
    info = {}
    _, want = _check(x, tr, lex, lm, None, 16, 16, info=info, what="ends")
    last = want["states"][:, :, 4]
    rows = np.arange(16)[None] < want["num_hyps"][:, None]
    assert (rows & (last == 0)).any() and (rows & (last == 1)).any() and (rows & (last == 2)).any()
    wl = want["word_lengths"]
    fin_word = np.take_along_axis(want["words"], np.maximum(wl - 1, 0)[..., None], 2)[..., 0]
    assert (fin_word[rows & (last == 2)] == 1).all() and (fin_word[rows & (last == 1)] == 0).all()      # the final word is there
    # an LM that knows word 0 only: a pair kept in the node of word 1 has no end and is no row
    rej = WordLM(2, [0, 1], [0], [-0.5], [0], [-1], [0.0], 0, [-1.0])
    info = {}
    _, want = _check(x, tr, lex, rej, None, 16, 16, info=info, what="rejected")
    assert (want["num_cands"] < np.array([s[-1] for s in info["sizes"]])).all() and (want["num_hyps"] > 0).all()
    assert (want["words"] != 1).all() and not (want["states"][:, :, 4] == 2).any()
    # every path ends mid-word: the beam is full and there is no row
    long = Lexicon([[0, 1, 0]], 3, 2)
    info = {}
    got, want = _check(x[:2], tr, long, WordLM.null(1), None, 8, 3, info=info, what="mid-word")
    assert all(s[-1] > 0 for s in info["sizes"]) and (got["num_hyps"] == 0).all() and (got["scores"] == -np.inf).all()


# ---------------------------------------------------------------------------------------------------------------- equivalences
@DTYPES
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_a_static_composition_in_eighths_equals_the_token_automaton_nbest(order, dtype):
    A = _asg()
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = without_unigrams(eighths(arpa_lm(5, order, 40 + order)), {3})
    static = A.TokenGraph(*compose_static(lex, lm))
    g = torch.Generator().manual_seed(35)
    x = (torch.randint(-32, 32, (8, 4, 5), generator=g) / 8.0).to(dtype)
    tr = (torch.randint(-16, 16, (5, 5), generator=g) / 8.0).to(dtype)
    il = torch.tensor([8, 5, 1, 0])
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    rows = 0
    for K in (1, 3, 8, 64, ALL):
        for theta in (INF, 2.0):
            nbest = min(K, 40)
            got = _gpu(x, tr, lex, lm, il, K, nbest, theta, ts=0.125, align=False)
            want = A.beam_decode_graph_nbest(xd, trd, static, ild, K, nbest, theta, 1.0, 0.125)
            for n in ("scores", "tokens", "token_lengths", "num_hyps", "emission_scores"):
                assert np.array_equal(got[n], getattr(want, n).cpu().numpy()), (n, K, theta)
            assert np.array_equal(got["graph_scores"] + got["lm_scores"], want.graph_scores.cpu().numpy()), (K, theta)
            assert np.array_equal(got["scores"], got["emission_scores"] + (got["graph_scores"] + got["lm_scores"]))      # exact
            rows += int(got["num_hyps"].sum())
    assert rows > 100


@DTYPES
def test_the_null_lm_equals_the_token_automaton_nbest(dtype):
    A = _asg()
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    x, tr = _normal(9, 4, 5, 34, dtype)
    il = torch.tensor([9, 6, 1, 0])
    for K in (1, 3, 7, 12):
        for theta in (INF, 1.5):
            got = _gpu(x, tr, lex, A.WordLM.null(5), il, K, 5, theta, ts=-0.3)
            want = A.beam_decode_graph_nbest(x.to(DEV), tr.to(DEV), lex.graph, il.to(DEV), K, 5, theta, 1.0, -0.3, True)
            for n in ("scores", "emission_scores", "graph_scores", "tokens", "token_lengths", "num_hyps", "path", "states"):
                assert np.array_equal(got[n], getattr(want, n).cpu().numpy()), (n, K, theta)
            fin = np.isfinite(got["scores"])
            assert (got["lm_scores"][fin] == 0).all() and (got["lm_scores"][~fin] == -np.inf).all()


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_capture_and_replay_with_new_emissions_and_lengths():
    A = _asg()
    lex, lm, x0, tr, _ = grid_case(3, torch.float32)
    T, B, N = 7, 4, 5
    x = torch.zeros(T, B, N, device=DEV)
    tr = tr.to(DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)
    args = (16, 6, 3.0, 0.7, -0.4, 0.3, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.beam_decode_words_nbest(x, tr, lex, lm, il, *args)      # warm-up: compiles and caches lexicon and LM
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = A.beam_decode_words_nbest(x, tr, lex, lm, il, *args)
    for seed in (1, 2, 3):
        gen = torch.Generator().manual_seed(seed)
        x.copy_(torch.randn(T, B, N, generator=gen))
        il.copy_(torch.tensor([T, seed, 0, T - seed]))
        gr.replay()
        torch.cuda.synchronize()
        want = beam_word_nbest_ref(x.cpu().numpy(), tr.cpu().numpy(), lex, lm, il.cpu().numpy(), *args[:6])
        _same(_np(out, NAMES), want, NAMES, "replay %d" % seed)


def test_two_runs_give_identical_bits_and_groups_equal_one_call():
    A = _asg()
    lex, lm = every_node_ends_a_word(40, 261)
    x, tr = _normal(10, 6, 40, 36, torch.float32)
    xd, trd = (x * 0.25).to(DEV), tr.to(DEV)
    ild = torch.tensor([10, 3, 0, 1, 9, 7], device=DEV)
    args = (300, 40, 6.0, 0.5, -0.2, 0.1, True)
    a = A.beam_decode_words_nbest(xd, trd, lex, lm, ild, *args)
    assert int(a.num_hyps.max()) == 40
    for _ in range(2):
        b = A.beam_decode_words_nbest(xd, trd, lex, lm, ild, *args)
        for u, v in zip(a, b):
            assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    from torch_asg_amd.asg import native
    be = native()
    seen = []
    buf = be._buf
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    try:
        A.beam_decode_words_nbest(xd, trd, lex, lm, ild, *args)
        per = seen[-1] // 6
        small = A.beam_decode_words_nbest(xd, trd, lex, lm, ild, *args, max_work_bytes=2 * per + per // 2)
        assert seen[-1] < 3 * per
    finally:
        del be._buf
    for u, v in zip(small, a):
        assert torch.equal(u, v)
    # a strided [T,B,N] view, the module method, and half precision as its widening
    xt = xd.transpose(0, 1).contiguous().transpose(0, 1)
    for u, v in zip(A.beam_decode_words_nbest(xt, trd, lex, lm, ild, *args), a):
        assert torch.equal(u, v)
    loss = A.ASGLoss(40).to(DEV)
    with torch.no_grad():
        loss.transition.copy_(trd)
    for u, v in zip(loss.beam_decode_words_nbest(xd, lex, lm, ild, *args), a):
        assert torch.equal(u, v)
    xh = xd.to(torch.bfloat16)
    for u, v in zip(A.beam_decode_words_nbest(xh, trd, lex, lm, ild, 50, 5), A.beam_decode_words_nbest(xh.float(), trd, lex, lm, ild, 50, 5)):
        assert u is v or torch.equal(u, v)


def test_the_other_decoders_are_undisturbed_by_nbest_calls():
    A = _asg()
    lex, lm, x, tr, il = grid_case(3, torch.float32)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    stream = A.BeamWordStream(trd, lex, lm, 4, 7, 16, 4.0, 0.7, -0.4, 0.3)
    stream.advance(xd, ild)

    def others():
        outs = list(A.beam_decode_words(xd, trd, lex, lm, ild, 64, 4.0, 0.7, -0.4, 0.3)) + list(stream.result(True))
        outs += list(A.beam_decode_graph(xd, trd, lex.graph, ild, 6, 4.0, 0.8, -0.5))
        outs += [o for o in A.beam_decode_graph_nbest(xd, trd, lex.graph, ild, 6, 3, 4.0, 0.8, -0.5) if o is not None]
        return [o.cpu() for o in outs]
    before = others()
    A.beam_decode_words_nbest(xd, trd, lex, lm, ild, 64, 10, 4.0, 0.7, -0.4, 0.3, True)
    stream.result_nbest(5, True, True)
    stream.result_nbest(5, False)
    for u, v in zip(before, others()):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------------------------- stream
CHUNKINGS = ([12], [1] * 12, [5, 7], [3, 0, 4, 1, 4])


@DTYPES
@pytest.mark.parametrize("chunks", CHUNKINGS, ids=["whole", "frames", "two", "ragged"])
def test_stream_prefixes_after_every_chunk_and_the_one_shot_rows_at_the_end(chunks, dtype):
    A = _asg()
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(12, 4, 5, 46, dtype)
    il = torch.tensor([12, 5, 1, 0])
    K, NB, args = 12, 8, (5.0, 0.7, -0.4, 0.3)            # at the end: 10 candidates in slot 0 (cut to 8), 4 in slot 1 (padded)
    s = A.BeamWordStream(tr.to(DEV), lex, lm, 4, 12, K, *args, dtype=dtype)
    ref = BeamWordNbestStreamRef(tr.numpy(), lex, lm, 4, 12, K, *args, dtype=x.numpy().dtype)
    t0 = 0
    mid_word = 0
    wos = np.asarray(lex.word_of_state)
    for n in chunks:
        cl = (il - t0).clamp(0, n)
        s.advance(x[t0:t0 + n].to(DEV), cl.to(DEV))
        ref.advance(x[t0:t0 + n].numpy(), cl.numpy())
        t0 += n
        before = s._state.clone()
        want = ref.result_nbest(NB, False)
        for align in (False, True):
            got = _np(s.result_nbest(NB, False, align), STREAM_NAMES)
            _same(got, want, STREAM_NAMES, "prefix after %d" % t0)
        one = s.result(False)
        for n_ in ONE_BEST:
            assert got[n_][:, 0].tobytes() == getattr(one, n_).cpu().numpy().tobytes(), n_
        assert torch.equal(before, s._state)               # it reads the state only
        for b in range(4):
            L, nh = int(want["frames"][b]), int(want["num_hyps"][b])
            if L:
                last = want["states"][b, :nh, L - 1]
                mid_word += int(((last != 0) & (wos[last] < 0)).sum())
    assert mid_word > 0                                    # prefixes that end mid-word are rows
    before = s._state.clone()
    got = _np(s.result_nbest(NB, True, True), STREAM_NAMES)
    assert torch.equal(before, s._state)
    _same(got, ref.result_nbest(NB, True), STREAM_NAMES, "final")
    shot = _gpu(x, tr, lex, lm, il, K, NB, *args)
    for n in STREAM_NAMES[:-2]:
        assert got[n].tobytes() == shot[n].tobytes(), n    # the one-shot call's bits, for this chunking
    assert (shot["num_hyps"][:2] >= 2).all() and got["frames"].tolist() == [12, 5, 1, 0]
    last = got["states"][0, :got["num_hyps"][0], 11]
    assert ((last == 0) | (wos[last] >= 0)).all()          # with the end, no row ends mid-word


def test_a_captured_advance_and_result_nbest_is_replayed():
    A = _asg()
    lex, lm, x0, tr, _ = grid_case(3, torch.float32)
    K, NB, args = 6, 4, (3.0, 0.7, -0.4, 0.3)
    s = A.BeamWordStream(tr.to(DEV), lex, lm, 4, 12, K, *args)
    chunk = torch.zeros(3, 4, 5, device=DEV)
    cl = torch.full((4,), 3, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.advance(chunk, cl)                               # warm-up; the scratch of result_nbest is allocated here
        s.result_nbest(NB, False, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    s.reset()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        s.advance(chunk, cl)
        out = s.result_nbest(NB, False, True)
    s.reset()
    ref = BeamWordNbestStreamRef(tr.numpy(), lex, lm, 4, 12, K, *args)
    for seed in (1, 2, 3):
        gen = torch.Generator().manual_seed(seed)
        chunk.copy_(torch.randn(3, 4, 5, generator=gen))
        cl.copy_(torch.tensor([3, seed, 0, 2]))
        gr.replay()
        torch.cuda.synchronize()
        ref.advance(chunk.cpu().numpy(), cl.cpu().numpy())
        _same(_np(out, STREAM_NAMES), ref.result_nbest(NB, False), STREAM_NAMES, "replay %d" % seed)


def test_errors():
    A = _asg()
    lex, lm, x, tr, il = grid_case(2, torch.float32)
    xd, trd = x.to(DEV), tr.to(DEV)
    with pytest.raises(RuntimeError):
        A.beam_decode_words_nbest(x, tr, lex, lm, beam_size=4, nbest=2)                   # CPU tensors
    with pytest.raises(RuntimeError, match="tokens"):
        A.beam_decode_words_nbest(torch.randn(4, 2, 6, device=DEV), torch.randn(6, 6, device=DEV), lex, lm, beam_size=4)
    with pytest.raises(RuntimeError):
        A.beam_decode_words_nbest(xd, trd, lex, lm, torch.tensor([4, 4], device=DEV), beam_size=4)
    with pytest.raises(TypeError):
        A.beam_decode_words_nbest(xd, trd, lex.graph, lm, beam_size=4)
    with pytest.raises(RuntimeError, match="knows"):
        A.beam_decode_words_nbest(xd, trd, lex, A.WordLM.null(2), beam_size=4)
    for kw in (dict(beam_size=0), dict(beam_size=4, nbest=0), dict(beam_size=4, beam_threshold=-1.0)):
        with pytest.raises(ValueError):
            A.beam_decode_words_nbest(xd, trd, lex, lm, **kw)
    s = A.BeamWordStream(trd, lex, lm, 4, 7, 8)
    with pytest.raises(ValueError, match="nbest"):
        s.result_nbest(0)
    with pytest.raises(RuntimeError, match="unsupported|limit|support"):
        s.result_nbest(8193)
    got = s.result_nbest(3, True)                          # no frame yet: no rows
    assert (got.num_hyps == 0).all() and (got.scores == -INF).all() and (got.tokens == -1).all() and (got.frames == 0).all()
