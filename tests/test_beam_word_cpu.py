"""CPU tests that pin the numpy restatement of beam decoding with a lexicon and a word LM (tests/beam_word_ref.py) before the
GPU tests compare the kernel with it: against the enumeration of every label path, against the restatement of the token-automaton
beam decoder (tests/beam_decode_ref.py) with the null LM and on a static composition of lexicon and LM, and the C ABI of
asg_beam_decode_words (sizes, argument checks) -- no kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch

from beam_decode_ref import beam_decode_ref
from beam_word_cases import (arpa_lm, best_by_enumeration, compose_static, eighths, path_score_words, small_lexicon,
                             without_unigrams)
from beam_word_ref import beam_word_ref

INF = float("inf")


def _emissions(T, B, N, seed, dt, grid=None):
    rng = np.random.default_rng(seed)
    if grid:                                              # multiples of 1 / grid
        return (rng.integers(-4 * grid, 4 * grid, (T, B, N)) / grid).astype(dt), (rng.integers(-2 * grid, 2 * grid, (N, N)) / grid).astype(dt)
    return rng.normal(size=(T, B, N)).astype(dt), rng.normal(size=(N, N)).astype(dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("order", [2, 3])
def test_a_full_beam_finds_the_best_of_all_label_paths(dt, order):
    from torch_asg_amd import Lexicon
    lex = Lexicon([[0], [0, 1], [1, 0], [2]], 4, 3, [0.25, -0.5, 0.0, 1.0])
    lm = without_unigrams(arpa_lm(4, order, 3 + order), {2})
    x, tr = _emissions(5, 3, 4, 21, dt)
    il = np.array([5, 4, 2])
    kw = dict(lm_weight=0.7, word_score=-0.4, token_score=0.3)
    got = beam_word_ref(x, tr, lex, lm, il, 10_000, INF, **kw)
    for b in range(3):
        L = int(il[b])
        want = best_by_enumeration(x[:L, b], tr, lex, lm, **kw)
        assert want > -np.inf and got["scores"][b] == want
        assert path_score_words(x[:L, b], tr, lex, lm, got["path"][b, :L], **kw) == want


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_null_lm_is_the_token_automaton_decoder(dt):
    from torch_asg_amd import WordLM
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    g = lex.graph
    x, tr = _emissions(9, 4, 5, 22, dt)
    il = np.array([9, 6, 1, 0])
    for K in (1, 2, 5, 50):
        for theta in (INF, 1.5, 0.0):
            got = beam_word_ref(x, tr, lex, WordLM.null(5), il, K, theta, token_score=-0.3)
            want = beam_decode_ref(x, tr, g.next, g.weight, g.final, 0, il, K, theta, 1.0, -0.3)
            for name, w in zip(("scores", "path", "tokens", "token_lengths", "states"), want):
                assert np.array_equal(got[name], w), (name, K, theta)
            assert ((got["lm_states"] == 0) == (got["path"] >= 0)).all()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("order", [2, 3])
def test_a_static_composition_in_eighths_gives_the_same_search(dt, order):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = without_unigrams(eighths(arpa_lm(5, order, 40 + order)), {3})
    S = lex.graph.S
    nxt, wt, fin, start = compose_static(lex, lm)
    x, tr = _emissions(8, 4, 5, 23, dt, grid=8)
    il = np.array([8, 5, 1, 0])
    seen = 0
    for K in (1, 2, 3, 8, 64, 10_000):
        for theta in (INF, 2.0, 0.0):
            info = {}
            got = beam_word_ref(x, tr, lex, lm, il, K, theta, token_score=0.125, info=info)
            sizes = []
            want = beam_decode_ref(x, tr, nxt, wt, fin, start, il, K, theta, 1.0, 0.125, sizes=sizes)
            for name, w in zip(("scores", "path", "tokens", "token_lengths"), want[:4]):
                assert np.array_equal(got[name], w), (name, K, theta)
            assert np.array_equal(np.where(got["path"] >= 0, got["lm_states"] * S + got["states"], -1), want[4])
            assert [s_ for s_ in info["sizes"] if s_] == sizes           # the same kept sets, frame by frame
            seen += sum(len({q for _, q in kept}) < len(kept) for kl in info["kept"] for kept in kl)
    assert seen > 0                                        # some frame kept one product state under two histories


def test_words_and_ends():
    from torch_asg_amd import Lexicon, WordLM
    lex = Lexicon([[0], [0, 1]], 3, 2)                     # nodes: 0 root, 1 "0" (word 0), 2 "01" (word 1)
    lm = WordLM.null(2)
    tr = np.zeros((3, 3))
    x = np.full((5, 3, 3), -9.0)
    for t, lab in enumerate([0, 2, 0, 1, 2]):              # ends at the root: words 0, 1
        x[t, 0, lab] = 0.0
    for t, lab in enumerate([0, 1, 2, 0, 1]):              # ends in a word-end node: words 1, then the final word 1
        x[t, 1, lab] = 0.0
    got = beam_word_ref(x, tr, lex, lm, np.array([5, 5, 5]), 8)
    assert got["words"][0].tolist() == [0, 1, -1, -1, -1] and got["word_lengths"][0] == 2 and got["scores"][0] == 0.0
    assert got["words"][1].tolist() == [1, 1, -1, -1, -1] and got["word_lengths"][1] == 2
    assert got["path"][1].tolist() == [0, 1, 2, 0, 1] and got["states"][1].tolist() == [1, 2, 0, 1, 2]
    # an LM that rejects word 1 everywhere: the second utterance must take another path, never word 1
    rej = WordLM(2, [0, 1], [0], [0.0], [0], [-1], [0.0], 0, [0.0])
    got = beam_word_ref(x, tr, lex, rej, np.array([5, 5, 5]), 8)
    assert (got["words"] != 1).all() and got["scores"][1] > -np.inf
    # nothing but mid-word ends: token 1 can only follow 0 inside word 1 ... a lexicon whose one word needs 3 frames, given 2
    long = Lexicon([[0, 1, 0]], 3, 2)
    got = beam_word_ref(x[:2], tr, long, WordLM.null(1), None, 8)
    assert (got["scores"] == -np.inf).all() and (got["path"] == -1).all() and (got["words"] == -1).all()
    assert (got["lm_states"] == -1).all() and (got["word_lengths"] == 0).all() and (got["token_lengths"] == 0).all()


def _abi(lex, lm, T, B, dtype=torch.float32, K=16):
    from torch_asg_amd import _lib, graph, wordlm
    c = lex.compile_words("cpu", dtype, 0.0)
    gb = graph.abi_graph_beam(c)
    w = wordlm.abi_word_lm(lm.compile("cpu", dtype, 1.0, 0.0), c)
    w.separator = lex.separator
    p = _lib.AsgProblem()
    x = torch.zeros(T, B, lex.graph.N, dtype=dtype)
    tr = torch.zeros(lex.graph.N, lex.graph.N, dtype=dtype)
    p.inputs, p.transition = x.data_ptr(), tr.data_ptr()
    p.T, p.B, p.N, p.S = T, B, lex.graph.N, 1
    p.dtype = _lib.ASG_DTYPE_F32 if dtype == torch.float32 else _lib.ASG_DTYPE_F64
    return _lib.lib(), p, gb, w, (c, x, tr)


def test_workspace_has_no_term_in_the_lm_or_the_vocabulary():
    lex = small_lexicon()
    small, big = arpa_lm(5, 2, 1), arpa_lm(5, 3, 1, keep=(1.0, 1.0, 1.0))
    assert big.H > 2 * small.H and big.A > 2 * small.A
    for T, B, K in ((7, 3, 16), (100, 2, 300)):
        L, p, gb, w, keep = _abi(lex, small, T, B)
        L2, p2, gb2, w2, keep2 = _abi(lex, big, T, B)
        a = int(L.asg_beam_decode_words_work_bytes(ctypes.byref(p), ctypes.byref(gb), ctypes.byref(w), K))
        b = int(L2.asg_beam_decode_words_work_bytes(ctypes.byref(p2), ctypes.byref(gb2), ctypes.byref(w2), K))
        assert a == b > 0
        # ... and is the documented formula
        al = lambda n: (n + 255) // 256 * 256                                                   # noqa: E731
        cap = max(K * (keep[0]["max_out"] + 1), keep[0]["num_start"])
        C = 2
        while C < 2 * cap:
            C *= 2
        assert a == B * (3 * al(T * K * 4) + 2 * al(C * 8) + al(C * 4) + al(cap * 4) + al(cap * 8) + al(cap * 4))
    # a lexicon of twice the words changes it only through the largest out-degree
    from torch_asg_amd import Lexicon
    wide = Lexicon([[0], [0, 1], [1, 0], [2], [0, 1, 2], [3], [3, 0], [2, 1], [1, 2, 0], [3, 1, 0]], 5, 4)
    L3, p3, gb3, w3, keep3 = _abi(wide, arpa_lm(10, 2, 1), 7, 3)
    L, p, gb, w, keep = _abi(lex, small, 7, 3)
    if keep3[0]["max_out"] == keep[0]["max_out"]:
        assert int(L3.asg_beam_decode_words_work_bytes(ctypes.byref(p3), ctypes.byref(gb3), ctypes.byref(w3), 16)) == \
            int(L.asg_beam_decode_words_work_bytes(ctypes.byref(p), ctypes.byref(gb), ctypes.byref(w), 16))


def test_abi_argument_checks_without_a_device():
    lex, lm = small_lexicon(), arpa_lm(5, 2, 1)
    L, p, gb, w, keep = _abi(lex, lm, 7, 3)
    wb = lambda K: int(L.asg_beam_decode_words_work_bytes(ctypes.byref(p), ctypes.byref(gb), ctypes.byref(w), K))  # noqa: E731
    assert wb(8192) > 0 and wb(8193) == 0 and wb(0) == 0
    out = [256] * 8                                        # non-null stand-ins: every check comes before anything is touched

    def call(K, th, work=256, nbytes=1 << 40, outs=out):
        return L.asg_beam_decode_words(None, ctypes.byref(p), ctypes.byref(gb), ctypes.byref(w), K, th, work, nbytes, *outs, 0, None)
    assert call(8193, 1.0) == 2                            # unsupported: no clamp to Q
    assert call(0, 1.0) == 1 and call(8, -1.0) == 1 and call(8, float("nan")) == 1
    assert call(8, 1.0, work=None) == 1 and call(8, 1.0, outs=[256] * 7 + [None]) == 1
    assert call(8, 1.0, nbytes=16) == 3                    # workspace too small
    w.dtype = 1 - w.dtype
    assert call(8, 1.0) == 1
    w.dtype = 1 - w.dtype
    for field, bad in (("start", lm.H), ("separator", 5), ("H", 0), ("row", None), ("word_of_state", None)):
        old = getattr(w, field)
        setattr(w, field, bad)
        assert call(8, 1.0) == 1, field
        setattr(w, field, old)
    w.H = (1 << 25) + 1
    assert call(8, 1.0) == 2                               # more histories than the pair word holds
    w.H = lm.H


def test_python_surface_refuses_bad_arguments_before_any_launch():
    import torch_asg_amd as A
    lex, lm = small_lexicon(), arpa_lm(5, 2, 1)
    x, tr = torch.zeros(4, 2, 5), torch.zeros(5, 5)
    with pytest.raises(ValueError, match="beam_size"):
        A.beam_decode_words(x, tr, lex, lm, beam_size=0)
    with pytest.raises(ValueError, match="beam_threshold"):
        A.beam_decode_words(x, tr, lex, lm, beam_threshold=-1.0)
    with pytest.raises(TypeError, match="Lexicon"):
        A.beam_decode_words(x, tr, lex.graph, lm)
    with pytest.raises(TypeError, match="WordLM"):
        A.beam_decode_words(x, tr, lex, None)
    with pytest.raises(RuntimeError, match="knows"):
        A.beam_decode_words(x, tr, lex, A.WordLM.null(3))
    assert hasattr(A.ASGLoss, "beam_decode_words") and A.BeamWords._fields[-2:] == ("words", "word_lengths")
