"""GPU tests (-m gpu) of the property that csrc/asg_beam_word_search.h turns into text: the four one-shot calls of the lexicon +
word-LM beam family -- `beam_decode_words`, `beam_decode_words_confidence`, `beam_decode_words_nbest`,
`beam_decode_words_nbest_confidence` -- and the loss's `beam_words_full_score` run ONE search (`beam_word_search<R, TRL, LA,
FIN, mode>`), so what they share they share bit for bit.

Cases: both sides of the transitions-in-LDS edge 4096 + K (e + 8) + N N e <= 160 KiB at beam_size = 8 (float32 N = 199 | 200,
float64 N = 141 | 142), each without look-ahead and with one of order 2: every TRL x LA instantiation of every mode, FIN and
not.  T = 6, B = 3 with input_lengths (6, 1, 0): the table-clearing path, the one-frame path that skips it and the no-path
fill.  beam_threshold = 8 prunes and leaves the first utterance its path of three words (asserted on the restatement's kept sets)."""
import functools

import numpy as np
import pytest
import torch

import beam_word_regime_cases as C
from beam_word_ref import beam_word_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
K, NBEST, THETA, TOL = 8, 3, 8.0, 1
W = (0.7, -0.4, 0.3)               # lm_weight, word_score, token_score
LENGTHS = (6, 1, 0)
CASES = [(torch.float32, 199), (torch.float32, 200), (torch.float64, 141), (torch.float64, 142)]
NP = {torch.float32: np.float32, torch.float64: np.float64}


def _asg():
    import torch_asg_amd
    return torch_asg_amd


@functools.lru_cache(maxsize=None)
def _inputs(dtype, N):
    """layout_inputs' emissions for three utterances: the first spells the lexicon's words, the others are noise."""
    x2, tr, _ = C.layout_inputs(N, NP[dtype])
    x = np.concatenate([x2, np.random.default_rng(5).standard_normal((6, 1, N)).astype(NP[dtype])], axis=1)
    return x, tr, np.array(LENGTHS)


@functools.lru_cache(maxsize=None)
def _prunes(dtype, N):
    """Whether THETA removes pairs that K alone would keep, from the restatement's kept sets of the full-length utterance."""
    x, tr, il = _inputs(dtype, N)
    lex, lm = C.layout_case(N)
    sizes = []
    for theta in (INF, THETA):
        info = {}
        beam_word_ref(x[:, :1], tr, lex, lm, il[:1], K, theta, *W, info=info)
        sizes.append(list(info["sizes"][0]))
    return sizes[0] != sizes[1]


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


@pytest.mark.parametrize("order", [None, 2], ids=["plain", "look-ahead"])
@pytest.mark.parametrize("dtype,N", CASES, ids=["f32-N199", "f32-N200", "f64-N141", "f64-N142"])
def test_the_four_calls_and_the_loss_run_one_search(dtype, N, order):
    A = _asg()
    e = 4 if dtype == torch.float32 else 8
    assert C.transitions_in_lds(K, N, e) == (N in (199, 141)) and (e, K, N - (N in (200, 142))) in C.LDS_STEPS
    assert _prunes(dtype, N)
    lex, lm = C.layout_case(N)
    la = None if order is None else A.WordLookahead(lex, lm, order)
    x, tr, il = (torch.from_numpy(a).to(DEV) for a in _inputs(dtype, N))
    one = A.beam_decode_words(x, tr, lex, lm, il, K, THETA, *W, lookahead=la)
    conf = A.beam_decode_words_confidence(x, tr, lex, lm, il, K, THETA, *W, TOL, lookahead=la)
    nb = A.beam_decode_words_nbest(x, tr, lex, lm, il, K, NBEST, THETA, *W, return_alignments=True, lookahead=la)
    nbc = A.beam_decode_words_nbest_confidence(x, tr, lex, lm, il, K, NBEST, THETA, *W, TOL, return_alignments=True, lookahead=la)
    Z = A.beam_words_full_score(x, tr, lex, lm, il, K, THETA, *W, lookahead=la)
    torch.cuda.synchronize()
    what = "%s N=%d order=%s" % (dtype, N, order)
    assert one._fields == conf._fields[:8]
    for n in one._fields:
        a = getattr(one, n)
        assert _bits(a) == _bits(getattr(conf, n)), (n, what)                                  # 1
        for rows in (nb, nbc):                                                                  # 2, 3
            r = getattr(rows, n)
            assert r.dtype == a.dtype and _bits(r[:, 0]) == _bits(a), (n, what)
    assert _bits(conf.normalisers) == _bits(Z) and _bits(nbc.normalisers) == _bits(Z), what    # 4
    assert _bits(nbc.word_frames[:, 0]) == _bits(conf.word_frames), what                        # 5
    # the full-length utterance has a path of words, the empty one the no-path fill
    assert float(one.scores[0]) > -INF and int(one.word_lengths[0]) >= 2 and float(one.scores[2]) == -INF
    assert int(one.token_lengths[2]) == 0 and (conf.word_frames[2] == -1).all()
