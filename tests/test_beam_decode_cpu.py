"""CPU tests of beam-pruned decoding with a token automaton: the test-side restatement (tests/beam_decode_ref.py) against the
exact reference, path scores and exhaustive enumeration; the source-side compiled graph (`TokenGraph.compile_beam_host`); the
lexicon automaton (`TokenGraph.from_lexicon`); the C ABI of asg_beam_decode_graph (sizes, argument checks) -- no kernel is
launched here."""
import ctypes
import itertools

import numpy as np
import pytest

from beam_decode_ref import beam_decode_ref
from graph_decode_ref import decode_graph_ref, path_score_graph, product, fold

NAMES = ("scores", "path", "tokens", "token_lengths", "states")


def _tg():
    from torch_asg_amd import TokenGraph
    return TokenGraph


def _ngram(N, order, seed, holes=False):
    rng = np.random.default_rng(seed)
    lp = np.log(rng.dirichlet(np.ones(N + 1), size=(N + 1,) * (order - 1))) if order > 1 else np.log(rng.dirichlet(np.ones(N + 1)))
    if holes:
        lp[rng.random(size=lp.shape) < 0.2] = -np.inf
    return _tg().from_ngram(lp)


def _random_graph(S, N, seed):
    """A random deterministic automaton whose upper states are unreachable, with missing arcs and non-accepting states."""
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, S // 2, size=(S, N))
    nxt[rng.random(size=(S, N)) < 0.3] = -1
    w = rng.normal(size=(S, N))
    f = rng.normal(size=S)
    f[rng.random(size=S) < 0.3] = -np.inf
    return _tg()(nxt, w, f, start=0)


def _case(T, B, N, seed, dtype=np.float32, integer=False):
    rng = np.random.default_rng(seed)
    if integer:
        x = rng.integers(-2, 3, size=(T, B, N)).astype(dtype)
        tr = rng.integers(-1, 2, size=(N, N)).astype(dtype)
    else:
        x = rng.normal(size=(T, B, N))
        x = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(dtype)
        tr = rng.normal(size=(N, N)).astype(dtype)
    il = rng.integers(0, T + 1, size=B)
    il[0] = T
    if B > 1:
        il[1] = 0
    if B > 2:
        il[2] = 1
    return x, tr, il


GRAPHS = {
    "unigram8": lambda: _ngram(8, 1, 1),
    "bigram8": lambda: _ngram(8, 2, 2, holes=True),
    "trigram6": lambda: _ngram(6, 3, 3, holes=True),
    "random": lambda: _random_graph(30, 12, 4),
}


def _Q(g):
    return g.compile_host(np.float32)["Q"]


def _both(g, x, tr, il, K, theta, lw=0.8, ts=-0.5, sizes=None):
    beam = beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, il, K, theta, lw, ts, sizes=sizes)
    exact = decode_graph_ref(x, tr, g.next, g.weight, g.final, g.start, il, lw, ts)
    return beam, exact


@pytest.mark.parametrize("integer", [False, True], ids=["random", "integer"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_a_full_beam_equals_the_exact_decoder(name, dtype, integer):
    g = GRAPHS[name]()
    x, tr, il = _case(25, 5, g.N, 21, dtype, integer)
    for K in (_Q(g), _Q(g) + 7):
        beam, exact = _both(g, x, tr, il, K, np.inf)
        for n, u, v in zip(NAMES, beam, exact):
            assert u.dtype == v.dtype and np.array_equal(u, v), n


@pytest.mark.parametrize("integer", [False, True], ids=["random", "integer"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_pruned_scores_are_path_scores_and_never_above_exact(name, dtype, integer):
    g = GRAPHS[name]()
    x, tr, il = _case(25, 5, g.N, 22, dtype, integer)
    for K in (1, 3, 8, max(1, _Q(g) // 4)):
        for theta in (np.inf, 4.0, 0.0):
            sizes = []
            (sc, path, tok, tl, st), exact = _both(g, x, tr, il, K, theta, sizes=sizes)
            assert all(n <= K for per in sizes for n in per)
            for b in range(x.shape[1]):
                L = int(il[b])
                assert sc[b] <= exact[0][b]
                assert (path[b, L:] == -1).all() and (st[b, L:] == -1).all()
                if not sc[b] > -np.inf:
                    assert (path[b] == -1).all() and (tok[b] == -1).all() and (st[b] == -1).all() and tl[b] == 0
                    continue
                s, sts = path_score_graph(x[:, b], tr, g.next, g.weight, g.final, path[b, :L], g.start, 0.8, -0.5)
                assert s == sc[b] and sts == list(st[b, :L])
                if np.array_equal(path[b], exact[1][b]):
                    assert sc[b] == exact[0][b]
                p = path[b, :L]
                c = [int(v) for i, v in enumerate(p) if i == 0 or p[i - 1] != v]
                assert tl[b] == len(c) and list(tok[b, :len(c)]) == c and (tok[b, len(c):] == -1).all()


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_full_beam_against_exhaustive_enumeration(seed, dtype):
    rng = np.random.default_rng(900 + seed)
    for _ in range(10):
        T, B, N, S = int(rng.integers(1, 6)), 2, int(rng.integers(2, 5)), int(rng.integers(1, 5))
        nxt = rng.integers(0, S, size=(S, N))
        nxt[rng.random(size=(S, N)) < 0.25] = -1
        w = rng.normal(size=(S, N))
        f = rng.normal(size=S)
        f[rng.random(size=S) < 0.3] = -np.inf
        x = rng.normal(size=(T, B, N)).astype(dtype)
        tr = rng.normal(size=(N, N)).astype(dtype)
        sc = beam_decode_ref(x, tr, nxt, w, f, 0, None, S * N, np.inf, 0.5, -0.3)[0]
        for b in range(B):
            best = max(path_score_graph(x[:, b], tr, nxt, w, f, p, 0, 0.5, -0.3)[0] for p in itertools.product(range(N), repeat=T))
            assert sc[b] == best


def test_threshold_zero_keeps_only_the_states_tied_with_the_best():
    g = _ngram(6, 2, 5)
    x, tr, il = _case(30, 4, 6, 23, np.float32, integer=True)
    sizes = []
    beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, None, _Q(g), 0.0, 0.0, 1.0, sizes=sizes)
    # lm_weight 0, token_score 1, integer emissions: ties happen, and every kept state has the frame's best value
    assert max(n for per in sizes for n in per) > 1
    # K = 1, theta = 0 and K = 1, theta = inf are the same greedy search
    a = beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, il, 1, 0.0)
    b = beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, il, 1, np.inf)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    # on distinct values theta = 0 is the greedy search whatever K is
    x, tr, il = _case(30, 4, 6, 24, np.float64)
    a = beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, il, 9, 0.0)
    b = beam_decode_ref(x, tr, g.next, g.weight, g.final, g.start, il, 1, np.inf)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_ties_at_the_last_rank_go_to_the_smallest_product_state():
    # all-zero scores: every candidate ties, so the K kept states are the K smallest candidate indices and the path is the
    # one the exact decoder's tie rule picks among those
    N = 5
    g = _tg().from_ngram(np.zeros((N + 1, N + 1)))
    x = np.zeros((6, 1, N), np.float32)
    tr = np.zeros((N, N), np.float32)
    sizes = []
    sc, path, tok, tl, st = beam_decode_ref(x, tr, g.next, g.weight, g.final, 0, None, 3, np.inf, sizes=sizes)
    assert sizes == [[3] * 6] and sc[0] == 0.0
    label, state, _, _, Q = product(g.next, fold(g.next, g.weight, g.final, np.float32, 1.0, 0.0)[0])
    assert path[0, 0] == label[0] and st[0, 0] == state[0]          # frame 0 keeps q = 0, 1, 2; the end takes the smallest


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_compile_beam_host_is_the_same_graph_from_the_source_side(name, dt):
    g = GRAPHS[name]()
    h = g.compile_host(dt, 0.8, -0.5)
    hb = g.compile_beam_host(dt, 0.8, -0.5)
    Q, E = h["Q"], h["E"]
    assert hb["orow"].shape == (Q + 1,) and hb["oarc"].shape == (E, 2) and hb["ow"].shape == (E,) and hb["ow"].dtype == dt
    assert hb["orow"].dtype == np.int32 and hb["oarc"].dtype == np.int32 and hb["start_q"].dtype == np.int32
    assert hb["orow"][0] == 0 and hb["orow"][-1] == E and (np.diff(hb["orow"]) >= 0).all()
    assert hb["max_out"] == int(np.diff(hb["orow"]).max(initial=0))
    osrc = np.repeat(np.arange(Q), np.diff(hb["orow"]))
    otgt = hb["oarc"][:, 0]
    assert np.array_equal(hb["oarc"][:, 1], h["label"][otgt])
    # rows ascending by target, no edge twice
    same = osrc[1:] == osrc[:-1]
    assert (otgt[1:][same] > otgt[:-1][same]).all()
    # the same multiset of (source, target, weight) as the incoming CSR
    tgt = np.repeat(np.arange(Q), np.diff(h["row"]))
    o = np.lexsort((tgt, h["src"]))
    assert np.array_equal(h["src"][o], osrc) and np.array_equal(tgt[o], otgt) and np.array_equal(h["edge_w"][o], hb["ow"])
    assert np.array_equal(hb["start_q"], np.nonzero(h["start_w"] > -np.inf)[0]) and hb["num_start"] == hb["start_q"].size
    # compile_host itself is untouched by the beam compile
    h2 = g.compile_host(dt, 0.8, -0.5)
    assert all(np.array_equal(h[k], h2[k]) for k in h)


def test_from_lexicon_numbering_scores_and_transcripts():
    TG = _tg()
    N, sep = 6, 5
    words = [[0, 1], [0, 1, 2], [3], [0, 2], [0, 1]]
    g = TG.from_lexicon(words, N, sep, word_scores=[-1.0, -2.0, -3.0, -4.0, -0.5])
    # nodes in order of first creation: 0 root, 1 = (0), 2 = (0,1), 3 = (0,1,2), 4 = (3), 5 = (0,2)
    assert g.S == 6 and g.start == 0
    assert g.next[0, 0] == 1 and g.next[1, 1] == 2 and g.next[2, 2] == 3 and g.next[0, 3] == 4 and g.next[1, 2] == 5
    assert g.weight[0, 0] == 0 and g.weight[1, 1] == 0 and g.weight[1, 2] == 0
    assert g.next[0, sep] == -1 and g.next[1, sep] == -1                       # the root and an inner node: no separator arc
    assert g.next[2, sep] == 0 and g.weight[2, sep] == -0.5 and g.final[2] == -0.5   # the larger score of the double
    assert g.next[3, sep] == 0 and g.weight[3, sep] == -2.0 and g.final[3] == -2.0
    assert g.final[0] == 0.0 and g.final[1] == -np.inf and g.final[4] == -3.0 and g.final[5] == -4.0
    assert (g.next >= 0).sum() == 5 + 4                                       # five trie arcs, four word ends
    x = np.zeros((8, N))
    tr = np.zeros((N, N))

    def score(labels):
        return path_score_graph(x[:len(labels)], tr, g.next, g.weight, g.final, labels, 0)[0]
    assert score([0, 1]) == -0.5                                   # "01" ending at its word end
    assert score([0, 0, 1, 1, sep]) == -0.5                        # ... or at the root behind the separator
    assert score([0, 1, sep, 3]) == -0.5 + -3.0
    assert score([0, 1, 2, sep, 0, 2, sep]) == -2.0 + -4.0
    assert score([0]) == -np.inf                                   # inside a word: not accepting
    assert score([1]) == -np.inf and score([sep]) == -np.inf       # no such word; the root has no separator arc
    assert score([0, 1, 3]) == -np.inf                             # words need the separator between them
    g0 = TG.from_lexicon(words[:4], N, sep)
    assert g0.weight[2, sep] == 0.0 and g0.final[5] == 0.0


def test_from_lexicon_rejects_bad_spellings():
    TG = _tg()
    with pytest.raises(ValueError):
        TG.from_lexicon([[0, 0, 1]], 4, 3)                          # a repeated token
    with pytest.raises(ValueError):
        TG.from_lexicon([[0, 3]], 4, 3)                             # the separator inside a word
    with pytest.raises(ValueError):
        TG.from_lexicon([[]], 4, 3)
    with pytest.raises(ValueError):
        TG.from_lexicon([[0, 4]], 4, 3)
    with pytest.raises(ValueError):
        TG.from_lexicon([[0]], 4, 4)
    with pytest.raises(ValueError):
        TG.from_lexicon([[0], [1]], 4, 3, word_scores=[0.0])


def test_a_lexicon_decodes_only_lexicon_words():
    rng = np.random.default_rng(31)
    N, sep = 8, 7
    words = []
    while len(words) < 40:
        w = rng.integers(0, sep, size=int(rng.integers(1, 5))).tolist()
        if all(a != b for a, b in zip(w, w[1:])):
            words.append(w)
    g = _tg().from_lexicon(words, N, sep, rng.normal(size=len(words)))
    x, tr, il = _case(30, 4, N, 32, np.float32)
    vocab = {tuple(w) for w in words}
    for K in (4, 16, _Q(g)):
        sc, path, tok, tl, st = beam_decode_ref(x, tr, g.next, g.weight, g.final, 0, il, K, np.inf, 1.0, 0.0)
        for b in range(4):
            if not sc[b] > -np.inf:
                continue
            t = tok[b, :tl[b]].tolist()
            cur, out = [], []
            for v in t:
                if v == sep:
                    out.append(tuple(cur))
                    cur = []
                else:
                    cur.append(v)
            if cur:
                out.append(tuple(cur))
            assert out and all(w in vocab for w in out)


def test_abi_sizes_and_argument_checks():
    from torch_asg_amd import _lib
    L = _lib.lib()
    p = _lib.AsgProblem()
    p.T, p.B, p.N, p.dtype = 400, 64, 40, _lib.ASG_DTYPE_F32
    p.inputs = p.transition = 256                                    # never dereferenced here
    g = _lib.AsgTokenGraph()
    g.Q, g.E, g.N, g.dtype = 65640, 2559960, 40, _lib.ASG_DTYPE_F32
    for n in ("label", "state", "row", "src", "src_label", "start_w", "final_w", "edge_w"):
        setattr(g, n, 256)
    gb = _lib.AsgTokenGraphBeam()
    gb.graph = ctypes.pointer(g)
    gb.num_start, gb.max_out = 40, 39
    for n in ("orow", "oarc", "ow", "start_q"):
        setattr(gb, n, 256)
    wb = lambda K: int(L.asg_beam_decode_graph_work_bytes(ctypes.byref(p), ctypes.byref(gb), K))
    exact = int(L.asg_viterbi_decode_graph_work_bytes(ctypes.byref(p), ctypes.byref(g)))

    def want(K, e=4):
        a = lambda v: (v + 255) // 256 * 256
        cap = max(min(g.Q, K * 40), 40)
        return 64 * (2 * a(400 * K * 4) + a(g.Q * 8) + a(g.Q * e) + a(cap * e) + a(cap * 4))
    for K in (1, 64, 256, 1024, 4096, 8192):
        assert wb(K) == want(K)
    assert wb(256) < exact // 40                                     # T*B*K, not T*B*Q
    assert wb(0) == 0 and wb(-3) == 0
    assert wb(8193) == 0                                             # above the limit (and below Q): unsupported
    g.Q = 100
    assert wb(1 << 30) == wb(100) > 0                                # a beam above Q is Q
    g.Q = 65640
    args = (None, None, None, None, None, 0, None)
    call = lambda K, th, work=256, nbytes=1 << 40: L.asg_beam_decode_graph(None, ctypes.byref(p), ctypes.byref(gb), K, th, work,
                                                                           nbytes, *args)
    assert call(0, 1.0) == 1 and call(8, -1.0) == 1 and call(8, float("nan")) == 1
    assert call(8193, 1.0) == 2                                      # ASG_ERR_UNSUPPORTED
    assert call(8, 1.0) == 1                                         # null outputs
    out = (256, 256, 256, 256, 256, 0, None)
    assert L.asg_beam_decode_graph(None, ctypes.byref(p), ctypes.byref(gb), 8, 1.0, 256, 16, *out) == 3   # workspace too small
    g.dtype = _lib.ASG_DTYPE_F64
    assert wb(8) == 0                                                # the graph's dtype is not the problem's
    p.dtype = _lib.ASG_DTYPE_F64
    assert wb(64) == want(64, 8)


def test_public_argument_errors_come_before_any_device_work():
    import torch
    import torch_asg_amd as A
    g = _ngram(5, 2, 10)
    x, tr = torch.zeros(4, 2, 5), torch.zeros(5, 5)
    for kw in (dict(beam_size=0), dict(beam_size=-2), dict(beam_size=4, beam_threshold=-0.5),
               dict(beam_size=4, beam_threshold=float("nan"))):
        with pytest.raises(ValueError):
            A.beam_decode_graph(x, tr, g, **kw)
    with pytest.raises(ValueError):
        A.ASGLoss(5).beam_decode_graph(x, g, beam_size=0)
