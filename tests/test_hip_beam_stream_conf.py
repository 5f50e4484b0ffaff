"""GPU tests (-m gpu) of the lattice-keeping beam stream (`torch_asg_amd.BeamStream(..., keep_lattice=True)`;
csrc/asg_beam_stream_conf.hip).  `result_confidence(final=True)` is held BIT FOR BIT to the device's own
`beam_decode_graph_confidence` on the whole utterance, for every chunking and every placement of confidence calls; the prefix
results are held to the numpy restatement tests/beam_stream_conf_ref.py under tests/test_hip_beam_conf.py's rule (float64 rtol =
atol = 1e-9, float32 util.assert_close, frames and padding exact); `result` and `result_nbest` are byte-equal to a plain
`BeamStream` fed the same chunks.  Every case first asserts from the restatement that its input is in the regime it names."""
import numpy as np
import pytest
import torch

from beam_conf_ref import beam_conf_ref, window_confidences
from beam_loss_cases import DEV, GRAPHS, INF, _asg, _lexicon, _ngram
from beam_stream_conf_ref import BeamStreamConfRef
from beam_stream_ref import BeamStreamRef
from util import assert_close

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
NAMES = ["unigram", "trigram_holes", "random", "lexicon"]
W = (0.8, 0.2)                                                             # lm_weight, token_score
WF = (0.1, -0.5)                                                           # ... of the long cases: a frame adds about nothing to Z
WIDE = ("path", "tokens", "states", "token_frames")
TEN = ("scores", "path", "tokens", "token_lengths", "states", "token_frames", "token_confidences", "normalisers", "frames", "status")


def _np(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def _case(T, B, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g, dtype=torch.float64), -1).to(dtype)
    tr = (0.5 * torch.randn(N, N, generator=g, dtype=torch.float64)).to(dtype)
    return x, tr


def _flat_case(T, B, N, seed, dtype):
    """tests/test_hip_beam_conf.py's long case: the best label of every frame is 0 and the stay is expensive, so the running sums
    stay small (float32 keeps the 1e-4 rule over hundreds of frames) and the winner changes its label at nearly every frame."""
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g, dtype=torch.float64), -1)
    x = x - x.max(-1, keepdim=True).values
    tr = 0.1 * torch.randn(N, N, generator=g, dtype=torch.float64) - 3.0 * torch.eye(N, dtype=torch.float64)
    return x.to(dtype), tr.to(dtype)


def _stream(graph, tr, B, M, K, th=INF, w=W, keep=True):
    return _asg().BeamStream(tr.to(DEV), graph, B, M, K, th, *w, dtype=tr.dtype, device=DEV, keep_lattice=keep)


def _ref(graph, tr, B, M, K, th=INF, w=W):
    return BeamStreamConfRef(tr.numpy(), graph.next, graph.weight, graph.final, graph.start, B, M, K, th, *w, dtype=_np(tr.dtype))


def _chunks(x, lens, cuts):
    """x [T,B,N] with lengths lens in chunks of `cuts` frames -> [(chunk, chunk_lengths)]."""
    out, a = [], 0
    for n in cuts:
        out.append((x[a:a + n], torch.clamp(lens - a, 0, n)))
        a += n
    return out


def _split(x, lens, seed):
    """Two chunks of Tc = ceil(T / 2) frames in which slot b takes its first s_b frames from the first and the rest from the second:
    per-slot lengths inside one Tc."""
    T, B, N = x.shape
    Tc = (T + 1) // 2
    g = torch.Generator().manual_seed(seed)
    sp = torch.tensor([int(torch.randint(max(0, int(l) - Tc), min(int(l), Tc) + 1, (1,), generator=g)) for l in lens])
    c1, c2 = torch.zeros_like(x[:Tc]), torch.zeros_like(x[:Tc])
    for b in range(B):
        s, l = int(sp[b]), int(lens[b])
        c1[:s, b] = x[:s, b]
        c2[:l - s, b] = x[s:l, b]
    return [(c1, sp), (c2, lens - sp)]


def _feed(s, chunks, after=None):
    for i, (c, cl) in enumerate(chunks):
        s.advance(c.to(DEV), cl.to(DEV))
        if after is not None:
            after(i)


def _bits(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in ts]


def _host(r):
    torch.cuda.synchronize()
    return {n: getattr(r, n).cpu().numpy() for n in r._fields}


def _equal_one_shot(got, one, T, what):
    """A stream result [B, M] against the device's one-shot result [B, T]: bits on the one-shot's columns, padding beyond."""
    g, o = _host(got), _host(one)
    for n in ("scores", "normalisers", "token_lengths"):
        assert g[n].dtype == o[n].dtype and g[n].tobytes() == o[n].tobytes(), (what, n)
    for n in WIDE:
        assert np.array_equal(g[n][:, :T], o[n]) and (g[n][:, T:] == -1).all(), (what, n)
    assert np.ascontiguousarray(g["token_confidences"][:, :T]).tobytes() == o["token_confidences"].tobytes(), what
    assert (g["token_confidences"][:, T:] == 0).all(), what


def _close(got, want, dtype, what):
    assert not np.isnan(got).any(), what
    if dtype == torch.float64:
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9), what
    else:
        assert_close(got, want, what=what)


def _equal_ref(got, want, dtype, what):
    """A stream result against the restatement's: integers, frames and padding exact, the real fields under the rule."""
    g = _host(got)
    for n in WIDE + ("token_lengths", "frames", "status"):
        assert np.array_equal(g[n], want[n]), (what, n)
    behind = np.arange(g["path"].shape[1])[None, :] >= want["token_lengths"][:, None]
    assert (g["token_confidences"][behind] == 0).all(), what
    _close(g["token_confidences"], want["token_confidences"], dtype, what)
    for n in ("scores", "normalisers"):
        fin = np.isfinite(want[n])
        assert np.array_equal(np.isfinite(g[n]), fin) and (g[n][~fin] == -np.inf).all(), (what, n)
        _close(g[n][fin], want[n][fin].astype(np.float64), dtype, "%s %s" % (what, n))


def _one_shot(x, tr, graph, lens, K, th, tol, w=W):
    return _asg().beam_decode_graph_confidence(x.to(DEV), tr.to(DEV), graph, lens.to(DEV), K, th, *w, tol)


# ---------------------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_final_is_the_one_shot_call_bit_for_bit_for_every_chunking_and_placement(name, dtype):
    graph = GRAPHS[name]()
    Q = graph.compile_host(np.float32)["Q"]
    T, B, M = 24, 5, 26
    x, tr = _case(T, B, graph.N, 31, dtype)
    lens = torch.tensor([T, 0, 1, 17, 9])
    want = beam_conf_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start, lens.numpy(), 3, INF, *W, 0)
    assert any(s == 3 for s in want["sizes"][0]) and 3 < Q                 # the beam of 3 prunes
    c = want["token_confidences"][0, :int(want["token_lengths"][0])]
    assert np.isfinite(want["normalisers"][[0, 2, 3, 4]]).all() and want["normalisers"][1] == -np.inf
    doubtful = bool(((c > 0.01) & (c < 0.99)).any())
    tols = (0, 1, 3, 64)
    chunkings = [_chunks(x, lens, [1] * T), _chunks(x, lens, [T]), _chunks(x, lens, [1, 7, 0, 16]), _split(x, lens, 5)]
    for K in (1, 3, 8, Q):
        for th in (INF, 2.0):
            one = {tol: _one_shot(x, tr, graph, lens, K, th, tol) for tol in tols}
            for ci, chunks in enumerate(chunkings):
                what = (name, K, th, ci)
                s = _stream(graph, tr, B, M, K, th)                        # result_confidence only at the end
                _feed(s, chunks)
                for tol in tols:
                    _equal_one_shot(s.result_confidence(tol, final=True), one[tol], T, what + (tol, "end"))
                s = _stream(graph, tr, B, M, K, th)                        # ... and after every chunk, both modes, every tolerance
                _feed(s, chunks, lambda i: s.result_confidence(tols[i % 4], final=bool(i % 2)))
                for tol in tols:
                    _equal_one_shot(s.result_confidence(tol, final=True), one[tol], T, what + (tol, "every"))
    assert doubtful or name == "unigram"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_prefix_results_after_every_chunk_and_the_plain_results_of_the_stream(name, dtype):
    graph = GRAPHS[name]()
    T, B, M = 12, 4, 13
    x, tr = _case(T, B, graph.N, 33, dtype)
    lens = torch.tensor([T, 0, 1, 7])
    for K, th in ((3, INF), (8, 2.0)):
        chunks = _chunks(x, lens, [1, 4, 0, 7])
        s, plain, ref = _stream(graph, tr, B, M, K, th), _stream(graph, tr, B, M, K, th, keep=False), _ref(graph, tr, B, M, K, th)
        pruned = 0
        for i, (c, cl) in enumerate(chunks):
            s.advance(c.to(DEV), cl.to(DEV))
            plain.advance(c.to(DEV), cl.to(DEV))
            ref.advance(c.numpy(), cl.numpy())
            for tol in (0, 2):
                want = ref.result_confidence(tol, final=False)
                _equal_ref(s.result_confidence(tol, final=False), want, dtype, (name, K, th, i, tol))
            pruned += any(z == K for z in ref.sizes()[0])
            for final in (False, True):                                    # result and result_nbest: a plain stream's bytes
                assert _bits(s.result(final)) == _bits(plain.result(final))
                a, b = s.result_nbest(3, final, True), plain.result_nbest(3, final, True)
                assert _bits(a) == _bits(b)
        assert pruned
        s.reset()
        plain.reset()
        assert _bits(s.result()) == _bits(plain.result())


# ---------------------------------------------------------------------------------------------------------------- the shapes
def _both_modes(graph, x, tr, lens, K, M, cuts, tols, w=W, what="", calls=()):
    """One stream over `cuts`, confidence calls after the chunks in `calls`: final against the one-shot call's bits and, with the
    prefix, against the restatement."""
    dtype, T, B = x.dtype, x.shape[0], x.shape[1]
    s, ref = _stream(graph, tr, B, M, K, INF, w), _ref(graph, tr, B, M, K, INF, w)
    for i, (c, cl) in enumerate(_chunks(x, lens, cuts)):
        s.advance(c.to(DEV), cl.to(DEV))
        ref.advance(c.numpy(), cl.numpy())
        if i in calls:
            s.result_confidence(tols[0], final=False)
    for tol in tols:
        got = s.result_confidence(tol, final=True)
        _equal_one_shot(got, _one_shot(x, tr, graph, lens, K, INF, tol, w), T, (what, tol))
        _equal_ref(got, ref.result_confidence(tol, final=True), dtype, (what, tol, "final"))
        _equal_ref(s.result_confidence(tol, final=False), ref.result_confidence(tol, final=False), dtype, (what, tol, "prefix"))
    return ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [32, 33, 63, 64, 65])
def test_kept_sets_around_the_subgroup_steps(K, dtype):
    graph = _ngram(70, 1, 11)
    x, tr = _case(6, 2, 70, 12, dtype)
    ref = _both_modes(graph, x, tr, torch.tensor([6, 4]), K, 6, [2, 4], (0, 2), what="subgroup", calls=(0,))
    assert all(z == K for b in range(2) for z in ref.sizes()[b])           # every kept set has exactly K states


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_trie_root_with_a_beam_below_its_degree(dtype):
    graph = _lexicon(12, 300, 9, maxlen=3)
    h, hb = graph.compile_host(np.float64), graph.compile_beam_host(np.float64)
    assert int(np.diff(h["row"]).max()) > 64 and int(hb["max_out"]) >= 11
    x, tr = _case(12, 3, 12, 4, dtype)
    for K in (8, 32):
        ref = _both_modes(graph, x, tr, torch.tensor([12, 7, 1]), K, 12, [5, 7], (0, 2), what="trie", calls=(0,))
        assert max(ref.sizes()[0]) == K < int(hb["max_out"]) * 3
        assert (ref.result(True)[2][0] == 0).any()                         # a separator: a word boundary


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_utterances_around_a_wavefront_with_a_full_window(dtype):
    graph = _ngram(10, 1, 1)
    x, tr = _flat_case(130, 4, 10, 15, dtype)
    ref = _both_modes(graph, x, tr, torch.tensor([63, 64, 65, 129]), 6, 130, [40, 90], (0, 64), WF, "M=130", calls=(0,))
    r = ref.result_confidence(64, final=True)
    f = r["token_frames"][3, :int(r["token_lengths"][3])]
    assert max(int(((f >= v - 64) & (f <= v + 64)).sum()) for v in f) >= 20                  # tokens inside one window
    assert all(int(r["token_lengths"][b]) > 32 for b in range(4)) and np.abs(r["normalisers"]).max() < 32


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_ring_wraps_behind_token_256(dtype):
    graph = _ngram(10, 1, 1)
    x, tr = _flat_case(300, 2, 10, 16, dtype)
    ref = _both_modes(graph, x, tr, torch.tensor([300, 280]), 4, 300, [100, 200], (0, 64), WF, "M=300")
    r = ref.result_confidence(0, final=True)
    assert np.abs(r["normalisers"]).max() < 32                             # the running sums did stay small
    assert int(r["token_lengths"][0]) > 257 and int(r["token_lengths"][1]) > 257             # a token index above 256


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_catch_up_that_starts_at_frame_0_at_frame_1_and_at_the_last_frame(dtype):
    graph = GRAPHS["bigram"]()
    T, B = 9, 3
    x, tr = _case(T, B, graph.N, 35, dtype)
    lens = torch.tensor([T, T, 6])
    one = _one_shot(x, tr, graph, lens, 6, 4.0, 1)
    ref = _ref(graph, tr, B, T, 6, 4.0)
    ref.advance(x.numpy(), lens.numpy())
    assert any(z == 6 for z in ref.sizes()[0])
    for calls in ((), (0,), (0, 1), (1,)):          # ranges [0, 9); [0, 1) [1, 9); [0, 1) [1, 8) [8, 9); [0, 8) [8, 9)
        s = _stream(graph, tr, B, T, 6, 4.0)
        _feed(s, _chunks(x, lens, [1, T - 2, 1]), lambda i: s.result_confidence(0, final=True) if i in calls else None)
        _equal_one_shot(s.result_confidence(1, final=True), one, T, calls)
        _equal_one_shot(s.result_confidence(1, final=True), one, T, calls)                    # caught up: nothing to do


# ---------------------------------------------------------------------------------------------------------------- the stream
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_beam_that_empties_inside_a_chunk_on_its_first_and_on_its_last_frame(dtype):
    A = _asg()
    ok = A.TokenGraph(np.zeros((1, 5), np.int64), np.zeros((1, 5)), np.zeros(1))
    x, tr = _case(8, 3, 5, 18, dtype)
    lens = torch.tensor([8, 8, 3])
    x[4:, 0] = -INF                                                        # slot 0: every candidate of frame 4 is -inf
    ref = _ref(ok, tr, 3, 8, 3)
    ref.advance(x.numpy(), lens.numpy())
    assert ref.sizes()[0][3] == 3 and ref.sizes()[0][4:] == [0, 0, 0, 0]
    one = _one_shot(x, tr, ok, lens, 3, INF, 2)
    for cuts in ([8], [2, 6], [4, 4], [5, 3]):                             # frame 4: inside, inside, first, last of its chunk
        s = _stream(ok, tr, 3, 8, 3)
        _feed(s, _chunks(x, lens, cuts), lambda i: s.result_confidence(2, final=False))
        got = s.result_confidence(2, final=True)
        _equal_one_shot(got, one, 8, cuts)
        _equal_ref(got, ref.result_confidence(2, final=True), dtype, cuts)
        pre = s.result_confidence(2, final=False)
        assert pre.scores[0].item() == -INF and pre.normalisers[0].item() == -INF and pre.token_lengths[0].item() == 0
        assert (pre.token_frames[0] == -1).all() and (pre.token_confidences[0] == 0).all()
        assert not torch.isnan(pre.token_confidences).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_plain_stream_and_the_lattice_keeping_one_run_one_advance(dtype):
    """The two states are advanced by ONE kernel text (csrc/asg_beam_stream.hip, with and without the keep policy): for the same
    chunks `result(final=False)`, `result(final=True)` and `result_nbest(2)` are the same bytes, at the smallest shape that
    reaches every branch of the shared loop.  B = 3, N = 4, max_frames = 6, beam_size = 3 < Q = 4, a finite threshold; chunks of
    1, 2 and 4 frames with per-slot lengths (1, 1, 1), (2, 2, 1), (4, 4, 2).  Checked with tests/beam_stream_ref.py, and asserted
    below from it: slots 0 and 1 are offered 7 > 6 frames, take 3 of the last chunk's 4 and set `status`; slot 2 takes 4 frames
    and does not; slot 1, whose emissions are -inf from frame 2 on, keeps 3, 3, 0, 0, 0, 0 states -- its beam empties on the
    second frame of the second chunk and skips the third chunk from its first frame, the only slot whose beam empties --, and
    slots 0 and 2 keep 3 states in every frame and have finite scores after every chunk."""
    N, B, M, K, th = 4, 3, 6, 3, 4.0
    graph = _asg().TokenGraph(np.zeros((1, N), np.int64), np.zeros((1, N)), np.zeros(1))
    x, tr = _case(7, B, N, 41, dtype)
    x[2:, 1] = -INF
    chunks = [(x[0:1], torch.tensor([1, 1, 1])), (x[1:3], torch.tensor([2, 2, 1])), (x[3:7], torch.tensor([4, 4, 2]))]
    ref = BeamStreamRef(tr.numpy(), graph.next, graph.weight, graph.final, graph.start, B, M, K, th, *W, dtype=_np(dtype))
    s, plain = _stream(graph, tr, B, M, K, th), _stream(graph, tr, B, M, K, th, keep=False)
    for i, (c, cl) in enumerate(chunks):
        ref.advance(c.numpy(), cl.numpy())
        for st in (s, plain):
            st._fed = 0                                    # (the host's bound counts offered frames; the device's clamp is the subject)
            st.advance(c.to(DEV), cl.to(DEV))
        finite = np.isfinite(ref.result(False)[0])
        assert finite.tolist() == [True, i < 1, True]
        for final in (False, True):
            a, b = s.result(final), plain.result(final)
            assert _bits(a) == _bits(b), (i, final)
            assert torch.isfinite(a.scores).cpu().numpy().tolist() == np.isfinite(ref.result(final)[0]).tolist()
            assert _bits(s.result_nbest(2, final, True)) == _bits(plain.result_nbest(2, final, True)), (i, final)
    assert ref.sizes() == [[3] * 6, [3, 3, 0, 0, 0, 0], [3] * 4]
    got = s.result()
    assert got.frames.tolist() == [6, 6, 4] == ref.result()[5].tolist() and got.status.tolist() == [1, 1, 0] == ref.result()[6].tolist()
    conf = s.result_confidence(1, final=False)             # (the catch-up reads the kept counts of the skipped frames: 0)
    assert conf.normalisers[1].item() == -INF and torch.isfinite(conf.normalisers[[0, 2]]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_masked_reset_in_mid_stream(dtype):
    graph = GRAPHS["random"]()
    x, tr = _case(8, 3, graph.N, 37, dtype)
    full = torch.tensor([8, 8, 8])
    s = _stream(graph, tr, 3, 8, 4)
    s.advance(x[:3].to(DEV))
    s.result_confidence(0)
    s.advance(x[3:5].to(DEV))
    s.reset(torch.tensor([0, 1, 0]))
    s.advance(x[5:8].to(DEV))
    got = _host(s.result_confidence(1, final=True))
    whole = _host(_one_shot(x, tr, graph, full, 4, INF, 1))
    tail = _host(_one_shot(x[5:8], tr, graph, torch.tensor([3, 3, 3]), 4, INF, 1))
    assert list(got["frames"]) == [8, 3, 8]
    for b, (o, T) in enumerate([(whole, 8), (tail, 3), (whole, 8)]):
        for n in ("scores", "normalisers", "token_lengths"):
            assert got[n][b].tobytes() == o[n][b].tobytes(), (b, n)
        for n in WIDE:
            assert np.array_equal(got[n][b, :T], o[n][b]) and (got[n][b, T:] == -1).all(), (b, n)
        assert got["token_confidences"][b, :T].tobytes() == o["token_confidences"][b].tobytes()
        assert (got["token_confidences"][b, T:] == 0).all()


def test_capture_with_three_replays_that_reach_and_pass_max_frames():
    graph = GRAPHS["trigram_holes"]()
    Tc, B, N, M = 3, 3, graph.N, 8
    _, tr = _case(Tc, B, N, 23, torch.float32)
    s, twin = _stream(graph, tr, B, M, 6, 3.0), _stream(graph, tr, B, M, 6, 3.0)
    x = torch.zeros(Tc, B, N, device=DEV)
    cl = torch.full((B,), Tc, dtype=torch.int64, device=DEV)

    def step(st):
        st.advance(x, cl)
        return st.result_confidence(1, final=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(s)                                            # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    s.reset()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = step(s)
    lengths = ([3, 3, 1], [3, 3, 0], [3, 2, 2])            # slot 0 is offered 9 > 8 frames, slot 1 reaches 8 exactly
    for k, seed in enumerate((1, 2, 3)):
        gen = torch.Generator().manual_seed(seed)
        x.copy_(torch.log_softmax(torch.randn(Tc, B, N, generator=gen), -1))
        cl.copy_(torch.tensor(lengths[k]))
        gr.replay()
        twin._fed = 0                                      # (the host's bound counts offered frames; the replays pass it by design)
        assert _bits(out) == _bits(step(twin)), k
    torch.cuda.synchronize()
    assert out.frames.tolist() == [8, 8, 3] and out.status.tolist() == [1, 0, 0]
    assert torch.isfinite(out.normalisers).all() and not torch.isnan(out.token_confidences).any()
    fin = s.result_confidence(1, final=True)
    assert _bits(fin) == _bits(twin.result_confidence(1, final=True)) and fin.status.tolist() == [1, 0, 0]


def test_two_runs_give_identical_bits():
    graph = GRAPHS["bigram"]()
    x, tr = _case(12, 4, graph.N, 22, torch.float32)
    lens = torch.tensor([12, 3, 0, 11])

    def run():
        s = _stream(graph, tr, 4, 12, 24, 6.0)
        outs = []
        _feed(s, _chunks(x, lens, [5, 0, 7]), lambda i: outs.extend(_bits(s.result_confidence(2, final=bool(i % 2)))))
        return outs + _bits(s.result_confidence(2, final=True))
    a = run()
    assert a == run() == run()


def test_the_neighbours_are_unchanged_after_the_calls():
    A = _asg()
    graph = GRAPHS["random"]()
    x, tr = _case(9, 4, graph.N, 24, torch.float32)
    il = torch.tensor([9, 0, 1, 6])
    g = torch.Generator().manual_seed(3)
    tg, tl = torch.randint(0, graph.N, (4, 3), generator=g), torch.tensor([3, 0, 1, 2])
    xd, trd, ild, tgd, tld = x.to(DEV), tr.to(DEV), il.to(DEV), tg.to(DEV), tl.to(DEV)

    def others():
        out = list(A.beam_decode_graph(xd, trd, graph, ild, 6, 4.0, *W))
        out += list(A.beam_decode_graph_confidence(xd, trd, graph, ild, 6, 4.0, *W, 2))
        p = _stream(graph, tr, 4, 9, 6, 4.0, keep=False)
        p.advance(xd[:4], torch.clamp(ild, 0, 4))
        out += list(p.result())
        p.advance(xd[4:], torch.clamp(ild - 4, 0, 5))
        out += list(p.result(final=True)) + [o for o in p.result_nbest(3, True) if o is not None]
        xg, tg_ = xd.clone().requires_grad_(True), trd.clone().requires_grad_(True)
        loss = A.beam_graph_asg_loss(xg, tgd, tg_, graph, ild, tld, 6, 4.0, *W)
        loss[torch.isfinite(loss)].sum().backward()
        out += [loss.detach(), xg.grad, tg_.grad]
        return [o.cpu() for o in out]
    before = others()
    s = A.ASGLoss(graph.N).to(DEV).beam_stream(graph, 4, 9, 6, 4.0, *W, keep_lattice=True)
    s.advance(xd, ild)
    s.result_confidence(3)
    s.result_confidence(0, final=True)
    for u, v in zip(before, others()):
        assert torch.equal(u, v)
    for bad in (65, 1 << 40):
        with pytest.raises(RuntimeError, match="asg_beam_conf_stream_confidence"):
            s.result_confidence(bad)
    with pytest.raises(ValueError):
        s.result_confidence(-1)
    with pytest.raises(RuntimeError, match="keep_lattice"):
        _stream(graph, tr, 4, 9, 6, keep=False).result_confidence()
