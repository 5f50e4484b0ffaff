"""GPU tests (-m gpu) of streaming beam decoding with a lexicon and a word LM (`torch_asg_amd.BeamWordStream`,
csrc/asg_beam_word_stream.hip): the bytes of all ten outputs against the test-side restatement with explicit carried state
(tests/beam_word_stream_ref.py, held to the one-shot restatement on the CPU by tests/test_beam_word_stream_cpu.py).  Every case
first asserts, from the restatement's own sets, that its input is in the regime it names: two histories on one product state, an
LM walk on the first frame of a chunk, ties cut at the K-th value and decided by source-pair order, more candidates and kept
pairs than the workgroup has threads, the largest beam, every kind of end, both transition layouts, a beam that empties, the
64-frame blocks of the collapse, the clamp at max_frames; then masked reset, capture, determinism, the device's own decoders and
errors."""
import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, integers, small_lexicon
from beam_word_ref import beam_word_ref
from beam_word_stream_ref import NAMES, BeamWordStreamRef

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
ONE = NAMES[:8]
ALL = 1024                                                 # more than every pair of the small cases
LW, WS, TS = 0.7, -0.4, 0.3
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
NP = {torch.float32: np.float32, torch.float64: np.float64}


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _res(s, final=True):
    out = s.result(final)
    torch.cuda.synchronize()
    assert out._fields == NAMES
    assert out.scores.dtype == s.dtype and all(o.dtype == torch.int64 for o in out[1:])
    assert all(tuple(out[i].shape) == (s.batch_size, s.max_frames) for i in (1, 2, 4, 5, 6))
    return {n: o.cpu().numpy() for n, o in zip(NAMES, out)}


def _same(got, want, what, names=NAMES):
    for n in names:
        assert got[n].dtype == want[n].dtype and got[n].tobytes() == want[n].tobytes(), "%s %s" % (n, what)


def _same_as_one_shot(res, one, T, what):
    """res: a stream result over max_frames >= T columns; one: a one-shot decode over T columns (a dict).  Bytes."""
    for n in ("scores", "token_lengths", "word_lengths"):
        assert res[n].tobytes() == one[n].tobytes(), (n, what)
    for n in ("path", "tokens", "states", "lm_states", "words"):
        assert np.array_equal(res[n][:, :T], one[n]) and (res[n][:, T:] == -1).all(), (n, what)


class Both:
    """The device stream and the restatement, driven by the same calls."""

    def __init__(self, tr, lex, lm, B, M, K, theta=INF, lw=LW, ws=WS, ts=TS):
        self.dev = _asg().BeamWordStream(tr.to(DEV), lex, lm, B, M, K, theta, lw, ws, ts, tr.dtype, DEV)
        self.ref = BeamWordStreamRef(tr.numpy(), lex, lm, B, M, K, theta, lw, ws, ts, NP[tr.dtype])

    def advance(self, x, lengths=None):
        self.dev.advance(x.to(DEV), None if lengths is None else lengths.to(DEV))
        self.ref.advance(x.numpy(), None if lengths is None else lengths.numpy(), beam_threshold=self.dev.beam_threshold)

    def feed(self, x, il, cuts, check=None):
        """The chunks x[t0:t1] for consecutive cuts; slot b takes the frames below il[b]."""
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            self.advance(x[t0:t1], (il - t0).clamp(0, t1 - t0))
            if check:
                self.check("%s after frame %d" % (check, t1), finals=(False,))

    def reset(self, mask=None):
        self.dev.reset(None if mask is None else mask.to(DEV))
        self.ref.reset(None if mask is None else mask.numpy())

    def check(self, what, finals=(False, True)):
        out = {}
        for final in finals:
            out[final] = _res(self.dev, final)
            _same(out[final], self.ref.result(final), "%s final=%s" % (what, final))
        return out


def _normal(T, B, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, B, N, generator=g, dtype=torch.float64).to(dtype), torch.randn(N, N, generator=g, dtype=torch.float64).to(dtype)


def _gpu_one_shot(x, tr, lex, lm, il, K, theta=INF, lw=LW, ws=WS, ts=TS):
    out = _asg().beam_decode_words(x.to(DEV), tr.to(DEV), lex, lm, None if il is None else il.to(DEV), K, theta, lw, ws, ts)
    torch.cuda.synchronize()
    return {n: o.cpu().numpy() for n, o in zip(ONE, out)}


# ---------------------------------------------------------------------------------------------------------------- 1. chunks
def grid_case(order, dtype, T=12):
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, order, 60 + order, keep=(1.0, 0.5, 0.5))
    x, tr = _normal(T, 4, 5, 31, dtype)
    for t, lab in enumerate([0, 4, 1, 0, 4, 2, 4, 0, 1, 2, 4, 0][:T]):     # slot 0 spells words: its path crosses separators
        x[t, 0, lab] += 4.0
    return lex, lm, x, tr, torch.tensor([T, 5, 1, 0])


@DTYPES
@pytest.mark.parametrize("order", [2, 3], ids=["bigram", "trigram"])
def test_any_chunking_gives_the_restatements_bytes(order, dtype):
    lex, lm, x, tr, il = grid_case(order, dtype)
    T, B, sep = 12, 4, 4
    shared = 0
    for K in (1, 3, 8, ALL):
        for theta in (INF, 2.0, 0.0):
            ends = []
            for name, cuts in (("ones", list(range(T + 1))), ("whole", [0, T]), ("mixed", [0, 1, 5, 5, 12])):
                s = Both(tr, lex, lm, B, T, K, theta)
                s.feed(x, il, cuts, check="%s K=%d theta=%s" % (name, K, theta))
                ends.append(s.check("%s K=%d theta=%s" % (name, K, theta))[True])
            # per-slot chunk_lengths inside one Tc: the slots take different numbers of frames from one chunk, so that the
            # same position of the next chunk holds different frames of their utterances
            s = Both(tr, lex, lm, B, T, K, theta)
            s.advance(x[:7], torch.tensor([7, 2, 1, 0]))
            second = torch.zeros(5, B, 5, dtype=dtype)
            second[:5, 0], second[:3, 1] = x[7:12, 0], x[2:5, 1]
            s.advance(second, torch.tensor([5, 3, 0, 0]))
            ends.append(s.check("lengths K=%d theta=%s" % (K, theta))[True])
            for e in ends[1:]:
                _same(e, ends[0], "chunkings agree K=%d theta=%s" % (K, theta))
            assert ends[0]["frames"].tolist() == il.tolist() and not ends[0]["status"].any()
            shared += sum(len({q for _, q in kept}) < len(kept) for kl in s.ref.kept() for kept in kl)
            if K == ALL and theta == INF:
                p = ends[0]["path"][0]
                # at least two separator edges on slot 0's path: under "ones" each is the first frame of a chunk -- the LM walk
                # ran from a set that an earlier call stored
                assert int(((p[1:] == sep) & (p[:-1] != sep)).sum()) >= 2 and ends[0]["word_lengths"][0] >= 2
    assert shared > 0                                      # some frame kept two pairs with one q and different h


# ---------------------------------------------------------------------------------------------------------------- 2. ties
@DTYPES
def test_ties_at_the_last_rank_and_between_sources(dtype):
    lex = small_lexicon()
    lm = integers(arpa_lm(5, 2, 71, keep=(1.0, 0.6, 0.5)))
    g = torch.Generator().manual_seed(32)
    x = torch.randint(-2, 3, (8, 5, 5), generator=g).to(dtype)
    tr, il = torch.zeros(5, 5, dtype=dtype), torch.tensor([8, 8, 5, 1, 0])
    cuts = srcs = 0
    for K in (1, 2, 3, 5, 8):
        for theta in (INF, 1.0, 0.0):
            for chunks in ([0, 3, 3, 8], list(range(9))):
                s = Both(tr, lex, lm, 5, 8, K, theta, 1.0, 1.0, 0.0)
                s.feed(x, il, chunks)
                s.check("ties K=%d theta=%s %s" % (K, theta, chunks))
                cuts += s.ref.tie_cuts
                srcs += s.ref.src_ties
    assert cuts > 0 and srcs > 0


# ---------------------------------------------------------------------------------------------------------------- 3. wide
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
    s = Both(tr * 0.25, lex, lm, 2, 6, 1200, INF, 0.5, -0.2, 0.1)
    s.feed(x * 0.25, torch.tensor([6, 5]), [0, 1, 3, 6])   # flat emissions: many pairs stay close
    assert max(max(c) for c in s.ref.cands()) > 1024 and max(max(z) for z in s.ref.sizes()) > 1024
    s.check("wide")


# ---------------------------------------------------------------------------------------------------------------- 4. limits
@DTYPES
def test_the_largest_beam(dtype):
    lex, lm, x, tr, _ = grid_case(2, dtype, T=4)
    s = Both(tr, lex, lm, 4, 4, 8192)
    s.feed(x, torch.tensor([4, 3, 1, 0]), [0, 1, 4])
    s.check("K=8192")
    with pytest.raises(RuntimeError, match="unsupported|limit|support"):
        _asg().BeamWordStream(tr.to(DEV), lex, lm, 4, 4, 8193, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------- 5. ends
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
    s = Both(tr, lex, lm, 3, 5, 8, INF, 1.0, 0.0, 0.0)
    s.feed(x, il, [0, 2, 5], check="ends")
    got = s.check("ends")
    assert got[True]["words"][0].tolist() == [0, 1, -1, -1, -1] and got[True]["path"][0].tolist() == [0, 2, 0, 1, 2]
    assert got[True]["words"][1].tolist() == [1, 1, -1, -1, -1] and got[True]["word_lengths"].tolist()[:2] == [2, 2]
    assert got[False]["words"][1].tolist() == [1, -1, -1, -1, -1]          # the prefix: the separator edge's word, no final word
    assert got[False]["path"][1].tolist() == [0, 1, 2, 0, 1]
    # an LM that knows word 0 only: the step of word 1 is rejected on its separator edge and at the end
    rej = WordLM(2, [0, 1], [0], [-0.5], [0], [-1], [0.0], 0, [-1.0])
    s = Both(tr, lex, rej, 3, 5, 8, INF, 1.0, 0.0, 0.0)
    s.feed(x, il, [0, 1, 4, 5])
    got = s.check("rejected")
    assert (got[True]["words"] != 1).all() and (got[True]["scores"] > -np.inf).all()
    # every path ends mid-word: final gives no hypothesis, the prefix gives one
    long = Lexicon([[0, 1, 0]], 3, 2)
    s = Both(tr, long, WordLM.null(1), 3, 5, 8, INF, 1.0, 0.0, 0.0)
    s.feed(x[:2], torch.tensor([2, 2, 2]), [0, 1, 2])
    got = s.check("mid-word")
    assert (got[True]["scores"] == -np.inf).all() and (got[True]["frames"] == 2).all()
    for n in ONE[1:]:
        assert (got[True][n] == (0 if n.endswith("lengths") else -1)).all(), n
    assert (got[False]["scores"] > -np.inf).all() and (got[False]["word_lengths"] == 0).all()
    assert got[False]["path"][1, :2].tolist() == [0, 1] and (got[False]["states"][:, 1] > 0).all()     # ... that ends mid-word


# ---------------------------------------------------------------------------------------------------------------- 6. layouts
@pytest.mark.parametrize("N", [141, 142], ids=["transitions-in-lds", "transitions-in-global-memory"])
def test_both_transition_layouts(N):
    """float64, K = 8: 4096 + 8 * 16 + N * N * 8 bytes is within the 160 KiB of LDS for N = 141 and beyond them for N = 142."""
    from torch_asg_amd import Lexicon
    K = 8
    assert (4096 + K * 16 + N * N * 8 <= 160 * 1024) == (N == 141)
    lex = Lexicon([[3, 7], [3, 100, 5], [N - 2]], N, N - 1)
    lm = arpa_lm(3, 2, 73)
    x, tr = _normal(6, 2, N, 37, torch.float64)
    for t, lab in enumerate([3, 7, N - 1, N - 2, N - 1, 3]):
        x[t, 0, lab] += 6.0
    s = Both(tr, lex, lm, 2, 6, K, INF)
    s.feed(x, torch.tensor([6, 4]), [0, 2, 6], check="N=%d" % N)
    got = s.check("N=%d" % N)
    assert got[True]["word_lengths"][0] >= 2 and max(max(z) for z in s.ref.sizes()) > 1


# ---------------------------------------------------------------------------------------------------------------- 7. empty
@DTYPES
def test_a_beam_that_empties_inside_a_chunk_and_at_both_ends_of_one(dtype):
    lex, lm, x, tr, _ = grid_case(2, dtype, T=9)
    x = x[:, :3].clone()
    x[4, 0] = -INF                                         # chunks [3, 3, 3]: inside the second chunk,
    x[3, 1] = -INF                                         # on its first frame,
    x[5, 2] = -INF                                         # on its last
    il = torch.tensor([9, 9, 9])
    s = Both(tr, lex, lm, 3, 12, 6, 4.0)
    s.feed(x, il, [0, 3, 6, 9], check="empty")
    sizes = s.ref.sizes()
    for b, t0 in enumerate((4, 3, 5)):
        assert all(z > 0 for z in sizes[b][:t0]) and all(z == 0 for z in sizes[b][t0:]) and len(sizes[b]) == 9
    got = s.check("empty")
    for final in (False, True):
        assert (got[final]["scores"] == -np.inf).all() and got[final]["frames"].tolist() == [9, 9, 9]      # frames still counts
        assert (got[final]["path"] == -1).all() and not got[final]["status"].any()
    s.reset(torch.tensor([True, False, False]))            # the slot stays empty until reset
    y, _ = _normal(2, 3, 5, 38, dtype)
    s.advance(y)
    got = s.check("after the reset of slot 0")
    assert got[False]["frames"].tolist() == [2, 11, 11]
    assert got[False]["scores"][0] > -np.inf and (got[False]["scores"][1:] == -np.inf).all()


# ---------------------------------------------------------------------------------------------------------------- 8. blocks
def test_collapse_blocks_and_max_frames_passed_by_replays():
    """max_frames = 130: results at 63, 64, 65 and 129 frames (the collapse works in blocks of 64 frames), at max_frames exactly,
    and beyond it through replays of a captured one-frame advance -- the host's bound does not see a replay; the device clamps,
    `status` says so and the result is the decode of the first max_frames frames."""
    lex, lm, _, tr, _ = grid_case(3, torch.float32)
    M, B, K, theta = 130, 2, 4, 6.0
    x, _ = _normal(M + 2, B, 5, 39, torch.float32)
    s = Both(tr, lex, lm, B, M, K, theta)
    s.advance(x[:63])                                      # (also the warm-up of the kernel that is captured below)
    s.check("63 frames")
    buf = torch.zeros(1, B, 5, device=DEV)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        s.dev.advance(buf)                                 # (the capture itself runs nothing)

    def replay(t):
        buf.copy_(x[t:t + 1])
        gr.replay()
        s.ref.advance(x[t:t + 1].numpy())
    replay(63)
    s.check("64 frames")
    replay(64)
    s.check("65 frames")
    s.advance(x[65:129])
    s.check("129 frames")
    replay(129)
    got = s.check("max_frames exactly")
    assert got[True]["frames"].tolist() == [M, M] and not got[True]["status"].any()
    replay(130)
    replay(131)
    got = s.check("beyond max_frames")
    assert got[True]["frames"].tolist() == [M, M] and got[True]["status"].tolist() == [1, 1]
    _same_as_one_shot(got[True], _gpu_one_shot(x[:M], tr, lex, lm, None, K, theta), M, "the first max_frames frames")
    with pytest.raises(ValueError, match="max_frames"):
        s.dev.advance(x[:3].to(DEV))                       # the host's own bound counts what it was offered: 128 + 3


# ---------------------------------------------------------------------------------------------------------------- 9. plumbing
def test_masked_reset_mid_stream():
    lex, lm, x, tr, _ = grid_case(3, torch.float32)
    y, _ = _normal(12, 4, 5, 40, torch.float32)
    il = torch.tensor([12, 12, 12, 12])
    s = Both(tr, lex, lm, 4, 12, 5, 5.0)
    s.advance(x[:6])
    s.reset(torch.tensor([False, True, False, True]))
    mixed = x[6:].clone()
    mixed[:, 1], mixed[:, 3] = y[:6, 1], y[:6, 3]          # slots 1 and 3 start a new utterance, the others go on
    s.advance(mixed)
    got = s.check("masked reset")[True]
    assert got["frames"].tolist() == [12, 6, 12, 6] and not got["status"].any()
    want_x = _gpu_one_shot(x, tr, lex, lm, il, 5, 5.0)
    want_y = _gpu_one_shot(y[:6], tr, lex, lm, None, 5, 5.0)
    for b in range(4):
        want, L = (want_x, 12) if b % 2 == 0 else (want_y, 6)
        _same_as_one_shot({n: got[n][b:b + 1] for n in ONE}, {n: want[n][b:b + 1] for n in ONE}, L, "slot %d" % b)
    s.dev.reset(torch.tensor([1, 0, 0, 0], dtype=torch.int32))             # an integer mask from the host
    s.ref.reset(np.array([1, 0, 0, 0]))
    got = s.check("integer mask")[True]
    assert got["frames"].tolist() == [0, 6, 12, 6] and got["scores"][0] == -np.inf
    s.reset()
    assert s.check("full reset")[True]["frames"].tolist() == [0, 0, 0, 0]


def test_capture_of_advance_and_result_with_six_replays():
    lex, lm, _, tr, _ = grid_case(3, torch.float32)
    Tc, B, K, theta = 4, 3, 12, 6.0
    T = 6 * Tc
    x, _ = _normal(T, B, 5, 41, torch.float32)
    il = torch.tensor([T, 9, T - 2])
    s = Both(tr, lex, lm, B, T, K, theta)
    buf = torch.zeros(Tc, B, 5, device=DEV)
    n = torch.zeros(B, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.dev.advance(buf, n)                              # warm-up; n = 0: the state stays as it is
        s.dev.result(False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        s.dev.advance(buf, n)
        out = s.dev.result(False)
    s.dev.reset()                                          # (the capture itself ran nothing)
    for c in range(6):
        buf.copy_(x[c * Tc:(c + 1) * Tc])
        n.copy_((il - c * Tc).clamp(0, Tc))
        gr.replay()
        torch.cuda.synchronize()
        s.ref.advance(x[c * Tc:(c + 1) * Tc].numpy(), (il - c * Tc).clamp(0, Tc).numpy())
        _same({k: o.cpu().numpy() for k, o in zip(NAMES, out)}, s.ref.result(False), "replay %d" % c)
    got = s.check("six replays")[True]
    _same_as_one_shot(got, _gpu_one_shot(x, tr, lex, lm, il, K, theta), T, "six replays")
    assert got["frames"].tolist() == il.tolist() and not got["status"].any()


def test_two_streams_give_identical_bits():
    lex, lm = wide_lexicon_and_lm()
    x, tr = _normal(12, 6, 40, 36, torch.float32)
    xd, trd = (x * 0.25).to(DEV), tr.to(DEV)
    il = torch.tensor([12, 3, 0, 1, 11, 7])
    runs = []
    for _ in range(2):
        s = _asg().BeamWordStream(trd, lex, lm, 6, 12, 300, 6.0, 0.5, -0.2, 0.1)
        for t0, t1 in ((0, 5), (5, 6), (6, 12)):
            s.advance(xd[t0:t1], (il - t0).clamp(0, t1 - t0).to(DEV))
        runs.append((_res(s, True), _res(s, False)))
    for u, v in zip(runs[0], runs[1]):
        _same(u, v, "two streams")
    _same_as_one_shot(runs[0][0], _gpu_one_shot(x * 0.25, tr, lex, lm, il, 300, 6.0, 0.5, -0.2, 0.1), 12, "wide, one shot")


# ---------------------------------------------------------------------------------------------------------------- 10. decoders
@DTYPES
def test_against_the_devices_own_decoders(dtype):
    A = _asg()
    lex, lm, x, tr, il = grid_case(3, dtype)
    T, B = 12, 4
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    loss = A.ASGLoss(5).to(DEV).to(dtype)
    with torch.no_grad():
        loss.transition.copy_(trd)
    for K, theta in ((3, INF), (16, 4.0), (ALL, INF)):
        s = loss.beam_word_stream(lex, lm, B, T + 3, K, theta, LW, WS, TS)         # the module method
        for t0, t1 in ((0, 4), (4, 5), (5, 12)):
            s.advance(xd[t0:t1], (il - t0).clamp(0, t1 - t0).to(DEV))
        _same_as_one_shot(_res(s), _gpu_one_shot(x, tr, lex, lm, il, K, theta), T, "K=%d" % K)
    # the null LM: the search over pairs is the search over product states of the lexicon's own graph
    null = A.WordLM.null(5)
    for K, theta in ((3, INF), (7, 1.5)):
        w = A.BeamWordStream(trd, lex, null, B, T, K, theta, 1.0, 0.0, -0.3, dtype)
        g = A.BeamStream(trd, lex.graph, B, T, K, theta, 1.0, -0.3, dtype)
        for t0, t1 in ((0, 4), (4, 5), (5, 12)):
            for s in (w, g):
                s.advance(xd[t0:t1], (il - t0).clamp(0, t1 - t0).to(DEV))
            for final in (False, True):
                got, want = _res(w, final), g.result(final)
                for n, o in zip(("scores", "path", "tokens", "token_lengths", "states", "frames", "status"), want):
                    assert np.array_equal(got[n], o.cpu().numpy()), (n, K, theta, t1, final)
    if dtype == torch.float32:
        # half precision chunks are widened to the transition's dtype; a strided chunk; the transition is read at every advance
        s, r = (A.BeamWordStream(trd, lex, lm, B, T, 16) for _ in range(2))
        s.advance(xd[:9].to(torch.bfloat16), ild.clamp(max=9))
        r.advance(xd[:9].to(torch.bfloat16).float(), ild.clamp(max=9))
        _same(_res(s), _res(r), "bfloat16")
        s.reset()
        s.advance(xd.transpose(0, 1).contiguous().transpose(0, 1), ild)
        _same_as_one_shot(_res(s), _gpu_one_shot(x, tr, lex, lm, il, 16, INF, 1.0, 0.0, 0.0), T, "strided")
        tr2 = trd.clone()
        s = A.BeamWordStream(tr2, lex, lm, B, T, 16)
        ref = BeamWordStreamRef(tr.numpy(), lex, lm, B, T, 16)
        s.advance(xd[:5])
        ref.advance(x[:5].numpy())
        tr2.mul_(0.5)
        s.beam_threshold = 1.0                             # ... and so is the attribute
        s.advance(xd[5:])
        ref.advance(x[5:].numpy(), transition=tr.numpy() * np.float32(0.5), beam_threshold=1.0)
        _same(_res(s), ref.result(True), "transition and threshold changed between chunks")


def test_the_older_decoders_are_undisturbed_by_streaming_calls():
    A = _asg()
    lex, lm, x, tr, il = grid_case(3, torch.float32)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)

    def older():
        g = A.BeamStream(trd, lex.graph, 4, 12, 6, 4.0, 0.8, -0.5)
        g.advance(xd[:5], ild.clamp(max=5))
        g.advance(xd[5:], (ild - 5).clamp(0, 7))
        outs = list(A.beam_decode_graph(xd, trd, lex.graph, ild, 6, 4.0, 0.8, -0.5)) + list(g.result(True))
        outs += list(A.beam_decode_words(xd, trd, lex, lm, ild, 64, 4.0, LW, WS, TS))
        return [o.cpu() for o in outs]
    before = older()
    s = A.BeamWordStream(trd, lex, lm, 4, 12, 64, 4.0, LW, WS, TS)
    s.advance(xd[:7], ild.clamp(max=7))
    _res(s, False)
    after = older()
    s.advance(xd[7:], (ild - 7).clamp(0, 5))
    again = older()
    for u, v, w in zip(before, after, again):
        assert torch.equal(u, v) and torch.equal(u, w)
    want = beam_word_ref(x.numpy(), tr.numpy(), lex, lm, il.numpy(), 64, 4.0, LW, WS, TS)
    for n, o in zip(ONE, before[-8:]):
        assert np.array_equal(o.numpy(), want[n]), n
    _same_as_one_shot(_res(s), want, 12, "the stream after the older decoders")


# ---------------------------------------------------------------------------------------------------------------- 11. errors
def test_errors():
    A = _asg()
    lex, lm = small_lexicon(), arpa_lm(5, 2, 62)
    tr = torch.randn(5, 5, device=DEV)
    s = A.BeamWordStream(tr, lex, lm, 2, 6, 4)
    x = torch.randn(3, 2, 5, device=DEV)
    with pytest.raises(RuntimeError):
        s.advance(x.cpu())
    with pytest.raises(RuntimeError):
        s.advance(torch.randn(3, 2, 6, device=DEV))                  # another alphabet
    with pytest.raises(RuntimeError):
        s.advance(torch.randn(3, 3, 5, device=DEV))                  # another batch
    with pytest.raises(RuntimeError):
        s.advance(x.double())
    with pytest.raises(RuntimeError):
        s.advance(x, torch.tensor([3, 3], dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        s.advance(x, torch.tensor([3], device=DEV))
    with pytest.raises(RuntimeError):
        s.reset(torch.tensor([1, 0, 1], device=DEV))
    with pytest.raises(RuntimeError):
        A.BeamWordStream(tr.double(), lex, lm, 2, 6, 4)              # not the stream's dtype
    with pytest.raises(RuntimeError):
        A.BeamWordStream(tr.cpu(), lex, lm, 2, 6, 4)                 # CPU tensors
    with pytest.raises(RuntimeError):
        A.BeamWordStream(torch.randn(6, 6, device=DEV), lex, lm, 2, 6, 4)
    with pytest.raises(TypeError):
        A.BeamWordStream(tr, lex.graph, lm, 2, 6, 4)
    with pytest.raises(RuntimeError, match="knows"):
        A.BeamWordStream(tr, lex, A.WordLM.null(2), 2, 6, 4)
    s.beam_threshold = -1.0
    with pytest.raises(ValueError):
        s.advance(x)
    s.beam_threshold = INF
    assert _res(s)["frames"].tolist() == [0, 0]                      # nothing above reached the state
    s.advance(x)
    s.advance(x)
    with pytest.raises(ValueError, match="max_frames"):
        s.advance(x[:1])
    s.advance(x[:0])                                                 # a chunk of no frames is fine
    res = _res(s)
    assert res["frames"].tolist() == [6, 6] and not res["status"].any()
    s.reset()
    s.advance(x)
    assert _res(s)["frames"].tolist() == [3, 3]
