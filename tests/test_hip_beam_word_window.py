"""GPU tests (-m gpu) of windowed streaming beam decoding with a lexicon and a word LM (`torch_asg_amd.BeamWordWindowStream`,
csrc/asg_beam_word_window.hip): every output of every call -- what each `advance` commits, words included, the tail, `frames` /
`committed` / `status` of `result` -- is, byte for byte, that of the restatement (tests/beam_word_window_ref.py, held to the
one-shot restatement on the CPU by tests/test_beam_word_window_cpu.py), over windows, commit periods, beams, thresholds, dtypes
and chunkings; the word regimes (a separator edge on a commit boundary, on a call boundary, on the boundary of the tail, a word
over three commits, a final word behind an empty tail, two histories on one product state), each asserted from the
restatement's records; dozens of wraps of the rings; forced commits; a beam that empties after a commit; integer ties; mark
sets wider than one stride of the workgroup; the largest beam; both transition layouts; the device's own one-shot decoder,
unbounded word stream and windowed graph stream; masked reset; capture and replay; determinism; errors; and the older beam
routes after window calls."""
import numpy as np
import pytest
import torch

import test_beam_word_window_cpu as cpu
from beam_word_cases import arpa_lm, eighths, integers, small_lexicon
from beam_word_window_ref import COMMIT, RESULT, BeamWordWindowRef

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
ALL = 1024                                                 # more than every pair of the small cases
LW, WS, TS = cpu.LW, cpu.WS, cpu.TS
SCORES = cpu.SCORES
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
NP = {torch.float32: np.float32, torch.float64: np.float64}
WIDE = cpu.WIDE
ONE = ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths")


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _same(got, want, what, names):
    """Every array bit for bit (array_equal would let -0 pass for +0)."""
    for n in names:
        g, w = got[n], np.ascontiguousarray(want[n])
        assert g.dtype == w.dtype and g.shape == w.shape, (n, what)
        assert g.tobytes() == w.tobytes(), "%s %s" % (n, what)


class Both:
    """The device stream and the restatement, driven by the same calls; every output of every call compared."""

    def __init__(self, tr, lex, lm, B, W, P, K, theta=INF, lw=LW, ws=WS, ts=TS, cls=BeamWordWindowRef):
        self.dev = _asg().BeamWordWindowStream(tr.to(DEV), lex, lm, B, W, P, K, theta, lw, ws, ts, tr.dtype, DEV)
        self.ref = cls(tr.numpy(), lex, lm, B, W, P, K, theta, lw, ws, ts, NP[tr.dtype])
        self.B, self.W = B, W
        self.cat = [tuple([] for _ in WIDE) for _ in range(B)]      # what the device has committed, per slot

    def advance(self, x, n, what):
        out = self.dev.advance(x.to(DEV), None if n is None else n.to(DEV))
        assert type(out).__name__ == "BeamWordWindowCommit" and out._fields == ("path", "states", "lm_states", "tokens",
                                                                                "token_lengths", "words", "word_lengths", "frames")
        got = {k: getattr(out, k).cpu().numpy() for k in COMMIT}
        want = dict(zip(COMMIT, self.ref.advance(x.numpy(), None if n is None else n.numpy())))
        assert got["path"].shape == (self.B, self.W + x.shape[0])
        _same(got, want, what, COMMIT)
        for b in range(self.B):
            for i, (k, m) in enumerate(zip(WIDE, ("frames", "frames", "frames", "token_lengths", "word_lengths"))):
                self.cat[b][i].extend(got[k][b, :got[m][b]].tolist())
        return got

    def results(self, what, finals=(False, True)):
        res = {}
        for final in finals:
            out = self.dev.result(final)
            assert type(out).__name__ == "BeamWordWindowResult" and out._fields == RESULT
            res[final] = {k: o.cpu().numpy() for k, o in zip(RESULT, out)}
            assert res[final]["path"].shape == (self.B, self.W)
            _same(res[final], self.ref.result(final), "%s final=%s" % (what, final), RESULT)
        return res

    def feed(self, x, il, cuts, what, results=False):
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            self.advance(x[t0:t1], None if il is None else (il - t0).clamp(0, t1 - t0), "%s chunk %d:%d" % (what, t0, t1))
            if results:
                self.results("%s after %d" % (what, t1))
        return self.results(what)

    def feed_ragged(self, x, il, Tc, seed, what):
        """Calls that each offer Tc frames of which every slot takes a number of its own: the slots drift apart inside one shape."""
        T, B, N = x.shape
        g = torch.Generator().manual_seed(seed)
        pad = torch.cat([x, torch.zeros(Tc, B, N, dtype=x.dtype)])
        pos = torch.zeros_like(il)
        while bool((pos < il).any()):
            n = torch.minimum(torch.randint(0, Tc + 1, (B,), generator=g), il - pos)
            chunk = torch.stack([pad[int(pos[b]):int(pos[b]) + Tc, b] for b in range(B)], 1)
            self.advance(chunk, n, "%s ragged at %s" % (what, pos.tolist()))
            self.results("%s ragged at %s" % (what, pos.tolist()))
            pos = pos + n
        return self.results(what)

    def reset(self, mask=None):
        self.dev.reset(None if mask is None else mask.to(DEV))
        self.ref.reset(None if mask is None else mask.numpy())


def _np_case(T, B, N, seed, dtype, integer=False):
    x, tr, il = cpu.case(T, B, N, seed, NP[dtype], integer)
    return torch.from_numpy(x), torch.from_numpy(tr), torch.from_numpy(il)


def _gpu_one_shot(x, tr, lex, lm, il, K, theta=INF, lw=LW, ws=WS, ts=TS):
    out = _asg().beam_decode_words(x.to(DEV), tr.to(DEV), lex, lm, None if il is None else il.to(DEV), K, theta, lw, ws, ts)
    return {n: o.cpu().numpy() for n, o in zip(ONE, out)}


# ---------------------------------------------------------------------------------------------------------------- 1. the grid
@pytest.mark.parametrize("K", [1, 3, 8, ALL])
@pytest.mark.parametrize("weights", ["eighths", "integers"])
@DTYPES
def test_every_output_of_every_call_equals_the_restatement(dtype, weights, K):
    lex = small_lexicon(SCORES)
    lm = (eighths if weights == "eighths" else integers)(arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5)))
    T, B = 40, 4
    x, tr, il = _np_case(T, B, 5, 14, dtype, integer=weights == "integers")
    il[3] = il[3].clamp(min=2)
    assert il[0] == T and il[1] == 0 and il[2] == 1
    for t, lab in enumerate([0, 4, 1, 0, 4, 2, 4, 0, 1, 2, 4, 0] * 3 + [4, 2, 4, 0]):      # slot 0 spells words: its path crosses
        x[t, 0, lab] += 3.0                                                             # separators, and commits carry words
    turn = {1: 0, 3: 1, 8: 2, ALL: 3}[K]
    forced = exact = words = 0
    for theta in (INF, 2.0, 0.0):
        one = _gpu_one_shot(x, tr, lex, lm, il, K, theta)
        for W in (4, 8, 16):
            for P in (1, 3, W):
                kind = turn % 6
                cuts = {0: list(range(T + 1)), 1: [0, T], 2: [0, 1, 8, 8, 24, 40],
                        3: None,                                            # per-slot lengths inside one Tc
                        4: list(range(0, T, 3 * P + 1)) + [T],              # a chunk spans several commit attempts
                        5: [0, 0, 20, 20, 40, 40]}[kind]                    # chunks of no frames
                what = "K=%d theta=%s W=%d P=%d chunking %d" % (K, theta, W, P, kind)
                turn += 1
                s = Both(tr, lex, lm, B, W, P, K, theta)
                res = s.feed_ragged(x, il, 7, turn, what) if cuts is None else s.feed(x, il, cuts, what, results=True)
                # the search is the device's own one-shot search, and without a forced commit so is the transcript
                assert res[True]["scores"].tobytes() == one["scores"].tobytes(), what
                exact += cpu.check_exact(s.cat, res[True], one, il.numpy(), what)
                forced += int((res[True]["status"] & 1).sum())
                words += sum(len(c[4]) for c in s.cat)
    assert exact > 0 and words >= 27 * 3 and (forced > 0 or K == 1)             # (three words or more per stream on average)


# ---------------------------------------------------------------------------------------------------------------- 2. words
def _word_both(seed, W, P, K, theta, T=24, shift=0.0):
    lex, lm, x, tr, il = cpu.word_case(seed, T)
    x[:, :, cpu.SEP] += shift
    s = Both(torch.from_numpy(tr), lex, lm, 1, W, P, K, theta, cls=cpu.Recording)
    return s, lex, lm, torch.from_numpy(x), torch.from_numpy(tr), torch.from_numpy(il)


def test_a_separator_edge_on_a_commit_boundary_and_on_a_call_boundary():
    for one_call in (True, False):
        s, lex, lm, x, tr, il = _word_both(cpu.SEED_BOUNDARY, 8, 2, 3, INF)
        T = int(il[0])
        calls = []
        for t0, t1 in ((0, T),) if one_call else zip(range(T), range(1, T + 1)):
            base = s.ref.slots[0].base
            got = s.advance(x[t0:t1], None, "boundary %d:%d" % (t0, t1))
            calls.append((base, int(got["frames"][0])))
            s.results("boundary after %d" % t1)
        v = s.ref.slots[0]
        starts = [f0 for f0, _ in v.commits if f0 in cpu.edge_frames(s.cat[0][0])]
        assert v.status == 0 and starts                    # the regime: a segment begins with the separator of an edge
        if one_call:
            assert len(v.commits) > 1 and min(starts) > v.commits[0][0]       # ... behind an earlier segment of the same call
        else:
            assert [b for b, n in calls if n and b in starts]                  # ... as the first frame that a call commits
        one = _gpu_one_shot(x, tr, lex, lm, il, 3)
        assert cpu.check_exact(s.cat, s.results("boundary")[True], one, il.numpy(), "boundary") == 1
        assert len(s.cat[0][4]) >= len(starts)


def test_a_separator_edge_on_the_first_frame_of_the_tail():
    s, lex, lm, x, tr, il = _word_both(cpu.SEED_TAIL, 8, 2, 3, INF)
    hits = 0
    for t in range(int(il[0])):
        s.advance(x[t:t + 1], None, "tail %d" % t)
        r = s.results("tail after %d" % t)[False]
        v = s.ref.slots[0]
        if 1 <= v.base < v.pos and r["path"][0, 0] == cpu.SEP and v.carry != cpu.SEP:
            hits += 1                                      # the regime: the tail begins with the separator of an edge
            assert r["words"][0, 0] == lex.word_of_state[v.carry_state] >= 0
    assert hits > 0 and s.ref.slots[0].status == 0


def test_a_word_whose_frames_span_three_commits():
    s, lex, lm, x, tr, il = _word_both(cpu.SEED_THREE, 4, 1, 3, 1.0, shift=-2.0)
    T = int(il[0])
    res = s.feed(x, il, [0, 5, 6, T], "three commits", results=True)
    v = s.ref.slots[0]
    path = s.cat[0][0]
    spans = []
    for e in cpu.edge_frames(path):
        w0 = e
        while w0 > 0 and path[w0 - 1] != cpu.SEP:
            w0 -= 1
        spans.append(len({i for i, (f0, f1) in enumerate(v.commits) if f0 <= e and f1 >= w0}))
    assert v.status == 0 and spans and max(spans) >= 3 and len(s.cat[0][4]) == len(spans)             # the regime
    assert cpu.check_exact(s.cat, res[True], _gpu_one_shot(x, tr, lex, lm, il, 3, 1.0), il.numpy(), "three") == 1


def test_a_final_word_with_everything_else_committed():
    s, lex, lm, x, tr, il = _word_both(cpu.SEED_FINAL, 4, 1, 1, INF, T=9)
    T = int(il[0])
    res = s.feed(x, il, [0, 4, T], "final word", results=True)
    v = s.ref.slots[0]
    assert v.base == v.pos == T and v.status == 0 and lex.word_of_state[s.cat[0][1][-1]] >= 0         # the regime
    assert (res[True]["path"] == -1).all() and res[True]["word_lengths"][0] == 1 and res[False]["word_lengths"][0] == 0
    assert res[True]["words"][0, 0] == lex.word_of_state[s.cat[0][1][-1]]
    assert cpu.check_exact(s.cat, res[True], _gpu_one_shot(x, tr, lex, lm, il, 1), il.numpy(), "final") == 1


def test_two_histories_on_one_product_state_do_not_converge():
    s, lex, lm, x, tr, il = _word_both(cpu.SEED_SHARED, 8, 1, 2, INF)
    T = int(il[0])
    s.feed(x, il, [0, 3, T], "shared", results=True)
    v = s.ref.slots[0]
    shared = [(pos, c) for (pos, pairs), (_, _, c, _) in zip(v.sets, v.attempts)
              if len(pairs) > 1 and len({q for _, q in pairs}) == 1]
    assert shared and all(c is None or c < pos - 1 for pos, c in shared)                              # the regime


# ---------------------------------------------------------------------------------------------------------------- 3. the window
def test_dozens_of_wraps_with_one_slot():
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 2, 62, keep=(1.0, 1.0)))
    T, B, W = 300, 2, 8
    x, tr, _ = _np_case(T, B, 5, 61, torch.float32)
    il = torch.tensor([T, T - 5])
    for P in (1, 8):
        s = Both(tr, lex, lm, B, W, P, 1)
        res = s.feed(x, il, list(range(0, T, 37)) + [T], "K=1 P=%d" % P)
        assert all(v.status == 0 and v.pos > 30 * W and v.base == v.pos // P * P for v in s.ref.slots)
        one = _gpu_one_shot(x, tr, lex, lm, il, 1)
        assert cpu.check_exact(s.cat, res[True], one, il.numpy(), "wraps") == int((one["scores"] > -INF).sum())
        assert min(len(c[4]) for c in s.cat) > 10          # dozens of words committed


def test_forced_commits_keep_the_specified_outputs():
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 2, 62, keep=(1.0, 0.6)))
    T, B, W, P = 30, 2, 6, 2
    x, tr, _ = _np_case(T, B, 5, 64, torch.float64)
    x, tr = x * 0.05, tr * 0.05                              # flat emissions: the hypotheses stay apart
    il = torch.tensor([T, T - 3])
    ends = []
    for cuts in ([0, 5, 6, 17, 30], list(range(T + 1))):
        s = Both(tr, lex, lm, B, W, P, ALL)
        ends.append((s.feed(x, il, cuts, "forced", results=True), s.cat))
        assert all(v.status == 1 and sum(F for _, _, _, F in v.attempts) > 0 for v in s.ref.slots)    # the regime
    assert ends[0][1] == ends[1][1]
    for final in (False, True):
        _same(ends[0][0][final], ends[1][0][final], "forced, two chunkings", RESULT)
    assert ends[0][0][True]["scores"].tobytes() == _gpu_one_shot(x, tr, lex, lm, il, ALL)["scores"].tobytes()


@DTYPES
def test_a_beam_that_empties_inside_a_chunk_after_a_commit(dtype):
    lex = small_lexicon(SCORES)
    lm = eighths(arpa_lm(5, 2, 62, keep=(1.0, 1.0)))
    T, B, K, W, P = 14, 2, 3, 4, 2
    x, tr, _ = _np_case(T, B, 5, 65, dtype)
    x[9] = -INF                                                     # nothing survives frame 9
    il = torch.tensor([T, 8])
    for cuts in ([0, 6, 12, 14], [0, 9, 10, 14], [0, 10, 14]):
        s = Both(tr, lex, lm, B, W, P, K)
        res = s.feed(x, il, cuts, str(cuts), results=True)
        v = s.ref.slots[0]
        assert v.base > 0 and not v.A and v.pos == T and res[False]["status"][0] & 2 and res[True]["committed"][0] == v.base


@DTYPES
def test_integer_ties_at_the_last_rank_and_between_sources(dtype):
    lex = small_lexicon()
    lm = integers(arpa_lm(5, 2, 71, keep=(1.0, 0.6, 0.5)))
    g = torch.Generator().manual_seed(32)
    T, B = 16, 4
    x = torch.randint(-2, 3, (T, B, 5), generator=g).to(dtype)
    tr, il = torch.zeros(5, 5, dtype=dtype), torch.tensor([T, T, 5, 1])
    cuts = srcs = 0
    for K in (2, 3, 5, 8):
        for theta in (INF, 1.0):
            for chunks, (W, P) in (([0, 3, 3, 8, T], (4, 2)), (list(range(T + 1)), (8, 3))):
                s = Both(tr, lex, lm, B, W, P, K, theta, 1.0, 1.0, 0.0)
                s.feed(x, il, chunks, "ties K=%d theta=%s" % (K, theta), results=True)
                cuts += s.ref.s.tie_cuts
                srcs += s.ref.s.src_ties
    assert cuts > 0 and srcs > 0


class _Sized(BeamWordWindowRef):
    """The restatement that records the size of the set at every attempt."""

    def _attempt(self, v, out):
        v.na = getattr(v, "na", []) + [len(v.A)]
        super()._attempt(v, out)


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


def test_mark_sets_wider_than_one_stride():
    lex, lm = wide_lexicon_and_lm()
    g = torch.Generator().manual_seed(33)
    x = torch.randn(8, 2, 40, generator=g) * 0.25           # flat emissions: many pairs stay close
    tr = torch.randn(40, 40, generator=g) * 0.25
    il = torch.tensor([8, 5])
    s = Both(tr, lex, lm, 2, 16, 2, 1200, INF, 0.5, -0.2, 0.1, cls=_Sized)
    s.feed(x, il, [0, 1, 3, 8], "wide")
    # more kept pairs than the workgroup has threads at an attempt whose scan walked rows: the marks take two strides
    assert all(max(v.na) > 1024 for v in s.ref.slots)
    assert any(n > 1024 and pos - base >= 2 for v in s.ref.slots for n, (pos, base, _, _) in zip(v.na, v.attempts))


@DTYPES
def test_the_largest_beam(dtype):
    lex = small_lexicon(SCORES)
    lm = arpa_lm(5, 2, 62, keep=(1.0, 0.5, 0.5))
    x, tr, _ = _np_case(6, 4, 5, 31, dtype)
    s = Both(tr, lex, lm, 4, 4, 2, 8192)
    s.feed(x, torch.tensor([6, 3, 1, 0]), [0, 1, 6], "K=8192")
    with pytest.raises(RuntimeError, match="unsupported|limit|support"):
        _asg().BeamWordWindowStream(tr.to(DEV), lex, lm, 4, 4, 2, 8193)


@pytest.mark.parametrize("N", [141, 142], ids=["transitions-in-lds", "transitions-in-global-memory"])
def test_both_transition_layouts(N):
    """float64, K = 8: the fixed 4096 bytes, 16 bytes of marks, the set K * 16 and N * N * 8 bytes of transitions are within the
    160 KiB of LDS for N = 141 and beyond them for N = 142."""
    from torch_asg_amd import Lexicon
    K = 8
    marks = (2 * ((K + 31) // 32) * 4 + 15) // 16 * 16
    assert (4096 + marks + K * (8 + 8) + N * N * 8 <= 160 * 1024) == (N == 141)
    lex = Lexicon([[3, 7], [3, 100, 5], [N - 2]], N, N - 1)
    lm = arpa_lm(3, 2, 73)
    g = torch.Generator().manual_seed(37)
    x = torch.randn(8, 2, N, generator=g, dtype=torch.float64)
    tr = torch.randn(N, N, generator=g, dtype=torch.float64)
    for t, lab in enumerate([3, 7, N - 1, N - 2, N - 1, 3, 7, N - 1]):
        x[t, 0, lab] += 6.0
    s = Both(tr, lex, lm, 2, 4, 2, K, INF)
    res = s.feed(x, torch.tensor([8, 4]), [0, 2, 6, 8], "N=%d" % N, results=True)
    assert len(s.cat[0][4]) + res[True]["word_lengths"][0] >= 3 and len(s.cat[0][0]) > 0


# ---------------------------------------------------------------------------------------------------------------- 4. the device's own
@DTYPES
def test_against_the_devices_own_decoders(dtype):
    A = _asg()
    lex = small_lexicon(SCORES)
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    T, B = 40, 4
    x, tr, il = _np_case(T, B, 5, 47, dtype)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    loss = A.ASGLoss(5).to(DEV).to(dtype)
    with torch.no_grad():
        loss.transition.copy_(trd)
    cuts = [0, 8, 16, 17, 40]
    exact = 0
    for K, theta in ((3, INF), (16, 4.0)):
        want = _gpu_one_shot(x, tr, lex, lm, il, K, theta)
        s = loss.beam_word_window_stream(lex, lm, B, 8, 2, K, theta, LW, WS, TS)         # the module method
        un = loss.beam_word_stream(lex, lm, B, T, K, theta, LW, WS, TS)
        assert s.window == 8 and s.commit_every == 2 and s.dtype == dtype
        cat = [tuple([] for _ in WIDE) for _ in range(B)]
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            n = (ild - t0).clamp(0, t1 - t0)
            new = s.advance(xd[t0:t1], n)
            un.advance(xd[t0:t1], n)
            for b in range(B):
                for i, (k, m) in enumerate(zip(WIDE, ("frames", "frames", "frames", "token_lengths", "word_lengths"))):
                    cat[b][i].extend(getattr(new, k)[b, :int(getattr(new, m)[b])].tolist())
            # the best prefix is the unbounded stream's: its score, and committed + tail its transcript
            a, u = s.result(False), un.result(False)
            assert a.scores.cpu().numpy().tobytes() == u.scores.cpu().numpy().tobytes()
            for b in range(B):
                if int(a.status[b]) & 1 or not float(u.scores[b]) > -INF:
                    continue
                assert cat[b][4] + a.words[b, :int(a.word_lengths[b])].tolist() == u.words[b, :int(u.word_lengths[b])].tolist()
                assert cat[b][3] + a.tokens[b, :int(a.token_lengths[b])].tolist() == u.tokens[b, :int(u.token_lengths[b])].tolist()
        res = {k: o.cpu().numpy() for k, o in zip(RESULT, s.result(True))}
        assert res["scores"].tobytes() == want["scores"].tobytes()
        exact += cpu.check_exact(cat, res, want, il.numpy(), "K=%d" % K)
    assert exact > 0
    # the null LM: the search over pairs is the search over product states of the lexicon's own graph, commits and all
    null = A.WordLM.null(5)
    for K, theta in ((3, INF), (7, 1.5)):
        w = A.BeamWordWindowStream(trd, lex, null, B, 8, 2, K, theta, 1.0, 0.0, -0.3)
        g = A.BeamWindowStream(trd, lex.graph, B, 8, 2, K, theta, 1.0, -0.3, dtype)
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            n = (ild - t0).clamp(0, t1 - t0)
            a, b = w.advance(xd[t0:t1], n), g.advance(xd[t0:t1], n)
            for k in b._fields:
                assert torch.equal(getattr(a, k), getattr(b, k)), (k, K, t1)
            for final in (False, True):
                a, b = w.result(final), g.result(final)
                for k in b._fields:
                    assert torch.equal(getattr(a, k), getattr(b, k)), (k, K, t1, final)
    if dtype == torch.float32:
        s = A.BeamWordWindowStream(trd, lex, lm, B, 8)                           # commit_every defaults to window // 4
        r = A.BeamWordWindowStream(trd, lex, lm, B, 8, 2)
        assert s.commit_every == 2
        a = s.advance(xd[:9].to(torch.bfloat16), ild.clamp(max=9))              # half precision chunks are widened
        b = r.advance(xd[:9].to(torch.bfloat16).float().transpose(0, 1).contiguous().transpose(0, 1), ild.clamp(max=9))
        assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_masked_reset_mid_stream():
    lex = small_lexicon(SCORES)
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    T, B, K, theta = 14, 2, 4, 5.0
    x, tr, _ = _np_case(T, B, 5, 43, torch.float32)
    y, _, _ = _np_case(T, B, 5, 44, torch.float32)
    s = Both(tr, lex, lm, B, 4, 2, K, theta)
    s.advance(x[:6], None, "before the reset")
    mask = torch.tensor([False, True])
    s.reset(mask)
    s.results("after the masked reset")
    mixed = x[6:].clone()
    mixed[:, 1] = y[:T - 6, 1]                                       # slot 1 starts a new utterance, slot 0 goes on
    s.advance(mixed, None, "after the reset")
    res = s.results("the end")[True]
    assert res["frames"].tolist() == [T, T - 6]
    assert res["scores"][0].tobytes() == _gpu_one_shot(x, tr, lex, lm, None, K, theta)["scores"][0].tobytes()
    assert res["scores"][1].tobytes() == _gpu_one_shot(y[:T - 6], tr, lex, lm, None, K, theta)["scores"][1].tobytes()
    s.dev.reset(torch.tensor([1, 0], dtype=torch.int32))             # an integer mask from the host
    out = s.dev.result()
    assert out.frames.tolist() == [0, T - 6] and out.committed.tolist()[0] == 0 and out.status.tolist()[0] == 0


def test_capture_and_replay():
    lex = small_lexicon(SCORES)
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    Tc, B, N, K, theta, W, P = 4, 3, 5, 12, 6.0, 6, 3
    T = 6 * Tc
    x, tr, _ = _np_case(T, B, N, 53, torch.float32)
    il = torch.tensor([T, 9, T - 2])
    s = Both(tr, lex, lm, B, W, P, K, theta)
    buf = torch.zeros(Tc, B, N, device=DEV)
    n = torch.zeros(B, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.dev.advance(buf, n)                                        # warm-up; n = 0: the state stays as it is
        s.dev.result()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        new = s.dev.advance(buf, n)
        tail = s.dev.result(True)
    s.dev.reset()                                                    # (the capture itself ran nothing)
    for c in range(6):
        buf.copy_(x[c * Tc:(c + 1) * Tc])
        cn = (il - c * Tc).clamp(0, Tc)
        n.copy_(cn)
        gr.replay()
        torch.cuda.synchronize()
        want = dict(zip(COMMIT, s.ref.advance(x[c * Tc:(c + 1) * Tc].numpy(), cn.numpy())))
        _same({k: getattr(new, k).cpu().numpy() for k in COMMIT}, want, "replay %d" % c, COMMIT)
        _same({k: o.cpu().numpy() for k, o in zip(RESULT, tail)}, s.ref.result(True), "result of replay %d" % c, RESULT)
    r = s.ref.result()
    assert r["frames"].tolist() == il.tolist() and r["committed"].max() > 0


def test_two_streams_give_identical_bits():
    lex, lm = wide_lexicon_and_lm()
    g = torch.Generator().manual_seed(36)
    x, tr = torch.randn(24, 6, 40, generator=g) * 0.25, torch.randn(40, 40, generator=g)
    xd, trd = x.to(DEV), tr.to(DEV)
    il = torch.tensor([24, 3, 0, 1, 21, 7])
    runs = []
    for _ in range(2):
        s = _asg().BeamWordWindowStream(trd, lex, lm, 6, 8, 2, 300, 6.0, 0.5, -0.2, 0.1)
        outs = []
        for t0 in (0, 8, 16):
            outs += [o.cpu() for o in s.advance(xd[t0:t0 + 8], (il - t0).clamp(0, 8).to(DEV))]
        assert s.result(True).frames.tolist() == il.tolist()
        runs.append(outs + [o.cpu() for o in s.result(True)] + [o.cpu() for o in s.result(False)])
    assert all(u.numpy().tobytes() == v.numpy().tobytes() for u, v in zip(*runs))


def test_errors():
    A = _asg()
    lex, lm = small_lexicon(), arpa_lm(5, 2, 62)
    tr = torch.randn(5, 5, device=DEV)
    s = A.BeamWordWindowStream(tr, lex, lm, 2, 6, 2, 4)
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
        A.BeamWordWindowStream(tr, lex, lm, 2, 6, dtype=torch.float64)           # not the transition's dtype
    with pytest.raises(RuntimeError):
        A.BeamWordWindowStream(tr.cpu(), lex, lm, 2, 6)                          # CPU tensors
    with pytest.raises(RuntimeError):
        A.BeamWordWindowStream(torch.randn(6, 6, device=DEV), lex, lm, 2, 6)
    with pytest.raises(TypeError):
        A.BeamWordWindowStream(tr, lex.graph, lm, 2, 6)
    with pytest.raises(RuntimeError, match="knows"):
        A.BeamWordWindowStream(tr, lex, A.WordLM.null(2), 2, 6)
    for W, P in ((0, None), (4, 0), (4, 5)):
        with pytest.raises(ValueError):
            A.BeamWordWindowStream(tr, lex, lm, 2, W, P)
    s.beam_threshold = -1.0
    with pytest.raises(ValueError):
        s.advance(x)
    s.beam_threshold = INF
    assert s.result().frames.tolist() == [0, 0]                      # nothing above reached the state
    for _ in range(5):                                               # no bound on the frames
        s.advance(x)
    out = s.advance(x[:0])                                           # a chunk of no frames: the empty outputs
    assert tuple(out.words.shape) == (2, 6) and all(bool((o == -1).all()) for o in (out.path, out.states, out.lm_states,
                                                                                   out.tokens, out.words))
    assert out.frames.tolist() == out.token_lengths.tolist() == out.word_lengths.tolist() == [0, 0]
    res = s.result()
    assert res.frames.tolist() == [15, 15] and min(res.committed.tolist()) >= 15 - 6
    s.reset()
    s.advance(x)
    assert s.result().frames.tolist() == [3, 3]


def test_the_older_beam_routes_are_unchanged_after_window_calls():
    A = _asg()
    lex = small_lexicon(SCORES)
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    T, B = 12, 4
    x, tr, il = _np_case(T, B, 5, 61, torch.float32)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)

    def older():
        g = A.BeamStream(trd, lex.graph, B, T, 6, 4.0, 0.8, -0.5)                # 5l
        gw = A.BeamWindowStream(trd, lex.graph, B, 4, 2, 6, 4.0, 0.8, -0.5)      # 5m
        ws = A.BeamWordStream(trd, lex, lm, B, T, 64, 4.0, LW, WS, TS)           # 5o
        outs = []
        for t0, t1 in ((0, 5), (5, T)):
            n = (ild - t0).clamp(0, t1 - t0)
            g.advance(xd[t0:t1], n)
            ws.advance(xd[t0:t1], n)
            outs += list(gw.advance(xd[t0:t1], n))
        outs += list(A.beam_decode_graph(xd, trd, lex.graph, ild, 6, 4.0, 0.8, -0.5))                 # 5i
        outs += list(g.result(True)) + list(gw.result(True)) + list(ws.result(True))
        outs += list(A.beam_decode_words(xd, trd, lex, lm, ild, 64, 4.0, LW, WS, TS))                 # 5n
        outs += [o for o in A.beam_decode_words_nbest(xd, trd, lex, lm, ild, 64, 3, 4.0, LW, WS, TS) if o is not None]   # 5p
        outs += [o for o in ws.result_nbest(3, True) if o is not None]
        return [o.cpu() for o in outs]
    before = older()
    s = Both(tr, lex, lm, B, 4, 2, 64, 4.0)
    s.advance(x[:7], il.clamp(max=7), "the window stream")
    after = older()
    s.advance(x[7:], (il - 7).clamp(0, T - 7), "the window stream")
    again = older()
    for u, v, w in zip(before, after, again):
        assert u.numpy().tobytes() == v.numpy().tobytes() == w.numpy().tobytes()
    s.results("the window stream after the older routes")
