"""GPU tests (-m gpu) of the n best hypotheses of the windowed word-LM beam stream (`BeamWordWindowStream.result_nbest`,
csrc/asg_beam_word_nbest.hip over a window state): after every chunk, prefix and final, every output is byte for byte the
restatement's (tests/beam_word_window_nbest_ref.py, held to the growing stream's n-best restatement on the CPU by
tests/test_beam_word_window_nbest_cpu.py); row 0 is the device's own `result`; while no commit was forced, commits plus tail of
every row are the device's own `BeamWordStream.result_nbest` fed the same chunks.  The sort's padding and strips, the 64-frame
blocks of the two collapses with separators in columns 0 and 64, a tail that wraps the ring, an empty tail with a final word,
forced commits, look-ahead, alignments on and off, the state left alone, an emptied beam, a masked reset, capture and replay,
determinism, and the older routes after the calls.  Every case asserts its regime from the restatement first."""
import numpy as np
import pytest
import torch

import test_beam_word_window_nbest_cpu as cpu
from beam_word_cases import small_lexicon
from beam_word_la_stream_ref import BeamWordLaWindowRef
from beam_word_window_nbest_ref import NAMES, SEQS, word_window_nbest
from beam_word_window_ref import BeamWordWindowRef
from test_hip_beam_word_nbest import every_node_ends_a_word

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
ALL = cpu.ALL
LW, WS, TS = cpu.LW, cpu.WS, cpu.TS
SEP = cpu.SEP
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
NP = {torch.float32: np.float32, torch.float64: np.float64}
ALIGN = ("path", "states", "lm_states")
FULL = dict(path="frames", states="frames", lm_states="frames", tokens="token_lengths", words="word_lengths")


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _nb(s, nbest, final, align=True):
    """One call, with the state compared byte for byte around it."""
    before = s._state.clone()
    out = s.result_nbest(nbest, final, align)
    torch.cuda.synchronize()
    assert torch.equal(before, s._state), "result_nbest wrote to the state"
    assert type(out).__name__ == "BeamWordWindowNbest" and out._fields == NAMES
    return {n: None if o is None else o.cpu().numpy() for n, o in zip(NAMES, out)}


def _same(got, want, what, align=True):
    """Every array bit for bit (array_equal would let -0 pass for +0)."""
    for n in NAMES:
        if n in ALIGN and not align:
            assert got[n] is None, (n, what)
            continue
        g, w = got[n], np.ascontiguousarray(want[n])
        assert g.dtype == w.dtype and g.shape == w.shape, (n, what)
        assert g.tobytes() == w.tobytes(), "%s %s" % (n, what)


class Both:
    """The device's window stream and the restatement driven by the same calls and, with `grow`, the device's own growing
    stream beside them."""

    def __init__(self, tr, lex, lm, B, W, P, K, theta=INF, la=None, grow=0):
        A = _asg()
        look = None if la is None else A.WordLookahead(lex, lm, la)
        self.dev = A.BeamWordWindowStream(tr.to(DEV), lex, lm, B, W, P, K, theta, LW, WS, TS, tr.dtype, DEV, lookahead=look)
        if la is None:
            self.ref = BeamWordWindowRef(tr.numpy(), lex, lm, B, W, P, K, theta, LW, WS, TS, NP[tr.dtype])
        else:
            self.ref = BeamWordLaWindowRef(tr.numpy(), lex, lm, la, B, W, P, K, theta, LW, WS, TS, NP[tr.dtype])
        self.grow = A.BeamWordStream(tr.to(DEV), lex, lm, B, grow, K, theta, LW, WS, TS, tr.dtype, DEV) if grow else None
        self.B, self.W = B, W
        self.cat = [[[] for _ in SEQS] for _ in range(B)]            # what the device has committed, per slot

    def advance(self, x, n=None):
        nd = None if n is None else n.to(DEV)
        out = self.dev.advance(x.to(DEV), nd)
        self.ref.advance(x.numpy(), None if n is None else n.numpy())
        if self.grow is not None:
            self.grow.advance(x.to(DEV), nd)
        fr, tl, wl = (getattr(out, k).cpu().numpy() for k in ("frames", "token_lengths", "word_lengths"))
        for b in range(self.B):
            for i, (k, m) in enumerate(zip(SEQS, (fr[b], fr[b], fr[b], tl[b], wl[b]))):
                self.cat[b][i].extend(getattr(out, k)[b, :m].cpu().tolist())

    def reset(self, mask):
        self.dev.reset(mask.to(DEV))
        self.ref.reset(mask.numpy())
        for b in np.nonzero(mask.numpy())[0]:
            self.cat[b] = [[] for _ in SEQS]
        if self.grow is not None:
            self.grow.reset(mask.to(DEV))

    def check(self, nbests, what, finals=(False, True), align=True, seen=None):
        """-> the restatement's result of the last call."""
        want = None
        for final in finals:
            one = self.dev.result(final)
            for nb in nbests:
                w = "%s nbest=%d final=%s" % (what, nb, final)
                want = word_window_nbest(self.ref, nb, final)
                got = _nb(self.dev, nb, final, align)
                _same(got, want, w, align)
                for n in ("scores", "path", "tokens", "token_lengths", "states", "lm_states", "words", "word_lengths"):
                    if align or n not in ALIGN:                      # row 0: the device's own one-best
                        assert np.ascontiguousarray(got[n][:, 0]).tobytes() == getattr(one, n).cpu().numpy().tobytes(), (n, w)
                for n in ("frames", "committed", "status"):
                    assert got[n].tobytes() == getattr(one, n).cpu().numpy().tobytes(), (n, w)
                if self.grow is not None:
                    self._against_the_growing_stream(got, nb, final, w)
                if seen is not None:
                    self._regimes(want, nb, seen)
        return want

    def _regimes(self, want, nb, seen):
        """What the restatement's state and result say about the regime of this call, counted into `seen`."""
        def add(k, v):
            seen[k] = seen.get(k, 0) + int(v)
        for b, v in enumerate(self.ref.slots):
            nh = int(want["num_hyps"][b])
            sc = want["scores"][b, :nh]
            seen["rows"] = max(seen.get("rows", 0), nh)
            add("padded", nh < nb)
            add("forced" if v.status & 1 else "clear", nh > 0)
            add("empty_tail", nh > 0 and v.base == v.pos)
            add("wrapped", nh > 0 and v.pos > v.base and v.base % self.W > (v.pos - 1) % self.W)
            add("sep0_late", sum(int(r > 0 and rec["sep0"]) for r, rec in enumerate(want["records"][b])))
            add("tied", (sc[1:] == sc[:-1]).sum())

    def _against_the_growing_stream(self, got, nb, final, what):
        """While bit 0 is clear: commits + tail of every row are the row of the device's own BeamWordStream.result_nbest."""
        full = self.grow.result_nbest(nb, final, True)
        full = {n: getattr(full, n).cpu().numpy() for n in full._fields}
        assert got["scores"].tobytes() == full["scores"].tobytes() and got["num_hyps"].tobytes() == full["num_hyps"].tobytes(), what
        for b in range(self.B):
            if got["status"][b] & 1:
                continue
            tail = int(got["frames"][b] - got["committed"][b])
            for r in range(int(got["num_hyps"][b])):
                lens = dict(path=tail, states=tail, lm_states=tail, tokens=got["token_lengths"][b, r],
                            words=got["word_lengths"][b, r])
                for i, n in enumerate(SEQS):
                    if got[n] is None:                               # (no alignments asked for)
                        continue
                    m = full["frames"][b] if FULL[n] == "frames" else full[FULL[n]][b, r]
                    assert self.cat[b][i] + got[n][b, r, :lens[n]].tolist() == full[n][b, r, :m].tolist(), (n, b, r, what)


def _case(T, B, seed, dtype, integer=False):
    x, tr, il = cpu.emissions(T, B, seed, NP[dtype], integer)
    return torch.from_numpy(x), torch.from_numpy(tr), torch.from_numpy(il)


def _chunks(name, x, il):
    """The (chunk, lengths) of a chunking: cuts of the utterances, or calls of 7 frames of which every slot takes a number of
    its own."""
    T, B, N = x.shape
    if name == "ragged":
        g = torch.Generator().manual_seed(5)
        pad = torch.cat([x, torch.zeros(7, B, N, dtype=x.dtype)])
        pos = torch.zeros_like(il)
        while bool((pos < il).any()):
            n = torch.minimum(torch.randint(0, 8, (B,), generator=g), il - pos)
            yield torch.stack([pad[int(pos[b]):int(pos[b]) + 7, b] for b in range(B)], 1), n
            pos = pos + n
    else:
        cuts = {"ones": list(range(T + 1)), "whole": [0, T], "1-7-0-16": [0, 1, 8, 8, 24]}[name]
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            yield x[t0:t1], (il - t0).clamp(0, t1 - t0)


# ---------------------------------------------------------------------------------------------------------------- 1. the grid
@pytest.mark.parametrize("K", [1, 3, 8, ALL])
@pytest.mark.parametrize("weights", ["random", "integers"])
@DTYPES
def test_every_row_after_every_chunk(dtype, weights, K):
    lex, lm = small_lexicon(cpu.SCORES), cpu.language(3, "eighths" if weights == "random" else "integers")
    T, B = 24, 5
    x, tr, il = _case(T, B, 14, dtype, integer=weights == "integers")
    il[1], il[2] = 0, 1
    assert il[0] == T
    seen = {}
    turn = {1: 0, 3: 1, 8: 2, ALL: 3}[K]
    names = ("ones", "whole", "1-7-0-16", "ragged")
    for theta in (INF, 2.0, 0.0):
        for W, P in cpu.WP:
            name = names[turn % 4]                                   # (the four chunkings take turns over thresholds and windows)
            turn += 1
            what = "K=%d theta=%s W=%d P=%d %s" % (K, theta, W, P, name)
            s = Both(tr, lex, lm, B, W, P, K, theta, grow=T + 7 * 30)
            s.check((2,), what + " before the first frame")
            for i, (chunk, n) in enumerate(_chunks(name, x, il)):
                few = name == "ones" and i % 4 and i < T - 1         # (frame by frame: the four sizes at every fourth position)
                s.advance(chunk, n)
                s.check((K + 5,) if few else sorted({1, 2, K, K + 5}), "%s call %d" % (what, i), seen=seen)
    # the regimes, from the restatement: padding rows, rows behind convergence commits, and (beyond K = 1) lists and forced commits
    assert seen["padded"] > 0 and seen["clear"] > 0 and (K == 1 or (seen["rows"] > 1 and seen["forced"] > 0))
    assert weights != "integers" or K == 1 or seen["tied"] > 0


# ---------------------------------------------------------------------------------------------------------------- 2. the sort
@pytest.mark.parametrize("K", [63, 64, 65])
def test_63_64_65_candidates(K):
    lex, lm = every_node_ends_a_word(10, 0)
    x, tr = torch.randn(5, 2, 10, generator=torch.Generator().manual_seed(37)) * 0.25, torch.zeros(10, 10)
    s = Both(tr, lex, lm, 2, 8, 8, K, grow=5)
    s.advance(x)
    for final in (False, True):
        want = word_window_nbest(s.ref, K + 1, final)
        assert (want["num_hyps"] == K).all()                         # the regime: exactly K candidates
    s.check((K, K + 1), "K=%d" % K)
    s.check((K + 1,), "K=%d, no alignments" % K, align=False)


def test_more_than_1024_candidates_strip_the_lanes_and_the_workgroup():
    lex, lm = every_node_ends_a_word(40, 261)
    x, tr = torch.randn(5, 2, 40, generator=torch.Generator().manual_seed(33)) * 0.25, torch.zeros(40, 40)
    s = Both(tr, lex, lm, 2, 8, 8, 1200, grow=5)
    s.advance(x, torch.tensor([5, 4]))
    for final in (False, True):
        assert (word_window_nbest(s.ref, 1200, final)["num_hyps"] > 1024).all()     # the regime
    s.check((1200,), "wide")


# ---------------------------------------------------------------------------------------------------------------- 3. the collapse
def _flat(T, B, dtype, seed=64):
    """Flat emissions under a wide beam: the hypotheses stay apart, nothing converges."""
    x, tr, _ = _case(T, B, seed, dtype)
    return x * 0.05, tr * 0.05


@DTYPES
@pytest.mark.parametrize("W", [64, 65, 66])
def test_tails_below_at_and_above_a_block_of_the_collapse(W, dtype):
    """P = 1 and hypotheses that never converge: W - 1 frames -- 63, 64, 65 -- is the longest tail a call can meet.  Among the
    rows are words whose separator stands in column 0 (behind the carried label) and, at W = 66, in column 64 (behind the label
    a block of the collapse ended with)."""
    lex, lm = small_lexicon(cpu.SCORES), cpu.language(2, "eighths")
    T, B, nb = W + 6, 2, 40
    x, tr = _flat(T, B, dtype)
    s = Both(tr, lex, lm, B, W, 1, ALL)
    col0 = col64 = 0
    for t0, t1 in ((0, W - 1), (W - 1, W), (W, W + 3), (W + 3, T)):
        s.advance(x[t0:t1])
        assert all(v.pos - v.base == W - 1 for v in s.ref.slots)     # the regime, from the restatement
        want = s.check((nb,), "W=%d after frame %d" % (W, t1))
        assert (want["num_hyps"] >= 30).all()
        p = want["path"]
        col0 += sum(int(rec["sep0"]) for recs in want["records"] for rec in recs)
        if W == 66:
            col64 += int(((p[:, :, 64] == SEP) & (p[:, :, 63] != SEP)).sum())
    assert col0 > 0 and (W != 66 or col64 > 0)
    s.check((3,), "W=%d, no alignments" % W, align=False)


# ---------------------------------------------------------------------------------------------------------------- 4. 5. the ring, the commits
@DTYPES
@pytest.mark.parametrize("WP", [(8, 2), (16, 4), (5, 5)])
def test_tails_through_a_ring_that_wraps_and_the_commit_regimes(WP, dtype):
    """pos far beyond W (dozens of wraps where P < W); base == pos with K = 1 and P = 1, where a final word stands behind an
    empty tail; forced commits on flat emissions with every pair kept."""
    W, P = WP
    lex, lm = small_lexicon(cpu.SCORES), cpu.language(3, "eighths")
    T, B, nb = 160, 2, 6
    cuts = [0, 1, 7, 7, 16, 24, 29, 30, 47, 64, 101, 160]
    seen = {}
    x, tr, _ = _case(T, B, 71, dtype)
    x[:, :, SEP] += 1.0                                              # (short words: many separator edges)
    s = Both(tr, lex, lm, B, W, P, 8, grow=T)
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        s.advance(x[t0:t1])
        s.check((nb,), "W=%d P=%d after frame %d" % (W, P, t1), seen=seen)
    assert seen["rows"] > 1 and seen["clear"] > 0 and (P == W or seen["wrapped"] > 0) and s.ref.slots[0].pos > 9 * W
    one = Both(tr, lex, lm, B, W, 1, 1, grow=T)                      # every frame is committed at once
    words = 0
    for t0, t1 in zip(cuts[:6], cuts[1:7]):
        one.advance(x[t0:t1])
        assert all(v.base == v.pos for v in one.ref.slots)           # the regime
        want = one.check((1, 3), "K=1 after frame %d" % t1)
        words += int((want["word_lengths"][:, 0] == 1).sum())
    assert words > 0                                                 # a final word behind an empty tail
    xf, trf = _flat(48, B, dtype)
    f = Both(trf, lex, lm, B, W, P, ALL)
    for t0, t1 in ((0, 5), (5, 6), (6, 17), (17, 48)):
        f.advance(xf[t0:t1])
        f.check((1, 7, ALL), "flat W=%d P=%d after frame %d" % (W, P, t1), seen=seen)
    assert all(v.status & 1 for v in f.ref.slots) and seen["forced"] > 0


# ---------------------------------------------------------------------------------------------------------------- 6. look-ahead
@DTYPES
@pytest.mark.parametrize("la", [1, 2])
def test_look_ahead_through_the_public_method(la, dtype):
    A = _asg()
    lex, lm = small_lexicon(cpu.SCORES), cpu.language(3, "eighths")
    T, B = 24, 3
    x, tr, il = _case(T, B, 21 + la, dtype)
    il[1] = 9
    look = A.WordLookahead(lex, lm, la)
    seen = {}
    for K, theta, (W, P) in ((3, 2.0, (8, 2)), (8, INF, (16, 4)), (ALL, INF, (5, 5))):
        s = Both(tr, lex, lm, B, W, P, K, theta, la=la)
        for chunk, n in _chunks("1-7-0-16", x, il):
            s.advance(chunk, n)
            s.check(sorted({1, 2, K, K + 5}), "la=%d K=%d W=%d P=%d" % (la, K, W, P), seen=seen)
        for nb in (1, K + 5):
            got = _nb(s.dev, nb, True)
            shot = A.beam_decode_words_nbest(x.to(DEV), tr.to(DEV), lex, lm, il.to(DEV), K, nb, theta, LW, WS, TS,
                                             lookahead=look)
            assert got["scores"].tobytes() == shot.scores.cpu().numpy().tobytes(), (K, nb)
            assert got["num_hyps"].tobytes() == shot.num_hyps.cpu().numpy().tobytes(), (K, nb)
    assert seen["rows"] > 1 and seen["clear"] > 0
    plain = A.BeamWordStream(tr.to(DEV), lex, lm, B, T, 4, dtype=dtype, lookahead=look)
    with pytest.raises(NotImplementedError):                         # the growing look-ahead stream's public method is as it was
        plain.result_nbest(2)


# ---------------------------------------------------------------------------------------------------------------- 7. 8. the state
@DTYPES
def test_a_beam_that_empties_inside_a_chunk_and_a_masked_reset(dtype):
    lex, lm = small_lexicon(cpu.SCORES), cpu.language(2, "eighths")
    x, tr, _ = _case(14, 3, 65, dtype)
    x[9, 0] = -INF                                                   # nothing survives frame 9 in slot 0
    il = torch.tensor([14, 8, 0])
    s = Both(tr, lex, lm, 3, 4, 2, 3)
    for t0, t1 in ((0, 6), (6, 12), (12, 14)):
        s.advance(x[t0:t1], (il - t0).clamp(0, t1 - t0))
        for align in (True, False):
            want = s.check((1, 3, 8), "after frame %d" % t1, align=align)
    assert want["status"][0] & 2 and want["num_hyps"].tolist()[0::2] == [0, 0] and want["num_hyps"][1] > 0      # the regimes
    assert want["frames"].tolist() == [14, 8, 0]
    s.reset(torch.tensor([True, False, False]))
    want = s.check((3,), "after the masked reset")
    assert want["frames"].tolist() == [0, 8, 0] and want["num_hyps"][0] == 0 and want["num_hyps"][1] > 0
    x2, _, _ = _case(10, 3, 66, dtype)
    for t0, t1 in ((0, 4), (4, 10)):
        s.advance(x2[t0:t1], torch.tensor([t1 - t0, 0, t1 - t0]))
        want = s.check((3,), "the new utterance after frame %d" % t1)
    assert want["frames"].tolist() == [10, 8, 10] and (want["num_hyps"] > 0).all()


@pytest.mark.parametrize("final", [False, True])
def test_capture_of_result_nbest_with_three_replays(final):
    """Behind a captured advance the first time round and eager ones after."""
    lex, lm = small_lexicon(cpu.SCORES), cpu.language(3, "eighths")
    Tc, B, K = 4, 3, 12
    x, tr, _ = _case(3 * Tc, B, 53, torch.float32)
    s = Both(tr, lex, lm, B, 6, 2, K, 6.0)
    buf = torch.zeros(Tc, B, 5, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.dev.advance(buf[:0])                                       # warm-ups: no frame, and the scratch of nbest = 3
        s.dev.result_nbest(3, final, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ga, gr = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(ga):
        s.dev.advance(buf)
    with torch.cuda.graph(gr):
        out = s.dev.result_nbest(3, final, True)
    s.dev.reset()                                                    # (the captures themselves ran nothing)
    for c in range(3):
        chunk = x[c * Tc:(c + 1) * Tc]
        if c == 0:
            buf.copy_(chunk)
            ga.replay()
        else:
            s.dev.advance(chunk.to(DEV))
        s.ref.advance(chunk.numpy())
        gr.replay()
        torch.cuda.synchronize()
        want = word_window_nbest(s.ref, 3, final)
        assert (want["num_hyps"] > 1).all()
        _same({n: o.cpu().numpy() for n, o in zip(NAMES, out)}, want, "replay %d final=%s" % (c, final))


# ---------------------------------------------------------------------------------------------------------------- 9. the other routes
def test_two_runs_give_identical_bits_and_the_older_routes_are_unchanged():
    A = _asg()
    lex, lm = small_lexicon(cpu.SCORES), cpu.language(3, "eighths")
    T, B = 16, 4
    x, tr, il = _case(T, B, 61, torch.float32)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    args = (4.0, LW, WS, TS)

    def older(w, g):
        outs = list(w.result(True)) + list(w.result(False)) + list(g.result_nbest(3, True, True)) + list(g.result_nbest(3, False))
        outs += list(A.beam_decode_words(xd, trd, lex, lm, ild, 6, *args))
        outs += list(A.beam_decode_words_nbest(xd, trd, lex, lm, ild, 6, 3, *args, return_alignments=True))
        outs += list(A.beam_decode_words_nbest_confidence(xd, trd, lex, lm, ild, 6, 3, *args, 1, True))
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs if o is not None]
    runs = []
    for _ in range(2):
        w = A.BeamWordWindowStream(trd, lex, lm, B, 8, 2, 6, *args)
        g = A.BeamWordStream(trd, lex, lm, B, T, 6, *args)
        for t0, t1 in ((0, 7), (7, 16)):
            nn = (il - t0).clamp(0, t1 - t0).to(DEV)
            w.advance(xd[t0:t1], nn)
            g.advance(xd[t0:t1], nn)
        before = older(w, g)
        mine = [o for final in (False, True) for align in (False, True) for o in _nb(w, 4, final, align).values()
                if o is not None]
        after = older(w, g)
        assert len(before) == len(after) and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        runs.append(mine)
    assert len(runs[0]) == len(runs[1]) and all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    with pytest.raises(ValueError):
        w.result_nbest(0)
    with pytest.raises(RuntimeError, match="unsupported|limit|support"):
        w.result_nbest(8193)
