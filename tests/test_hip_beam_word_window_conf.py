"""GPU tests (-m gpu) of the lattice-keeping word window stream (`torch_asg_amd.BeamWordWindowStream(..., keep_lattice=True)`;
csrc/asg_beam_word_conf_window.hip).  Per call: the plain fields BYTE FOR BYTE against a plain
`BeamWordWindowStream` fed the same chunks; frames and padding exactly, confidences under tests/test_hip_beam_conf.py's rule
(float64 rtol = atol = 1e-9, float32 util.assert_close) against the numpy restatement tests/beam_word_window_conf_ref.py; the
committed values BIT FOR BIT against the device's own `BeamWordStream(keep_lattice=True)`, advanced frame by frame, wherever the
restatement's status bit 0 was clear at that attempt.  At the end: the same bits frame by frame and in chunks of max_chunk, and
the `final=True` tail with the commits against the device's `beam_decode_words_confidence`.  Inputs are
tests/test_beam_word_window_cpu.py's `word_case` at T = 40, W = 8, P = 2, where RW = 10 .. 18 + tol wraps several times."""
import numpy as np
import pytest
import torch

from beam_word_window_conf_ref import BeamWordWindowConfRef
from test_beam_word_window_cpu import LW, TS, WS, word_case
from util import assert_close

pytestmark = pytest.mark.gpu
DEV, INF, T, W, P = "cuda", float("inf"), 40, 8, 2
NP = {torch.float32: np.float32, torch.float64: np.float64}
PLAIN = ("path", "states", "lm_states", "tokens", "token_lengths", "words", "word_lengths", "frames")
# K = 4: seeds at which the restatement commits words both in convergence-only attempts and in attempts with a forced commit;
# K = 65 (a kept set wider than a wavefront): every word of this lexicon comes with a forced commit.
SEEDS = {4: (0, 2, 4), 65: (4,)}


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _look(lex, lm, order):
    return None if order is None else _asg().WordLookahead(lex, lm, order)


def _window(tr, lex, lm, B, K, tol=0, C=None, order=None, theta=INF, keep=True):
    kw = dict(keep_lattice=True, frame_tolerance=tol, max_chunk=C) if keep else {}
    return _asg().BeamWordWindowStream(tr.to(DEV), lex, lm, B, W, P, K, theta, LW, WS, TS, dtype=tr.dtype,
                                       lookahead=_look(lex, lm, order), **kw)


def _ref(tr, lex, lm, B, K, tol=0, C=None, order=None, theta=INF):
    return BeamWordWindowConfRef(tr.numpy(), lex, lm, B, W, P, K, theta, LW, WS, TS, NP[tr.dtype], tol, C, order)


def _close(got, want, dtype, what):
    assert not np.isnan(got).any(), what
    if dtype == torch.float64:
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9), what
    else:
        assert_close(got, want, what=what)


def _feed(s, plain, ref, x, il, C, what):
    """Feed x in chunks of C frames to the lattice-keeping stream, a plain stream (or None) and the restatement (or None), with
    the per-call checks.  -> per slot the concatenated (frames, confidence bytes)."""
    B, dtype = s.batch_size, x.dtype
    wfs, cfs = [[] for _ in range(B)], [b"" for _ in range(B)]
    for a in range(0, x.shape[0], C):
        c, n = x[a:a + C], (il - a).clamp(0, min(C, x.shape[0] - a))
        out = s.advance(c.to(DEV), n.to(DEV))
        assert type(out).__name__ == "BeamWordWindowConfCommit" and out._fields[:8] == PLAIN, what
        got = {k: getattr(out, k).cpu().numpy() for k in out._fields}
        if plain is not None:                                    # property 1
            assert [got[k].tobytes() for k in PLAIN] == [t.cpu().numpy().tobytes() for t in plain.advance(c.to(DEV), n.to(DEV))], \
                (what, a)
        wf, cf, wl = got["word_frames"], got["word_confidences"], got["word_lengths"]
        assert wf.dtype == np.int64 and cf.dtype == NP[dtype] and wf.shape == cf.shape == got["path"].shape, (what, a)
        behind = np.arange(wf.shape[1])[None, :] >= wl[:, None]
        assert (wf[behind] == -1).all() and (cf[behind] == 0).all() and (wf[~behind] >= 1).all(), (what, a)
        if ref is not None:
            want = ref.advance(c.numpy(), n.numpy())
            for k, v in zip(("path", "states", "lm_states", "tokens", "words", "frames", "token_lengths", "word_lengths"), want):
                assert np.array_equal(got[k], v), (what, a, k)
            assert np.array_equal(wf, want[8]), (what, a)        # frames and padding exact
            _close(cf, want[9], dtype, (what, a))
        for b in range(B):
            wfs[b] += wf[b, :wl[b]].tolist()
            cfs[b] += cf[b, :wl[b]].tobytes()
    return wfs, cfs


def _grown(x, tr, lex, lm, K, tol, order):
    """The device's growing lattice stream fed frame by frame and asked, with final=False, at every multiple of P."""
    s = _asg().BeamWordStream(tr.to(DEV), lex, lm, 1, T, K, INF, LW, WS, TS, dtype=tr.dtype,
                              lookahead=_look(lex, lm, order), keep_lattice=True)
    at = {}
    for t in range(T):
        s.advance(x[t:t + 1].to(DEV))
        if (t + 1) % P == 0:
            r = s.result_confidence(tol, final=False)
            at[t + 1] = [v.cpu().numpy()[0] for v in (r.word_frames, r.word_confidences, r.word_lengths)]
    return at


def _case(seed, K, tol, C, dtype, order):
    """One seed through the whole body -> (words compared bit for bit with the growing stream, words of attempts with a forced
    commit, tail words compared bit for bit with the one-shot call)."""
    lex, lm, x, tr, il = word_case(seed, T, NP[dtype])
    x, tr, il = torch.from_numpy(x), torch.from_numpy(tr), torch.from_numpy(il)
    what = "seed %d K %d tol %d C %d order %s" % (seed, K, tol, C, order)
    s, ref = _window(tr, lex, lm, 1, K, tol, C, order), _ref(tr, lex, lm, 1, K, tol, C, order)
    plain = _window(tr, lex, lm, 1, K, order=order, keep=False)
    wfs, cfs = _feed(s, plain, ref, x, il, C, what)
    for final in (False, True):                                  # property 1 for the calls that only read the state
        for a, b in ((s.result(final), plain.result(final)), (s.result_nbest(3, final, True), plain.result_nbest(3, final, True))):
            assert [t.cpu().numpy().tobytes() for t in a] == [t.cpu().numpy().tobytes() for t in b], (what, final)
    # property 3, from the restatement's own status
    grown, cat, k, clear, forced = _grown(x, tr, lex, lm, K, tol, order), np.frombuffer(cfs[0], NP[dtype]), 0, 0, 0
    for p1, b0, k0, k1, status in ref.ends[0]:
        n = k1 - k0
        if status & 1:
            forced += n
        else:
            gf, gc, gl = grown[p1]
            assert gl >= k + n and wfs[0][k:k + n] == gf[k:k + n].tolist(), (what, p1)
            assert cat[k:k + n].tobytes() == np.ascontiguousarray(gc[k:k + n]).tobytes(), (what, p1)
            clear += n
        k += n
    assert k == len(wfs[0]), what
    # property 2: frame by frame, the same bits
    one = _window(tr, lex, lm, 1, K, tol, C, order)
    assert _feed(one, None, None, x, il, 1, what + " by frame") == (wfs, cfs), what
    # the tail, and property 4 against the one-shot call
    for final in (False, True):
        r, want = s.result_confidence(final), ref.result_confidence(final)
        assert type(r).__name__ == "BeamWordWindowConfidence", what
        h = {n: getattr(r, n).cpu().numpy() for n in r._fields}
        assert [h[n].tobytes() for n in r._fields[:11]] == [t.cpu().numpy().tobytes() for t in s.result(final)], what
        for n in ("path", "tokens", "states", "lm_states", "words", "word_lengths", "word_frames", "frames", "committed", "status"):
            assert np.array_equal(h[n], want[n]), (what, final, n)
        _close(h["word_confidences"], want["word_confidences"], dtype, (what, final))
        _close(h["normalisers"], want["normalisers"], dtype, (what, final))
        assert [getattr(one.result_confidence(final), n).cpu().numpy().tobytes() for n in r._fields] == \
            [h[n].tobytes() for n in r._fields], (what, final)
    tail = 0
    if not h["status"][0] & 1:
        o = _asg().beam_decode_words_confidence(x.to(DEV), tr.to(DEV), lex, lm, il.to(DEV), K, INF, LW, WS, TS, tol,
                                                lookahead=_look(lex, lm, order))
        n, m = len(wfs[0]), int(h["word_lengths"][0])
        assert wfs[0] + h["word_frames"][0, :m].tolist() == o.word_frames[0, :n + m].tolist() and o.word_lengths[0] == n + m, what
        assert h["word_confidences"][0, :m].tobytes() == o.word_confidences[0, n:n + m].cpu().numpy().tobytes(), what
        tail = m
    return clear, forced, tail


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("K", [4, 65])
@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("tol", [0, 3, 64])
def test_grid(tol, C, K, dtype):
    got = [_case(seed, K, tol, C, dtype, None) for seed in SEEDS[K]]
    assert sum(g[1] for g in got) > 0 and (K > 4 or sum(g[0] for g in got) > 0)      # neither comparison is empty


def test_look_ahead():
    got = [_case(seed, 4, 3, 5, torch.float64, 2) for seed in SEEDS[4]]
    assert sum(g[0] for g in got) > 0 and sum(g[1] for g in got) > 0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_the_commits_and_the_final_tail_are_the_one_shot_call(dtype):
    """Property 4 needs a stream that ends with status bit 0 clear: K = 3, seed 5 commits 15 words by convergence alone and
    leaves three in the tail (from the restatement, on the CPU)."""
    clear, forced, tail = _case(5, 3, 3, 5, dtype, None)
    assert clear > 0 and forced == 0 and tail > 0


def test_empty_chunks_a_masked_reset_and_an_emptied_beam():
    """Two slots (seeds 0 and 4 under seed 0's transitions); calls of no frames between the chunks; slot 0 is reset behind frame
    20 and starts seed 2's frames; slot 1 gets -inf emissions from frame 30 on, which empty its beam under a finite threshold."""
    lex, lm, x0, tr, _ = word_case(0, T, np.float64)
    x = np.concatenate([x0, word_case(4, T, np.float64)[2]], 1)
    x[20:, 0] = word_case(2, T, np.float64)[2][:20, 0]
    x[30:, 1] = -np.inf
    x, tr, il = torch.from_numpy(x), torch.from_numpy(tr), torch.tensor([T, T])
    s, plain, ref = (_window(tr, lex, lm, 2, 4, 3, 5, theta=50.0), _window(tr, lex, lm, 2, 4, theta=50.0, keep=False),
                     _ref(tr, lex, lm, 2, 4, 3, 5, theta=50.0))
    words = 0
    for a in (0, 20):
        wfs, _ = _feed(s, plain, ref, x[a:a + 20], il - a, 5, "from %d" % a)
        words += len(wfs[0]) + len(wfs[1])
        e = s.advance(x[:0].to(DEV))                             # Tc = 0: every element written, nothing committed
        assert e.word_frames.shape == (2, W) and (e.word_frames == -1).all() and (e.word_confidences == 0).all()
        assert [t.cpu().numpy().tobytes() for t in e[:8]] == [t.cpu().numpy().tobytes() for t in plain.advance(x[:0].to(DEV))]
        ref.advance(x[:0].numpy())
        if a == 0:
            mask = torch.tensor([1, 0])
            s.reset(mask), plain.reset(mask), ref.reset(mask.numpy())
    r, want = s.result_confidence(True), ref.result_confidence(True)
    assert words > 0 and want["status"][1] & 2 and r.status.cpu().tolist() == want["status"].tolist()
    assert np.array_equal(r.word_frames.cpu().numpy(), want["word_frames"])
    _close(r.word_confidences.cpu().numpy(), want["word_confidences"], torch.float64, "tail")


def test_advance_is_captured_and_replays():
    lex, lm, x, tr, _ = word_case(4, T, np.float32)
    x, tr = torch.from_numpy(x), torch.from_numpy(tr)
    eager = _window(tr, lex, lm, 1, 4, 3, 5)
    want = [[t.cpu().numpy().tobytes() for t in eager.advance(x[a:a + 5].to(DEV))] for a in range(0, T, 5)]
    s, buf = _window(tr, lex, lm, 1, 4, 3, 5), x[:5].to(DEV).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = s.advance(buf)
    torch.cuda.current_stream().wait_stream(side)
    for rep in range(2):
        s.reset()
        for i, a in enumerate(range(0, T, 5)):
            buf.copy_(x[a:a + 5])
            g.replay()
            assert [t.cpu().numpy().tobytes() for t in out] == want[i], (rep, a)


def test_result_confidence_needs_the_lattice():
    lex, lm, _, tr, _ = word_case(0, T, np.float32)
    with pytest.raises(RuntimeError, match="keep_lattice"):
        _window(torch.from_numpy(tr), lex, lm, 1, 4, keep=False).result_confidence()
