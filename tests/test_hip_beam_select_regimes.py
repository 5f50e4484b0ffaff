"""GPU tests (-m gpu) of the per-frame select that every beam feature compiles -- the end of `beam_frame`
(csrc/asg_beam_frame.h: the token-graph decoder, its n-best, BeamStream, BeamWindowStream, the beam-pruned loss) and its copy in
`beam_word_frame` (csrc/asg_beam_word_frame.h: the lexicon + word-LM family) -- at the sizes where it changes shape:

  1. the key select at widths rem = 0, 3, 8, 9 (digits 8 | 1), 12, 16, 17, 20, kBits (candidates on both sides of zero) and, in
     float64, 40 -- digits that random data never reaches -- through every exit: rem == 0 with at most K and with more than K
     equal keys, everything that passes taken whole on the first pass (also at rem > 8), the K-th key found with its ties all
     taken, and the tie select; beams below, at and above the count that passes; thresholds infinity, 0 and a finite one that
     cuts inside the band;
  2. the tie select over q at 8, 9 (8 | 1), 16 (8 | 8), 17 (8 | 8 | 1) and 18 (8 | 8 | 2) bits of q, with cuts decided in every
     digit, in frames of more than 1024 candidates and at a beam above 1024;
  3. beams around every halving of the lanes per state (64 -> 1) with rows of 69 arcs, longer than a wavefront;
  4. K = 8192 with the transitions inside LDS and in global memory: N = 153 | 154 (float32), 87 | 88 (float64);
  5. the key widths of 1. through the other copy of the select: a lexicon of one-token words, lm_weight = word_score = 0.

The inputs are those of tests/beam_select_cases.py.  Every case first repeats its precondition from the restatement's own `info`
and the restated launch arithmetic (tests/test_beam_select_regimes_cpu.py holds the same assertions, and that a subtly wrong
select changes the outputs), then compares the device with the restatements bit for bit in float32 and float64: the decoder
with tests/beam_decode_ref.py, the n-best lists with tests/beam_nbest_ref.py (row 0 is the decoder), BeamStream fed one frame at
a time and in uneven chunks (the one-shot bits at the end), BeamWindowStream with tests/beam_window_ref.py after every call.
The beam-pruned loss is compared with tests/beam_loss_ref.py by the rule of tests/test_hip_beam_loss.py, unchanged: its sets are
the select's, so a wrong set shows in Z.

Left out: q of 19 to 24 bits (no digit that 18 bits do not have) and of 25 bits and more (a fourth digit needs 2^24 product
states); +inf emissions (max - threshold is then undefined); the n-best kernels' own LDS layout; the pair widths
of the word family, which tests/test_hip_beam_word_regimes.py pins."""
import numpy as np
import pytest
import torch

import beam_select_cases as C
import test_hip_beam_decode as one_shot
import test_hip_beam_nbest as nbest
import test_hip_beam_stream as stream
import test_hip_beam_window as window
import test_hip_beam_word as word_one_shot
import test_hip_beam_word_stream as word_stream
from beam_decode_ref import beam_decode_ref, q_bits
from beam_loss_cases import _compare, _full, _ref
from beam_window_ref import BeamWindowRef
from test_beam_select_regimes_cpu import (ALL_KEY_CASES, KEY_IDS, WIDTH_BITES, assert_key_regime, assert_width_regime, key_runs,
                                          lanes_regime, width_regime)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
NAMES = ("scores", "path", "tokens", "token_lengths", "states")


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _t(*arrays):
    return tuple(torch.from_numpy(np.array(a)) for a in arrays)


def _decode(graph, x, tr, il, K, theta, what, info=None, sizes=None):
    """beam_decode_graph against the restatement, every output bit for bit -> the restatement's five arrays."""
    got = one_shot._gpu(x, tr, graph, il, K, theta)
    want = beam_decode_ref(x.numpy(), tr.numpy(), graph.next, graph.weight, graph.final, graph.start, il.numpy(), K, theta,
                           info=info, sizes=sizes)
    for name, g, w in zip(NAMES, got, want):
        assert g.numpy().dtype == w.dtype and g.numpy().tobytes() == w.tobytes(), "%s %s K=%d theta=%s" % (name, what, K, theta)
    return want


def _nbest(graph, x, tr, il, K, theta, one, what):
    got, _ = nbest._check(x, tr, graph, il, K, min(K, 4), theta, what=what)
    rows = (got.scores, got.path, got.tokens, got.token_lengths, got.states)
    for name, u, v in zip(NAMES, rows, one):
        assert u[:, 0].numpy().tobytes() == v.tobytes(), "row 0 is the decoder: %s %s" % (name, what)


def _streams(graph, x, tr, il, K, theta, one, what, chunkings=None):
    """BeamStream fed one frame at a time and in uneven chunks: the one-shot bits at the end."""
    T, B = x.shape[0], x.shape[1]
    xd = x.to(DEV)
    for cuts in chunkings or (list(range(T + 1)), [0, 1, 1, T - 1, T]):
        s = _asg().BeamStream(tr.to(DEV), graph, B, T, K, theta, 1.0, 0.0, dtype=tr.dtype)
        stream._feed(s, xd, il, cuts)
        stream._same_as_one_shot(stream._res(s), one, T, "%s chunks %s" % (what, cuts))


def _windows(graph, x, tr, il, K, theta, one, what):
    """BeamWindowStream against its restatement after every call; the search is the one-shot search."""
    T, B = x.shape[0], x.shape[1]
    for W, P, cuts in ((2, 1, list(range(T + 1))), (4, 2, [0, 1, 1, T - 1, T])):
        s = _asg().BeamWindowStream(tr.to(DEV), graph, B, W, P, K, theta, 1.0, 0.0, dtype=tr.dtype)
        ref = BeamWindowRef(tr.numpy(), graph.next, graph.weight, graph.final, graph.start, B, W, P, K, theta, 1.0, 0.0,
                            stream.NP[tr.dtype])
        window._feed(s, ref, x, il, cuts, "%s W=%d P=%d" % (what, W, P), results=True)
        assert ref.result(True)[0].tobytes() == one[0].tobytes(), what


def _loss(graph, x, tr, il, K, theta, what):
    """beam_graph_full_score and its gradients by the rule of tests/test_hip_beam_loss.py -> the restatement's Z."""
    gs = torch.linspace(1.0, -0.5, x.shape[1], dtype=torch.float64)
    got, want = _full(x, tr, graph, il, K, theta, gs=gs), _ref(x, tr, graph, il, K, theta, gs=gs)
    _compare(got, want, x.dtype, what)
    return want[0]


def _every_entry_point(graph, x, tr, il, K, theta, what, info=None, all_five=True):
    """The decoder, its n-best and BeamStream; with `all_five` also BeamWindowStream and the loss."""
    one = _decode(graph, x, tr, il, K, theta, what, info=info)
    _nbest(graph, x, tr, il, K, theta, one, what)
    _streams(graph, x, tr, il, K, theta, one, what)
    if all_five:
        _windows(graph, x, tr, il, K, theta, one, what)
        Z = _loss(graph, x, tr, il, K, theta, what)
        assert (np.isfinite(Z) == np.isfinite(one[0])).all(), what      # a finite best path, a finite Z
    return one


# ---------------------------------------------------------------------------------------------------------------- 1. key widths
@pytest.mark.parametrize("name,dtype", ALL_KEY_CASES, ids=KEY_IDS)
def test_key_widths_and_exits_in_every_entry_point(name, dtype):
    """The frame `name` (tests/beam_select_cases.py::KEY_FRAMES: the width of the key select and the exit it takes at K = 7)
    behind another frame, as the first frame and behind a second one, under the three thresholds and the beams below, at
    and above the count that passes each: the decoder, its n-best, both streams and the loss."""
    x, tr, il = _t(*C.key_case(name, dtype)[:3])
    graph = C.one_state()
    seen = []
    for theta, K in key_runs(name, dtype):
        info = {}
        what = "%s %s K=%d theta=%s" % (name, dtype.__name__, K, theta)
        one = _every_entry_point(graph, x, tr, il, K, theta, what, info=info)
        r = assert_key_regime(name, dtype, theta, K, info)
        seen.append((theta if theta in (INF, 0) else "finite", K, r["rem"], r["exit"]))
        assert (one[1][0, 2] == C.WITNESS) and np.isfinite(one[0]).all()
    print("%s %s: (threshold, K, rem, exit) %s" % (name, dtype.__name__, seen))
    assert (INF, C.K_KEY, C.key_rem(name, dtype), C.KEY_FRAMES[name][1]) in seen


# -------------------------------------------------------------------------------------------------------------- 2. state widths
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("bits", sorted(C.WIDTHS))
def test_state_widths_in_every_entry_point(bits, dtype):
    """q of 8, 9, 16, 17 and 18 bits: the tie select walks 1, 2 (8 | 1), 2 (8 | 8), 3 (8 | 8 | 1) and 3 (8 | 8 | 2) digits, and
    the runs cut ties in every one of them; from 16 bits on also in frames of more than 1024 candidates and at K = 2000.  The
    window stream and the loss run at the infinite threshold and K <= 200 (their restatements over 66 000 and more states take
    the longest)."""
    graph = C.width_graph(bits)
    x, tr, il = _t(*C.width_inputs(bits, dtype))
    total = {}
    for K in C.width_beams(bits):
        for theta in C.WIDTH_THETAS:
            info = {}
            what = "q of %d bits %s K=%d theta=%s" % (bits, dtype.__name__, K, theta)
            _every_entry_point(graph, x, tr, il, K, theta, what, info=info, all_five=theta == INF and K <= 200)
            assert q_bits(info["Q"]) == bits
            for k, v in width_regime(info, K).items():
                total[k] = total.get(k, 0) + v
    print("q of %d bits %s: Q %d; cuts %s (wrong selects that change the outputs: %s)"
          % (bits, dtype.__name__, info["Q"], total, WIDTH_BITES[bits]))
    assert graph.compile_host(dtype)["Q"] == info["Q"]
    assert_width_regime(bits, total)


# --------------------------------------------------------------------------------------------------------------------- 3. lanes
@pytest.mark.parametrize("K", C.LANE_BEAMS)
def test_lanes_per_state_bit_for_bit(K):
    """A frame with a successor keeps exactly K states, each with a row of 69 arcs: the G = beam_lanes_per_state(K) <= 64
    lanes of a state stride its row more than once on either side of every halving of G."""
    graph = C.lane_graph()
    x, tr, il = _t(*C.lane_inputs())
    sizes = []
    one = _decode(graph, x, tr, il, K, INF, "lanes", sizes=sizes)
    G, row = lanes_regime(K, sizes)
    print("K %d: G %d, rows of %d arcs" % (K, G, row))
    assert row == 69 > 64 >= G and max(max(s) for s in sizes) == K
    _streams(graph, x, tr, il, K, INF, one, "lanes", chunkings=([0, 1, 3, 4],))


# ----------------------------------------------------------------------------------------------------------------------- 4. LDS
@pytest.mark.parametrize("side", ["transitions-in-lds", "transitions-in-global-memory"])
@pytest.mark.parametrize("elem,K,N0", C.LDS_STEPS, ids=["f32", "f64"])
def test_both_transition_layouts_at_the_largest_beam(elem, K, N0, side):
    """4096 + K (e + 4) + 8 + N N e against 160 KiB at K = 8192 (kBeamMaxK), where the set alone takes 64 or 96 KiB:
    N = 153 | 154 in float32, 87 | 88 in float64.  The automaton has more than 8192 product states, so K is not clamped, and
    the last frame fills the beam."""
    dtype = np.float32 if elem == 4 else np.float64
    N = N0 + (side != "transitions-in-lds")
    assert C.transitions_in_lds(K, N, elem) == (N == N0) and C.transitions_in_lds(K, N0, elem)
    assert not C.transitions_in_lds(K, N0 + 1, elem) and K == C.MAX_K
    graph = C.lds_graph(N)
    assert graph.compile_host(dtype)["Q"] > K
    x, tr, il = _t(*C.lds_inputs(N, dtype))
    sizes = []
    one = _decode(graph, x, tr, il, K, INF, "N=%d" % N, sizes=sizes)
    assert sizes[0][-1] == K and np.isfinite(one[0]).all()
    _streams(graph, x, tr, il, K, INF, one, "N=%d" % N, chunkings=([0, 1, 3],))


# ------------------------------------------------------------------------------------------------------------- 5. the word copy
@pytest.mark.parametrize("name,dtype", ALL_KEY_CASES, ids=KEY_IDS)
def test_key_widths_through_the_word_copy_of_the_select(name, dtype):
    """One-token words, lm_weight = word_score = 0: the frame behind a separator has the candidates of the one-state
    automaton, so the word family's copy of the select sees the same widths and exits (asserted from the word restatement's
    own record).  beam_decode_words, and BeamWordStream fed in uneven chunks."""
    lex, lm = C.word_case()
    x, tr, il = _t(*C.word_key_case(name, dtype)[:3])
    xg, trg, ilg, _ = C.key_case(name, dtype)
    T, B = x.shape[0], x.shape[1]
    W0 = (0.0, 0.0, 0.0)
    for theta, K in key_runs(name, dtype):
        what = "%s %s K=%d theta=%s" % (name, dtype.__name__, K, theta)
        info, winfo = {}, {}
        beam_decode_ref(xg, trg, C.one_state().next, C.one_state().weight, C.one_state().final, 0, ilg, K, theta, info=info)
        r = assert_key_regime(name, dtype, theta, K, info)
        one = word_one_shot._check(x, tr, lex, lm, il, K, theta, *W0, info=winfo, what=what)
        for rec in (winfo["select"][0][2], winfo["select"][1][0]):
            assert all(rec[k] == r[k] for k in ("n", "passing", "rem", "exit")), what
        assert np.isfinite(one["scores"]).all()
        cuts = [0, 1, 1, T - 1, T]
        s = word_stream.Both(tr, lex, lm, B, T, K, theta, *W0)
        s.feed(x, il, cuts, check="%s chunks %s" % (what, cuts))
        word_stream._same_as_one_shot(s.check("%s chunks %s" % (what, cuts))[True], one, T, what)
