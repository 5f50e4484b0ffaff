"""GPU tests (-m gpu) of the n-best lists of the word-LM beam search WITH LM LOOK-AHEAD (`beam_decode_words_nbest(...,
lookahead=)`, `BeamWordStream._result_nbest` of a look-ahead stream, csrc/asg_beam_word_nbest.hip with the LA flag behind
csrc/asg_beam_word_la.hip with the FIN flag): the bytes of every output against the test-side numpy restatement
(tests/beam_word_la_nbest_ref.py, pinned on the CPU by tests/test_beam_word_la_nbest_cpu.py).  Every case first asserts from the
restatement that its input is in the regime it names; then the four required properties on the device, capture, determinism,
grouping, the stream and the neighbours."""
import numpy as np
import pytest
import torch

from beam_word_cases import arpa_lm, eighths, small_lexicon
from beam_word_la_nbest_ref import BeamWordLaNbestStreamRef, beam_word_la_nbest_ref
from beam_word_nbest_cases import split_bound
from beam_word_nbest_ref import NAMES
from test_beam_word_la_cpu import hand_case
from test_hip_beam_word import ties_case
from test_hip_beam_word_nbest import ALIGN, ONE_BEST, STREAM_NAMES, _first, _np, _normal, _same, every_node_ends_a_word, grid_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
ALL = 1024                                                 # more than every pair of the small cases
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])


def _asg():
    import torch_asg_amd
    return torch_asg_amd


def _gpu(x, tr, lex, lm, la, il, K, nbest, theta=INF, lw=1.0, ws=0.0, ts=0.0, align=True, **kw):
    out = _asg().beam_decode_words_nbest(x.to(DEV), tr.to(DEV), lex, lm, None if il is None else il.to(DEV), K, nbest, theta, lw, ws,
                                         ts, align, lookahead=la, **kw)
    torch.cuda.synchronize()
    assert all(o.dtype == x.dtype for o in out[:4]) and all(o.dtype == torch.int64 for o in out[4:] if o is not None)
    return _np(out, NAMES)


def _ref(x, tr, lex, lm, la, il, K, nbest, theta=INF, lw=1.0, ws=0.0, ts=0.0, info=None):
    return beam_word_la_nbest_ref(x.numpy(), tr.numpy(), lex, lm, la.order, None if il is None else il.numpy(), K, nbest, theta, lw,
                                  ws, ts, info)


def _check(x, tr, lex, lm, la, il, K, nbest, theta=INF, lw=1.0, ws=0.0, ts=0.0, align=True, info=None, what=""):
    got = _gpu(x, tr, lex, lm, la, il, K, nbest, theta, lw, ws, ts, align)
    want = _ref(x, tr, lex, lm, la, il, K, nbest, theta, lw, ws, ts, info)
    _same(got, want, NAMES, "%s K=%d nbest=%d theta=%s order=%d" % (what, K, nbest, theta, la.order))
    diff, bound, fin = split_bound(want, x.numpy().dtype.type)
    assert (diff[fin] <= bound[fin]).all()
    return got, want


# ---------------------------------------------------------------------------------------------------------------- grid
@DTYPES
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("lm_order", [2, 3], ids=["bigram", "trigram"])
def test_grid_of_beams_thresholds_orders_and_nbest(lm_order, order, dtype):
    A = _asg()
    lex, lm, x, tr, il = grid_case(lm_order, dtype)
    la = A.WordLookahead(lex, lm, order)
    LW, WS, TS = 0.7, -0.4, 0.3
    padded = several = inexact = 0
    for K in (1, 3, 8, ALL):
        for theta in (INF, 2.0):
            info = {}
            want = _ref(x, tr, lex, lm, la, il, K, K + 5, theta, LW, WS, TS, info)
            assert (want["num_cands"] <= K).all() and want["num_cands"][3] == 0
            if K == ALL and theta == INF:
                assert max(max(s) for s in info["sizes"] if s) < ALL
            several += int((want["num_cands"] > 1).sum())
            diff, bound, fin = split_bound(want, x.numpy().dtype.type)
            assert (diff[fin] <= bound[fin]).all()
            inexact += int((diff[fin] > 0).sum())
            # property 1: row 0 is the device's own one-best with the same look-ahead
            one = _np(A.beam_decode_words(x.to(DEV), tr.to(DEV), lex, lm, il.to(DEV), K, theta, LW, WS, TS, lookahead=la), ONE_BEST)
            for nbest in (1, 2, K + 5):
                w = _first(want, nbest)
                padded += int((w["num_hyps"] < nbest).sum())
                for align in (False, True):
                    got = _gpu(x, tr, lex, lm, la, il, K, nbest, theta, LW, WS, TS, align)
                    _same(got, w, NAMES, "grid K=%d nbest=%d theta=%s" % (K, nbest, theta))
                    assert all((got[n] is None) != align for n in ALIGN)
                for n in ONE_BEST:
                    assert got[n][:, 0].tobytes() == one[n].tobytes(), (n, K, theta)
    assert padded > 0 and several > 0 and inexact > 0


# ---------------------------------------------------------------------------------------------------------------- property 4
@DTYPES
@pytest.mark.parametrize("order", [1, 2, 3])
def test_unpruned_and_in_eighths_the_list_is_the_plain_list_bit_for_bit(order, dtype):
    A = _asg()
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = eighths(arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5)))
    la = A.WordLookahead(lex, lm, order)
    g = torch.Generator().manual_seed(41)
    x = (torch.randint(-32, 32, (6, 3, 5), generator=g) / 8.0).to(dtype)
    tr = (torch.randint(-16, 16, (5, 5), generator=g) / 8.0).to(dtype)
    il = torch.tensor([6, 3, 1])
    info = {}
    got, want = _check(x, tr, lex, lm, la, il, ALL, ALL, INF, 1.0, 0.25, 0.125, info=info, what="eighths")
    assert max(max(s) for s in info["sizes"]) < ALL and info["dead"] == 0 and want["num_hyps"][0] > 20
    plain = A.beam_decode_words_nbest(x.to(DEV), tr.to(DEV), lex, lm, il.to(DEV), ALL, ALL, INF, 1.0, 0.25, 0.125, True)
    _same(got, _np(plain, NAMES), NAMES, "against the plain list")
    fin = np.isfinite(got["scores"])
    assert (got["scores"][fin] == (got["emission_scores"] + (got["graph_scores"] + got["lm_scores"]))[fin]).all()      # exact


# ---------------------------------------------------------------------------------------------------------------- ties
@DTYPES
def test_integer_ties_between_ends_are_broken_by_h_then_q(dtype):
    A = _asg()
    lex, lm, x, tr, il = ties_case(dtype)
    tied = same_q = 0
    for order in (1, 2):
        la = A.WordLookahead(lex, lm, order)
        for K in (3, 8, 64):
            for theta in (INF, 1.0):
                _, want = _check(x, tr, lex, lm, la, il, K, K, theta, 1.0, 1.0, 0.0, what="ties")
                for b in range(5):
                    nh = int(want["num_hyps"][b])
                    L = int(il[b])
                    sc = want["scores"][b, :nh]
                    tied += int((sc[1:] == sc[:-1]).sum())
                    ends = [(int(want["lm_states"][b, r, L - 1]), int(want["states"][b, r, L - 1]), int(want["path"][b, r, L - 1]))
                            for r in range(nh)]
                    for r in range(1, nh):
                        if sc[r] == sc[r - 1]:
                            assert ends[r - 1] < ends[r]   # pair order: h, then q (state and label ascend with q)
                    qs = [e[1:] for e in ends]
                    same_q += len(qs) - len(set(qs))
    assert tied > 0 and same_q > 0                         # two candidates on one q with different h among them


# ---------------------------------------------------------------------------------------------------------------- the sort's edges
@pytest.mark.parametrize("K", [63, 64, 65])
def test_63_64_65_candidates(K):
    A = _asg()
    lex, lm = every_node_ends_a_word(10, 0)
    x, tr = _normal(5, 2, 10, 37, torch.float32)
    _, want = _check(x * 0.25, tr * 0.25, lex, lm, A.WordLookahead(lex, lm, 2), None, K, K + 1, INF, 0.5, -0.2, 0.1, what="edge")
    assert (want["num_cands"] == K).all() and (want["num_hyps"] == K).all()


def test_more_than_1024_hypotheses_strip_the_lanes_and_the_workgroup():
    A = _asg()
    lex, lm = every_node_ends_a_word(40, 261)              # N = 40, 300 words
    x, tr = _normal(5, 2, 40, 33, torch.float32)
    info = {}
    _, want = _check(x * 0.25, tr * 0.25, lex, lm, A.WordLookahead(lex, lm, 2), torch.tensor([5, 4]), 1200, 1200, INF, 0.5, -0.2, 0.1,
                     info=info, what="wide")
    assert (want["num_hyps"] > 1024).all() and max(info["sizes"][0]) > 1024


@DTYPES
def test_the_64_frame_steps_of_the_write_loop(dtype):
    A = _asg()
    lex, lm, _, _, _ = grid_case(3, dtype)
    la = A.WordLookahead(lex, lm, 2)
    x, tr = _normal(130, 4, 5, 38, dtype)
    il = torch.tensor([63, 64, 65, 129])
    for align in (True, False):
        _, want = _check(x, tr, lex, lm, la, il, 8, 6, INF, 0.7, -0.4, 0.3, align, what="T=130")
    assert (want["num_hyps"] >= 2).all() and (want["token_lengths"][:, 0] > 8).all() and (want["word_lengths"][:, 0] > 4).all()


@pytest.mark.parametrize("N", [141, 142], ids=["transitions-in-lds", "transitions-in-global-memory"])
def test_both_transition_layouts_of_the_search_behind_the_list(N):
    """float64, K = 8: 4096 + 8 * 16 + N * N * 8 bytes is within the 160 KiB of LDS for N = 141 and beyond them for N = 142: the two
    instantiations of the look-ahead search that leave their last set for the n-best stage."""
    A = _asg()
    K = 8
    assert (4096 + K * 16 + N * N * 8 <= 160 * 1024) == (N == 141)
    lex = A.Lexicon([[3, 7], [3, 100, 5], [N - 2]], N, N - 1)
    lm = arpa_lm(3, 2, 73)
    x, tr = _normal(6, 2, N, 37, torch.float64)
    for t, lab in enumerate([3, 7, N - 1, N - 2, N - 1, 3]):
        x[t, 0, lab] += 6.0
    info = {}
    _, want = _check(x, tr, lex, lm, A.WordLookahead(lex, lm, 2), torch.tensor([6, 4]), K, K, info=info, what="N=%d" % N)
    assert want["word_lengths"][0, 0] >= 2 and max(max(z) for z in info["sizes"]) > 1 and (want["num_hyps"] >= 2).all()


# ---------------------------------------------------------------------------------------------------------------- ends
@DTYPES
def test_every_kind_of_end_a_dead_end_and_a_rejected_final_word(dtype):
    A = _asg()
    from torch_asg_amd import Lexicon, WordLM
    lex = Lexicon([[0], [0, 1]], 3, 2)                     # nodes: 0 root, 1 "0" (word 0), 2 "01" (word 1)
    tr = torch.zeros(3, 3, dtype=dtype)
    x, _ = _normal(5, 3, 3, 39, dtype)
    lm = WordLM(2, [0, 2, 3], [0, 1, 0], [-0.5, -1.0, -0.25], [1, 1, 0], [-1, 0], [0.0, -0.125], 0, [-2.0, -0.75])
    _, want = _check(x, tr, lex, lm, A.WordLookahead(lex, lm, 2), None, 16, 16, what="ends")
    last = want["states"][:, :, 4]
    rows = np.arange(16)[None] < want["num_hyps"][:, None]
    assert (rows & (last == 0)).any() and (rows & (last == 1)).any() and (rows & (last == 2)).any()
    wl = want["word_lengths"]
    fin_word = np.take_along_axis(want["words"], np.maximum(wl - 1, 0)[..., None], 2)[..., 0]
    assert (fin_word[rows & (last == 2)] == 1).all() and (fin_word[rows & (last == 1)] == 0).all()      # the final word is there
    # word 0 = [0] is unknown to the LM, word 1 = [0, 1] known: the node of word 0 lives (word 1 lies below it), a pair kept
    # there has no end and is no row
    rej = WordLM(2, [0, 1], [1], [-0.5], [0], [-1], [0.0], 0, [-1.0])
    for order in (1, 2):
        info = {}
        _, want = _check(x, tr, lex, rej, A.WordLookahead(lex, rej, order), None, 16, 16, info=info, what="rejected")
        assert (want["num_cands"] < np.array([len(kept) for kept in info["last"]])).all() and (want["num_hyps"] > 0).all()
        assert (want["words"] != 0).all() and not (want["states"][:, :, 4] == 1).any()
    # the nodes [3] and [3, 0] of the hand case have no word below them that the LM knows: edges into [3] are no candidates
    lex, lm = hand_case()
    x, tr = _normal(7, 4, 5, 37, dtype)
    x[:, :, 3] += 2.0                                      # acoustics like the dead branch
    il = torch.tensor([7, 4, 1, 0])
    for order in (1, 2, 3):
        for K in (2, 8, ALL):
            info = {}
            _, want = _check(x, tr, lex, lm, A.WordLookahead(lex, lm, order), il, K, K, INF, 0.7, -0.4, 0.3, info=info, what="dead")
            assert info["dead"] > 0 and (want["states"] < 5).all()          # (the trie nodes 5 and 6 are [3] and [3, 0])
    # every path ends mid-word: the beam is full and there is no row
    long, null = Lexicon([[0, 1, 0]], 3, 2), WordLM.null(1)
    info = {}
    got, want = _check(x[:2, :3, :3], tr[:3, :3], long, null, A.WordLookahead(long, null, 1), None, 8, 3, info=info, what="mid-word")
    assert all(s[-1] > 0 for s in info["sizes"]) and (got["num_hyps"] == 0).all() and (got["scores"] == -np.inf).all()


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_capture_and_replay_with_fresh_emissions_and_lengths():
    A = _asg()
    lex, lm, x0, tr, _ = grid_case(3, torch.float32)
    la = A.WordLookahead(lex, lm, 2)
    T, B, N = 7, 4, 5
    x = torch.zeros(T, B, N, device=DEV)
    tr = tr.to(DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)
    args = (16, 6, 3.0, 0.7, -0.4, 0.3, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.beam_decode_words_nbest(x, tr, lex, lm, il, *args, lookahead=la)      # warm-up: compiles and caches lexicon, LM, look-ahead
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = A.beam_decode_words_nbest(x, tr, lex, lm, il, *args, lookahead=la)
    for seed in (1, 2, 3):
        gen = torch.Generator().manual_seed(seed)
        x.copy_(torch.randn(T, B, N, generator=gen))
        il.copy_(torch.tensor([T, seed, 0, T - seed]))
        gr.replay()
        torch.cuda.synchronize()
        want = beam_word_la_nbest_ref(x.cpu().numpy(), tr.cpu().numpy(), lex, lm, 2, il.cpu().numpy(), *args[:6])
        _same(_np(out, NAMES), want, NAMES, "replay %d" % seed)


def test_two_runs_give_identical_bits_groups_equal_one_call_and_none_is_the_plain_call():
    A = _asg()
    lex, lm = every_node_ends_a_word(40, 261)
    la = A.WordLookahead(lex, lm, 2)
    x, tr = _normal(10, 6, 40, 36, torch.float32)
    xd, trd = (x * 0.25).to(DEV), tr.to(DEV)
    ild = torch.tensor([10, 3, 0, 1, 9, 7], device=DEV)
    args = (300, 40, 6.0, 0.5, -0.2, 0.1, True)
    a = A.beam_decode_words_nbest(xd, trd, lex, lm, ild, *args, lookahead=la)
    assert int(a.num_hyps.max()) == 40
    for _ in range(2):
        b = A.beam_decode_words_nbest(xd, trd, lex, lm, ild, *args, lookahead=la)
        for u, v in zip(a, b):
            assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    from torch_asg_amd.asg import native
    be = native()
    seen = []
    buf = be._buf
    be._buf = lambda n, d: (seen.append(n), buf(n, d))[1]
    try:
        plain = A.beam_decode_words_nbest(xd, trd, lex, lm, ild, *args)
        plain_bytes = seen[-1]
        A.beam_decode_words_nbest(xd, trd, lex, lm, ild, *args, lookahead=la)
        assert seen[-1] == plain_bytes                     # no workspace of its own
        per = seen[-1] // 6
        small = A.beam_decode_words_nbest(xd, trd, lex, lm, ild, *args, max_work_bytes=2 * per + per // 2, lookahead=la)
        la_group = seen[-1]
        A.beam_decode_words_nbest(xd, trd, lex, lm, ild, *args, max_work_bytes=2 * per + per // 2)
        assert la_group == seen[-1] < 3 * per              # groups of equal workspace bytes with and without
    finally:
        del be._buf
    for u, v in zip(small, a):
        assert torch.equal(u, v)
    assert any(not torch.equal(u, v) for u, v in zip(a, plain))                       # it is another search
    # lookahead=None is the call without the keyword, byte for byte
    for u, v in zip(A.beam_decode_words_nbest(xd, trd, lex, lm, ild, *args, lookahead=None), plain):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    # a strided [T,B,N] view and the module method
    xt = xd.transpose(0, 1).contiguous().transpose(0, 1)
    for u, v in zip(A.beam_decode_words_nbest(xt, trd, lex, lm, ild, *args, lookahead=la), a):
        assert torch.equal(u, v)
    loss = A.ASGLoss(40).to(DEV)
    with torch.no_grad():
        loss.transition.copy_(trd)
    for u, v in zip(loss.beam_decode_words_nbest(xd, lex, lm, ild, *args, lookahead=la), a):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------------------------- stream
CHUNKINGS = ([12], [1] * 12, [5, 7], [3, 0, 4, 1, 4])


def _values_of_the_rows(ref, want, b, nh, L):
    """The search's own value v (the estimate included) of the pair each row of slot b ends in, in row order."""
    v = dict(ref.slots[b].A)
    se = ref.search
    q_of = {(int(se.label[q]), int(se.state[q])): q for q in range(se.Q)}
    return [v[(int(want["lm_states"][b, r, L - 1]), q_of[(int(want["path"][b, r, L - 1]), int(want["states"][b, r, L - 1]))])]
            for r in range(nh)]


@DTYPES
@pytest.mark.parametrize("chunks", CHUNKINGS, ids=["whole", "frames", "two", "ragged"])
def test_stream_prefixes_after_every_chunk_and_the_one_shot_rows_at_the_end(chunks, dtype):
    A = _asg()
    lex = small_lexicon([0.5, -1.0, 0.0, 2.0, -0.25])
    lm = arpa_lm(5, 3, 63, keep=(1.0, 0.5, 0.5))
    la = A.WordLookahead(lex, lm, 2)
    x, tr = _normal(12, 4, 5, 46, dtype)
    il = torch.tensor([12, 5, 1, 0])
    K, NB, args = 12, 8, (5.0, 0.7, -0.4, 0.3)
    s = A.BeamWordStream(tr.to(DEV), lex, lm, 4, 12, K, *args, dtype=dtype, lookahead=la)
    ref = BeamWordLaNbestStreamRef(tr.numpy(), lex, lm, 2, 4, 12, K, *args, dtype=x.numpy().dtype)
    t0 = 0
    mid_word = reordered = 0
    wos = np.asarray(lex.word_of_state)
    for n in chunks:
        cl = (il - t0).clamp(0, n)
        s.advance(x[t0:t0 + n].to(DEV), cl.to(DEV))
        ref.advance(x[t0:t0 + n].numpy(), cl.numpy())
        t0 += n
        before = s._state.clone()
        want = ref.result_nbest(NB, False)
        for align in (False, True):
            got = _np(s._result_nbest(NB, False, align), STREAM_NAMES)
            _same(got, want, STREAM_NAMES, "prefix after %d" % t0)
        one = s.result(False)                              # property 2, final == 0
        for n_ in ONE_BEST:
            assert got[n_][:, 0].tobytes() == getattr(one, n_).cpu().numpy().tobytes(), n_
        assert torch.equal(before, s._state)               # it reads the state only
        for b in range(4):
            L, nh = int(want["frames"][b]), int(want["num_hyps"][b])
            if L:
                last = want["states"][b, :nh, L - 1]
                mid_word += int(((last != 0) & (wos[last] < 0)).sum())
                vals = _values_of_the_rows(ref, want, b, nh, L)
                reordered += int(any(u < v for u, v in zip(vals, vals[1:])))
    assert mid_word > 0                                    # prefixes that end mid-word are rows
    assert reordered > 0                                   # ... and v - L orders some list otherwise than v would
    before = s._state.clone()
    got = _np(s._result_nbest(NB, True, True), STREAM_NAMES)
    assert torch.equal(before, s._state)
    _same(got, ref.result_nbest(NB, True), STREAM_NAMES, "final")
    one = s.result(True)                                   # property 2, final != 0
    for n_ in ONE_BEST:
        assert got[n_][:, 0].tobytes() == getattr(one, n_).cpu().numpy().tobytes(), n_
    shot = _gpu(x, tr, lex, lm, la, il, K, NB, *args)      # property 3
    for n in STREAM_NAMES[:-2]:
        assert got[n].tobytes() == shot[n].tobytes(), n
    assert (shot["num_hyps"][:2] >= 2).all() and got["frames"].tolist() == [12, 5, 1, 0]
    last = got["states"][0, :got["num_hyps"][0], 11]
    assert ((last == 0) | (wos[last] >= 0)).all()          # with the end, no row ends mid-word
    with pytest.raises(NotImplementedError, match="look-ahead"):
        s.result_nbest(NB)                                 # the public method is not opened yet


def test_a_captured_advance_and_result_nbest_is_replayed():
    A = _asg()
    lex, lm, x0, tr, _ = grid_case(3, torch.float32)
    la = A.WordLookahead(lex, lm, 2)
    K, NB, args = 6, 4, (3.0, 0.7, -0.4, 0.3)
    s = A.BeamWordStream(tr.to(DEV), lex, lm, 4, 12, K, *args, lookahead=la)
    chunk = torch.zeros(3, 4, 5, device=DEV)
    cl = torch.full((4,), 3, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.advance(chunk, cl)                               # warm-up; the scratch of _result_nbest is allocated here
        s._result_nbest(NB, False, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    s.reset()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        s.advance(chunk, cl)
        out = s._result_nbest(NB, False, True)
    s.reset()
    ref = BeamWordLaNbestStreamRef(tr.numpy(), lex, lm, 2, 4, 12, K, *args)
    for seed in (1, 2, 3):
        gen = torch.Generator().manual_seed(seed)
        chunk.copy_(torch.randn(3, 4, 5, generator=gen))
        cl.copy_(torch.tensor([3, seed, 0, 2]))
        gr.replay()
        torch.cuda.synchronize()
        ref.advance(chunk.cpu().numpy(), cl.cpu().numpy())
        _same(_np(out, STREAM_NAMES), ref.result_nbest(NB, False), STREAM_NAMES, "replay %d" % seed)


# ---------------------------------------------------------------------------------------------------------------- afterwards
def test_the_neighbours_are_unchanged_after_these_calls():
    A = _asg()
    lex, lm, x, tr, il = grid_case(3, torch.float32)
    la = A.WordLookahead(lex, lm, 2)
    xd, trd, ild = x.to(DEV), tr.to(DEV), il.to(DEV)
    plain_stream = A.BeamWordStream(trd, lex, lm, 4, 7, 16, 4.0, 0.7, -0.4, 0.3)
    plain_stream.advance(xd, ild)
    la_stream = A.BeamWordStream(trd, lex, lm, 4, 7, 16, 4.0, 0.7, -0.4, 0.3, lookahead=la)
    la_stream.advance(xd, ild)

    def others():
        outs = [o for o in A.beam_decode_words_nbest(xd, trd, lex, lm, ild, 64, 10, 4.0, 0.7, -0.4, 0.3, True)]
        outs += [o for o in plain_stream.result_nbest(5, True, True)] + list(plain_stream.result(False))
        outs += list(A.beam_decode_words(xd, trd, lex, lm, ild, 64, 4.0, 0.7, -0.4, 0.3))
        outs += list(A.beam_decode_words(xd, trd, lex, lm, ild, 64, 4.0, 0.7, -0.4, 0.3, lookahead=la))
        outs += list(la_stream.result(True)) + list(la_stream.result(False))
        outs += list(A.beam_decode_graph(xd, trd, lex.graph, ild, 6, 4.0, 0.8, -0.5))
        return [o.cpu() for o in outs]
    before = others()
    A.beam_decode_words_nbest(xd, trd, lex, lm, ild, 64, 10, 4.0, 0.7, -0.4, 0.3, True, lookahead=la)
    la_stream._result_nbest(5, True, True)
    la_stream._result_nbest(5, False, False)
    for u, v in zip(before, others()):
        assert torch.equal(u, v)
