"""CPU tests of the case table behind tests/test_hip_graph_regimes.py (tests/graph_regime_cases.py): every automaton has the
product-graph size the table states (from the restatement tests/graph_decode_ref.py::product, and from TokenGraph.compile_host),
every case is in the regime it names under the routing rules restated from include/asg_hip.h, the references of the big graphs
are not trivially -inf, and the reference of a wide batch equals the reference of each of its utterances alone."""
import numpy as np
import pytest

import graph_regime_cases as C
from graph_loss_ref import full_graph_ref

F32, F64 = C.F32, C.F64


@pytest.mark.parametrize("name", list(C.GRAPHS))
def test_product_graph_sizes(name):
    Q, E = C.facts(name)
    assert (Q, E) == C.expected(name)
    h = C.graph(name).compile_host(np.float32)
    assert (h["Q"], h["E"]) == (Q, E)
    assert C.graph(name).N == C.GRAPHS[name][1]


def test_case_a_and_b_sit_on_either_side_of_the_edge_threshold():
    (Qa, Ea), (Qb, Eb) = C.facts("bigram65"), C.facts("bigram64")
    assert Eb <= C.LOSS_EDGES < Ea
    for e in (4, 8):
        assert C.loss_resident(0, e, Qb, Eb) and not C.loss_resident(0, e, Qa, Ea)
        assert C.loss_resident(C.LOSS_RESIDENT, e, Qa, Ea) and not C.loss_resident(C.LOSS_STREAM, e, Qb, Eb)
        assert C.dec_resident(0, e, 65, Qa, Ea)                # (the decoder's threshold is 32768 edges)
    for B in (65, 130):
        il = C.inputs(7, B, 65, 1, True)[2]
        assert (B + 63) // 64 in (2, 3) and B % 64 != 0         # a partial last block of lanes
        assert C.mixed_parity(il)
        second = il[64:128].tolist()
        assert set(il[:3].tolist()) == {7, 0, 1} and (1 in second)
    il = C.inputs(7, 130, 65, 1, True)[2]
    assert {0, 1, 7} <= set(il[64:128].tolist()) and {0, 7} <= set(il[128:].tolist())


def test_case_d_takes_two_passes_of_the_resident_loops():
    Q, E = C.facts("trigram40_holes")
    assert C.WG < Q <= 2 * C.WG                                 # the q += 1024 loops run twice; a thread owns up to two states
    for e in (4, 8):
        assert C.loss_lds(e, Q) <= C.LDS_PLAIN                  # (plain launch: the LDS attribute is cases e to g)
        assert not C.loss_resident(0, e, Q, E) and C.loss_resident(C.LOSS_RESIDENT, e, Q, E)
    g = C.graph("trigram40_holes")
    h = g.compile_loss_host(np.float32)
    out = np.diff(h["orow"].astype(np.int64))
    assert ((out[:Q - C.WG] > 0) & (out[C.WG:Q] > 0)).any()    # both states of some thread own edge accumulators


def test_cases_e_and_f_need_the_lds_attribute_and_fit():
    for name, e in (("enterable600", 8), ("enterable1000", 4)):
        Q, E = C.facts(name)
        N = C.graph(name).N
        assert (4081 <= Q <= 8192) if e == 8 else (8161 <= Q <= 16384)
        assert C.LDS_PLAIN < C.loss_lds(e, Q) <= 256 + C.VEC_BYTES
        assert C.loss_resident(C.LOSS_RESIDENT, e, Q, E) and not C.loss_resident(0, e, Q, E)
        assert C.LDS_PLAIN < C.dec_lds(e, N, Q) <= 160 * 1024
        assert C.dec_resident(C.DEC_RESIDENT, e, N, Q, E) and not C.dec_resident(0, e, N, Q, E)
        assert C.dec_stage_frames(e, N, Q) == (4 if e == 8 else 2)


@pytest.mark.parametrize("fits,over,e", [("shift16384", "shift16385", 4), ("shift8192", "shift8193", 8)])
def test_case_g_loss_fit_limit(fits, over, e):
    (Q0, E0), (Q1, E1) = C.facts(fits), C.facts(over)
    assert 2 * Q0 * e == C.VEC_BYTES and Q1 == Q0 + 1
    assert C.loss_resident(C.LOSS_RESIDENT, e, Q0, E0) and not C.loss_resident(C.LOSS_RESIDENT, e, Q1, E1)
    assert C.loss_lds(e, Q0) == 256 + C.VEC_BYTES


@pytest.mark.parametrize("fits,over,e", [("shift16380", "shift16381", 4), ("shift8188", "shift8189", 8)])
def test_case_g_decoder_fit_limit(fits, over, e):
    (Q0, E0), (Q1, E1) = C.facts(fits), C.facts(over)
    assert 2 * (Q0 + 4) * e == C.VEC_BYTES and Q1 == Q0 + 1
    assert C.dec_resident(C.DEC_RESIDENT, e, 4, Q0, E0) and not C.dec_resident(C.DEC_RESIDENT, e, 4, Q1, E1)
    assert C.dec_stage_frames(e, 4, Q0) == (4 if e == 8 else 2)


def test_case_h_alphabet_limit_of_the_resident_decoder():
    (Q0, E0), (Q1, E1) = C.facts("one_state1024"), C.facts("one_state1025")
    assert C.dec_resident(C.DEC_RESIDENT, 4, 1024, Q0, E0) and not C.dec_resident(0, 4, 1024, Q0, E0)
    assert C.dec_lds(4, 1024, Q0) == 512 + 4 * 1024 * 4         # the transition matrix (4 MiB) stays in global memory
    assert not C.dec_resident(C.DEC_RESIDENT, 4, 1025, Q1, E1)
    assert 2 * (Q1 + 1025) * 4 <= C.VEC_BYTES                   # ... refused for N > 1024 alone


@pytest.mark.parametrize("name", ["cycle3", "cycle3_n14"])
def test_case_i_has_more_labels_than_product_states(name):
    g = C.graph(name)
    Q, E = C.facts(name)
    assert g.N > Q
    tokens = list(C.CYCLE_TOKENS[name])
    # a label with product states beyond the wavefronts of a grid sized by Q alone: only where the case says so
    assert (max(tokens) >= (Q + 3) // 4 * 4) == (name == "cycle3_n14")
    h = g.compile_loss_host(np.float64)
    per_label = np.diff(h["lrow"])
    assert (per_label[tokens] == 3).all() and per_label.sum() == Q
    if name == "cycle3_n14":                                    # ... and its gradient is not zero
        gx = C.loss_reference(name, 6, 66, 9, True)[1]
        assert (gx[:, :, 13] != 0).any() and (gx[:, :, 2:13] == 0).all()


def test_restated_routing_is_the_librarys_own_at_the_limits():
    """The GPU tests assert their regimes from the rules restated in tests/graph_regime_cases.py, and a call that streams where
    it should have stayed resident still computes the right numbers.  So the restatement is compared here with the library's own
    predicates (host code, no GPU): asg::graph_loss_resident(route, elem, Q, E) and asg::graph_decode_resident(elem, N, Q, E).

    A stop-gap: neither predicate is in include/asg_hip.h, so they are looked up by their Itanium-mangled names (int64_t as `l`:
    LP64 Linux), and the decoder's static resident_fits is reached only through graph_decode_resident(.., E = 0).  A changed
    signature or hidden visibility fails here by name, and the cure is then an exported predicate in the C ABI, not dropping
    this test: it is the only one that tells `<=` from `<` in the fit and edge rules and `N <= 1024` from `N < 1024`."""
    import ctypes
    from torch_asg_amd import _lib
    L = _lib.lib()

    def internal(symbol, argtypes):
        try:
            f = getattr(L, symbol)
        except AttributeError:
            pytest.fail("libasg_hip.so no longer exports %s: the routing predicate changed its signature or its visibility; "
                        "export a predicate through include/asg_hip.h and compare with that" % symbol)
        f.restype, f.argtypes = ctypes.c_bool, argtypes
        return f
    loss = internal("_ZN3asg19graph_loss_residentEiiil", [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64])
    dec = internal("_ZN3asg21graph_decode_residentEiiii", [ctypes.c_int] * 4)
    route = {0: 0, C.LOSS_STREAM: 1, C.LOSS_RESIDENT: 2}
    for e in (4, 8):
        limit = C.VEC_BYTES // (2 * e)
        for Q in (0, 1, 64, 65, 1024, 1025, limit - 1, limit, limit + 1, 2 * limit):
            for E in (0, C.LOSS_EDGES - 1, C.LOSS_EDGES, C.LOSS_EDGES + 1, 1 << 20):
                for flags, r in route.items():
                    assert bool(loss(r, e, Q, E)) == C.loss_resident(flags, e, Q, E), (e, Q, E, flags)
        for N in (1, 4, 1023, 1024, 1025, 4096):
            for Q in (1, 1024, limit - N - 1, limit - N, limit - N + 1, 2 * limit):
                if Q < 1:
                    continue
                for E in (0, C.DEC_EDGES - 1, C.DEC_EDGES, C.DEC_EDGES + 1):
                    assert bool(dec(e, N, Q, E)) == C.dec_resident(0, e, N, Q, E), (e, N, Q, E)
                assert bool(dec(e, N, Q, 0)) == C.dec_resident(C.DEC_RESIDENT, e, N, Q, 1 << 20), (e, N, Q)
    for name in C.GRAPHS:
        Q, E = C.facts(name)
        N = C.graph(name).N
        for e in (4, 8):
            assert bool(loss(0, e, Q, E)) == C.loss_resident(0, e, Q, E) and bool(loss(2, e, Q, E)) == C.loss_resident(256, e, Q, E)
            if Q:
                assert bool(dec(e, N, Q, E)) == C.dec_resident(0, e, N, Q, E)


def test_subgroup_of_64_lanes_is_unreachable():
    """dec_subgroup returns 64 only for Q <= 16 with a mean in-degree of 128 or more, and a target has at most Q - 1 sources."""
    for Q in range(1, 65):
        assert C.dec_subgroup(Q, Q * (Q - 1)) != 64             # the densest product graph of Q states
    assert C.dec_subgroup(40, 1560) == 16 and C.dec_subgroup(1024, 1024 * 1023) == 4
    for name in C.GRAPHS:
        Q, E = C.facts(name)
        if Q:
            h = C.graph(name).compile_host(np.float32)
            assert np.diff(h["row"]).max(initial=0) <= Q - 1
            assert C.dec_subgroup(Q, E) in (4, 16)


@pytest.mark.parametrize("name,T,B,seed,f64", [("enterable600", 5, 3, 4, True), ("enterable1000", 5, 2, 5, False),
                                               ("shift16384", 6, 2, 6, False), ("shift16385", 6, 2, 6, False),
                                               ("shift8192", 6, 2, 6, True), ("shift8193", 6, 2, 6, True),
                                               ("shift16380", 6, 2, 6, False), ("shift16381", 6, 2, 6, False),
                                               ("shift8188", 6, 2, 6, True), ("shift8189", 6, 2, 6, True)])
def test_big_graph_references_are_not_trivial(name, T, B, seed, f64):
    il = C.inputs(T, B, C.graph(name).N, seed, f64)[2].numpy()
    Z = C.loss_reference(name, T, B, seed, f64)[0]
    live = il >= 1
    assert np.isfinite(Z[live]).sum() * 2 > live.sum()
    assert C.finite_states(name, T) >= 64                       # at the last frame of a full-length utterance
    if name.startswith("shift"):                                # live values in every quarter of the state vectors
        mask = C.finite_mask(name, T)
        assert all(part.sum() >= 16 for part in np.array_split(mask, 4))
    sc = C.decode_reference(name, T, B, seed, f64)[0]
    assert np.isfinite(sc[live]).sum() * 2 > live.sum()


def test_reference_of_a_wide_batch_equals_its_utterances_alone():
    g = C.graph("bigram65")
    T, B = 7, 130
    x, tr, il, gs = C.inputs(T, B, 65, 1, True)
    Z, gx, gtr = C.loss_reference("bigram65", T, B, 1, True)
    acc = np.zeros_like(gtr)
    for b in range(B):
        z1, gx1, gtr1 = full_graph_ref(x[:, b:b + 1].numpy(), tr.numpy(), g.next, g.weight, g.final, g.start, il[b:b + 1].numpy(),
                                       1.0, 0.0, gs[b:b + 1].numpy())
        assert z1[0] == Z[b] and np.array_equal(gx1[:, 0], gx[:, b])
        acc += gtr1
    assert np.allclose(acc, gtr, rtol=1e-12, atol=1e-12)
    sc, path, tok, tl, st = C.decode_reference("bigram65", T, B, 1, True)
    from graph_decode_ref import decode_graph_ref
    for b in (0, 1, 2, 63, 64, 65, 66, 127, 128, 129):
        one = decode_graph_ref(x[:, b:b + 1].numpy(), tr.numpy(), g.next, g.weight, g.final, g.start, il[b:b + 1].numpy())
        assert one[0][0] == sc[b] and np.array_equal(one[1][0], path[b]) and np.array_equal(one[2][0], tok[b])
        assert one[3][0] == tl[b] and np.array_equal(one[4][0], st[b])
