"""Test-only numpy restatement of beam-pruned Viterbi decoding over the ASG lattice composed with a token automaton
(`torch_asg_amd.beam_decode_graph`), written from the specification (include/asg_hip.h::asg_beam_decode_graph) and not from the
package.  Folding and product states are those of tests/graph_decode_ref.py (`fold`, `product`).

Per utterance and frame, vectorised over the candidates: the candidates of frame t come only from the active set of frame t-1
(the stay of an active q, whose source is q, and every edge out of an active q'); a target keeps its largest candidate, the
smallest source on a tie; c = best + emission; states with c = -inf are dropped; with m = max c and lo = fl(m - threshold) the new
active set is the first K states in (c descending, q ascending) order that have c >= lo.  All arithmetic in the dtype of the
emissions, in the kernels' order: stay v + tr[i][i]; move (v + tr[i][j]) + arcw; then + emission.

For the tests that ask in which regime of the device's select a frame falls (tests/beam_select_cases.py), `select_info` restates
what that select would do with a frame's candidates -- the order-preserving keys, the width `rem` of its radix select, the exit
it takes -- and `wrong_rank` orders the candidates as a subtly wrong select would.  Neither changes an output of the
specification path.
"""
import numpy as np

from graph_decode_ref import _clamped_lengths, fold, product

# the exits of the select, in the order the device tests for them
EXITS = ("nothing", "equal-fit", "equal-cut", "whole", "kth-ties-taken", "tie-select")
WRONG = ("low_bits", "last_digit", "raw_bits", "q_second_digit", "q_last_digit", "ties_from_top")


def key_enc(c):
    """Key<R>::enc of csrc/asg_beam_common.h: the float's bits as an unsigned integer that orders as the float does; x + 0 first,
    so that -0 and +0 are one key."""
    c = np.asarray(c) + 0
    U = {4: np.uint32, 8: np.uint64}[c.dtype.itemsize]
    b = np.atleast_1d(c).view(U)
    top = U(1 << (8 * c.dtype.itemsize - 1))
    return np.where(b & top, ~b, b | top).reshape(c.shape)


def digit_shifts(bits):
    """A radix select over `bits` bits walks them from the top in digits of 8 bits, the last one narrower: [(shift, width)]."""
    out = []
    while bits > 0:
        w = min(bits, 8)
        out.append((bits - w, w))
        bits -= w
    return out


def q_bits(Q):
    """The bits of the tie select over q: those that hold 0 .. Q - 1, at least 1."""
    return max(1, int(Q - 1).bit_length())


def select_info(q, c, K, theta):
    """What the device's select does with the finite candidates (q, c) of one frame -> dict: n; passing (candidates with
    c >= lo = fl(max - theta)); rem (the bit length of enc(max(lo, kmin)) ^ enc(kmax): the bits its radix select walks); exit,
    one of EXITS -- nothing passes; rem == 0 and at most K keys (all equal) pass; rem == 0 and more than K; everything that
    passes taken whole on the first pass; the K-th key found and all its ties taken; the tie select over q.  For the two
    exits that cut ties also need (how many of the tied are taken), tied (how many there are) and cut (the last q taken, the
    first q dropped)."""
    q, c = np.asarray(q), np.asarray(c)
    if c.size == 0:
        return dict(n=0, passing=0, rem=0, exit="nothing")
    key = key_enc(c)
    kmax, kmin = key.max(), key.min()
    lokey = key_enc(np.asarray(c.max() + 0 - theta, c.dtype))
    rem = (int(max(lokey, kmin)) ^ int(kmax)).bit_length()
    passing = int((key >= lokey).sum())
    rec = dict(n=int(c.size), passing=passing, rem=rem)
    if passing <= K:
        rec["exit"] = "equal-fit" if rem == 0 else "whole"
        return rec
    kth = np.sort(key[key >= lokey])[::-1][K - 1]
    need, tied = K - int((key > kth).sum()), int((key == kth).sum())
    if tied == need:
        rec["exit"] = "kth-ties-taken"
        return rec
    tq = np.sort(q[key == kth])
    rec.update(exit="equal-cut" if rem == 0 else "tie-select", need=need, tied=tied, cut=(int(tq[need - 1]), int(tq[need])))
    return rec


def wrong_rank(wrong, q, c, theta, Q):
    """The candidates in the order of a select that is wrong in one way (one of WRONG): the low rem % 8 bits of the keys -- the
    narrow last digit of the key select -- ignored; its whole last digit ignored; the keys compared as raw sign-magnitude bits,
    so that negative values order upside down; the second digit, or the last digit, of the tie select over q cleared (two
    states it cannot tell apart come out in REVERSED order: one representative of what such a select may do); the tied taken
    from the largest q down."""
    assert wrong in WRONG
    key = key_enc(c)
    U = key.dtype.type
    rem = select_info(q, c, 1, theta)["rem"]
    q2 = q
    if wrong == "low_bits":
        key = key >> U(rem % 8)
    elif wrong == "last_digit":
        key = key >> U((rem % 8 or 8) if rem else 0)
    elif wrong == "raw_bits":
        key = (np.asarray(c) + 0).view(U) ^ U(1 << (8 * key.dtype.itemsize - 1))
    elif wrong == "ties_from_top":
        q2 = -q
    else:
        digits = digit_shifts(q_bits(Q))
        shift, w = digits[1 if wrong == "q_second_digit" else -1] if len(digits) > 1 else (0, 0)
        q2 = q & ~(((1 << w) - 1) << shift)
    return np.lexsort((-q, q2, ~key))                    # key descending, q2 ascending, then q descending


def beam_decode_ref(inputs, transition, next_, weight, final, start=0, input_lengths=None, beam_size=1, beam_threshold=np.inf,
                    lm_weight=1.0, token_score=0.0, sizes=None, info=None, wrong=None):
    """inputs [T,B,N], transition [N,N], the automaton -> scores [B], path, tokens [B,T], token_lengths [B], states [B,T] as
    `decode_graph_ref`.  `sizes`, if a list, receives per utterance the list of |A_t|.  `info`, if a dict, receives Q and
    frames: per utterance, per frame, the record of `select_info` (frames behind an empty set have none).  `wrong`, one of
    WRONG, runs every frame's select wrongly in that way; the default is the specification."""
    x = np.asarray(inputs)
    T, B, N = x.shape
    dt = x.dtype.type
    K = int(beam_size)
    theta = dt(beam_threshold)
    assert K >= 1 and theta >= 0
    tr = np.ascontiguousarray(np.asarray(transition), dtype=dt)
    nxt = np.asarray(next_, np.int64)
    present, arcw, finw = fold(nxt, weight, final, dt, lm_weight, token_score)
    label, state, src, tgt, Q = product(nxt, present)
    lens = _clamped_lengths(input_lengths, T, B)
    scores = np.full(B, -np.inf, dt)
    path = np.full((B, T), -1, np.int64)
    tokens = np.full((B, T), -1, np.int64)
    token_lengths = np.zeros(B, np.int64)
    states = np.full((B, T), -1, np.int64)
    if info is not None:
        info.update(Q=Q, frames=[])
    if T == 0 or Q == 0:
        return scores, path, tokens, token_lengths, states
    ninf = dt(-np.inf)
    frames = []                                          # the records of the utterance in hand
    start_w = np.where(present[start, label] & (nxt[start, label] == state), arcw[start, label], ninf).astype(dt)
    # the edges from the source side
    order = np.lexsort((tgt, src))
    osrc, otgt = src[order], tgt[order]
    orow = np.zeros(Q + 1, np.int64)
    np.cumsum(np.bincount(osrc, minlength=Q), out=orow[1:])
    otr = tr[label[otgt], label[osrc]]
    ow = arcw[state[osrc], label[otgt]]
    stay_tr = tr[label, label]

    def prune(q, c):
        """candidate states q with values c -> the active set (q, c, positions kept)."""
        ok = c > ninf
        idx = np.nonzero(ok)[0]
        q, c = q[idx], c[idx]
        if info is not None:
            frames.append(select_info(q, c, K, theta))
        if q.size == 0:
            return q, c, idx
        lo = c.max() - theta
        if wrong is not None:                            # (a wrong order may rank a candidate below lo among the first K)
            rank = wrong_rank(wrong, q, c, theta, Q)
            rank = rank[c[rank] >= lo][:K]
            return q[rank], c[rank], idx[rank]
        rank = np.lexsort((q, -c))                       # c descending, q ascending
        rank = rank[:K]
        rank = rank[c[rank] >= lo]
        return q[rank], c[rank], idx[rank]

    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            L = int(lens[b])
            frames = []
            if info is not None:
                info["frames"].append(frames)
            if L == 0:
                continue
            xb = x[:, b]
            q0 = np.arange(Q)
            aq, av, _ = prune(q0, start_w + xb[0, label])
            hist = [(aq, None)]                               # per frame: active states, their sources
            nact = [aq.size]
            for t in range(1, L):
                if aq.size == 0:
                    hist.append((aq, aq))
                    nact.append(0)
                    continue
                cnt = orow[aq + 1] - orow[aq]
                k_of = np.repeat(np.arange(aq.size), cnt)
                e = orow[aq][k_of] + (np.arange(k_of.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))
                ct = np.concatenate([aq, otgt[e]])
                cs = np.concatenate([aq, aq[k_of]])
                cv = np.concatenate([av + stay_tr[aq], (av[k_of] + otr[e]) + ow[e]])
                o = np.lexsort((cs, -cv, ct))                # per target: value descending, source ascending
                ct, cs, cv = ct[o], cs[o], cv[o]
                first = np.ones(ct.size, bool)
                first[1:] = ct[1:] != ct[:-1]
                bt, bsrc, bv = ct[first], cs[first], cv[first]
                aq, av, kept = prune(bt, bv + xb[t, label[bt]])
                hist.append((aq, bsrc[kept]))
                nact.append(aq.size)
            if sizes is not None:
                sizes.append(nact)
            if aq.size == 0:
                continue
            end = av + finw[state[aq]]
            o = np.lexsort((aq, -end))[0]
            if not end[o] > ninf:
                continue
            scores[b] = end[o]
            q = int(aq[o])
            for t in range(L - 1, -1, -1):
                path[b, t], states[b, t] = label[q], state[q]
                if t >= 1:
                    fq, fs = hist[t]
                    q = int(fs[np.nonzero(fq == q)[0][0]])
            p = path[b, :L]
            keep = np.ones(L, bool)
            keep[1:] = p[1:] != p[:-1]
            tk = p[keep]
            tokens[b, :len(tk)] = tk
            token_lengths[b] = len(tk)
    return scores, path, tokens, token_lengths, states
