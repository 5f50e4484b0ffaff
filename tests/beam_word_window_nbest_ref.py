"""Test-only numpy restatement of the N BEST hypotheses of the windowed word-LM beam stream
(`BeamWordWindowStream.result_nbest`), written from the specification (include/asg_hip.h::asg_beam_word_window_nbest and
::asg_beam_word_window_nbest_la) and not from the package: no ranks, no tables.  It works over the carried state of the two window
restatements (tests/beam_word_window_ref.py `BeamWordWindowRef`, tests/beam_word_la_stream_ref.py `BeamWordLaWindowRef`): the
stored set `A`, the ring through `_walk`, and `base`, `carry`, `carry_state`.  It only reads them.

Candidates: every kept pair (h, q) with value v whose end is > -inf, where
  final   end = (v + final_w[q]) + endw; endw = ew[h] at the root, a + ew[h'] behind the LM walk (h, word) -> (h', a) in a word-end
          node -- with look-ahead (a - L(h, state(q))) + ew[h'] --, none mid-word or where the LM rejects the word;
  prefix  end = v -- with look-ahead v - L(h, state(q)),
in (end descending, pair ascending) order; the first nbest are the rows.  A row is the candidate's own chain from frame pos-1
down to `base`, at most W frames, possibly none.  Tokens: a label that differs from the label before it, the label before column
0 being `carry`.  Words: a separator behind a label that is neither the separator nor -1 gives word_of_state[the automaton state
before it], which before column 0 is `carry_state`; with `final` the word of a word-end last node is appended, also behind an
empty tail.

Besides the outputs the result holds `records`: per slot a list, per row, of dict(pair, tail, sep0) -- the candidate's pair, the
length of its tail and whether column 0 is a separator edge out of the committed part -- for the tests that must reach a regime.
"""
import numpy as np

NAMES = ("scores", "tokens", "token_lengths", "words", "word_lengths", "num_hyps", "path", "states", "lm_states", "frames",
         "committed", "status")
SEQS = ("path", "states", "lm_states", "tokens", "words")


def _end(s, h, q, v, final):
    """-> (end, final word or -1) of the kept pair (h, q) with value v, or None."""
    dt = s.dt
    look = hasattr(s, "look")
    ls = s.L(h, q) if look else None                        # finite for every kept pair
    if not final:
        return (dt(v - ls) if look else v), -1
    st = s.state[q]
    if st == 0:
        return dt(dt(v + s.finw[st]) + s.ew[h]), -1
    if s.wos[st] < 0:
        return None                                         # mid-word: no end
    w = s.step(h, int(s.wos[st]))
    if w is None:
        return None
    endw = dt(dt(w[1] - ls) + s.ew[w[0]]) if look else dt(w[1] + s.ew[w[0]])
    return dt(dt(v + s.finw[st]) + endw), int(s.wos[st])


def word_window_nbest(ref, nbest, final):
    """ref: a BeamWordWindowRef or BeamWordLaWindowRef -> a dict with the keys of NAMES (scores [B,nbest]; tokens, words, path,
    states, lm_states [B,nbest,W]; token_lengths, word_lengths [B,nbest]; num_hyps, frames, committed, status [B]) and `records`."""
    B, W, dt, s, nbest = ref.B, ref.W, ref.dt, ref.s, int(nbest)
    assert nbest >= 1
    res = {"scores": np.full((B, nbest), -np.inf, dt), "num_hyps": np.zeros(B, np.int64),
           "token_lengths": np.zeros((B, nbest), np.int64), "word_lengths": np.zeros((B, nbest), np.int64),
           "frames": np.array([v.pos for v in ref.slots], np.int64),
           "committed": np.array([v.base for v in ref.slots], np.int64),
           "status": np.array([v.status | (2 if v.pos >= 1 and not v.A else 0) for v in ref.slots], np.int64),
           "records": [[] for _ in range(B)]}
    for n in SEQS:
        res[n] = np.full((B, nbest, W), -1, np.int64)
    for b, v in enumerate(ref.slots):
        if v.pos == 0 or not v.A:
            continue
        cands = []
        with np.errstate(invalid="ignore", over="ignore"):
            for (h, q), val in v.A:
                e = _end(s, h, q, val, final)
                if e is not None and e[0] > s.ninf:
                    cands.append((e[0], (h, q), e[1]))
        cands.sort(key=lambda it: (-it[0], it[1]))          # (-0.0 and +0.0 compare equal)
        res["num_hyps"][b] = min(nbest, len(cands))
        for r, (e, pair, fw) in enumerate(cands[:nbest]):
            res["scores"][b, r] = e
            tail = ref._walk(v, pair, v.pos - 1, v.base)    # [] when base == pos: the row still counts
            assert len(tail) == v.pos - v.base <= W
            seqs = {n: [] for n in SEQS}
            lab0, sta0 = v.carry, v.carry_state
            sep0 = False
            for t, (h, q) in enumerate(tail):
                lab, sta = int(s.label[q]), int(s.state[q])
                seqs["path"].append(lab)
                seqs["states"].append(sta)
                seqs["lm_states"].append(int(h))
                if lab != lab0:
                    seqs["tokens"].append(lab)
                if lab == s.sep and lab0 != s.sep and lab0 != -1:
                    seqs["words"].append(int(s.wos[sta0]))
                    sep0 = sep0 or t == 0
                lab0, sta0 = lab, sta
            if fw >= 0 and len(seqs["words"]) < W:
                seqs["words"].append(fw)
            for n in SEQS:
                res[n][b, r, :len(seqs[n])] = seqs[n]
            res["token_lengths"][b, r], res["word_lengths"][b, r] = len(seqs["tokens"]), len(seqs["words"])
            res["records"][b].append(dict(pair=pair, tail=len(tail), sep0=sep0))
    return res
