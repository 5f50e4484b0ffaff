"""Test-only numpy restatement of the beam-pruned full score over the pairs a LOOK-AHEAD search keeps
(`torch_asg_amd.beam_words_full_score(..., lookahead=)`, `beam_words_asg_loss(..., lookahead=)`), written from the specification
(include/asg_hip.h::asg_beam_words_full_forward_la): the kept sets A_t are those of tests/beam_word_la_ref.py
(`beam_word_la_ref(..., info=)["kept"]`, plain loops over the words below a node: no ranks, no tables), the forced sets F_t
those of tests/beam_word_loss_ref.py (`forced_sets`: no look-ahead enters the walk of the target), and the lattice over
U_t = A_t | F_t is that file's, with the plain weights, through `beam_word_loss_ref(..., sets=)`."""
import numpy as np

from beam_word_la_ref import beam_word_la_ref
from beam_word_loss_ref import beam_word_loss_ref, forced_sets, word_model
from graph_decode_ref import _clamped_lengths


def la_lattice_sets(inputs, transition, lexicon, lm, order, input_lengths=None, beam_size=1, beam_threshold=np.inf, lm_weight=1.0,
                    word_score=0.0, token_score=0.0, targets=None, target_lengths=None, info=None):
    """`beam_word_loss_ref.lattice_sets` with the kept sets of the look-ahead search of `order` -> (model, lens, A, F, U).
    `info`, if a dict, receives beam_word_la_ref's info and its result under 'decode'."""
    xs = np.asarray(inputs)
    dt = xs.dtype.type
    T, B, _ = xs.shape
    lens = _clamped_lengths(input_lengths, T, B)
    inf = {}
    res = beam_word_la_ref(xs, np.asarray(transition).astype(dt), lexicon, lm, order, input_lengths, beam_size, beam_threshold,
                           lm_weight, word_score, token_score, info=inf)
    if info is not None:
        info.update(inf)
        info["decode"] = res
    m = word_model(lexicon, lm, dt, lm_weight, word_score, token_score)
    tg = None if targets is None else np.asarray(targets)
    tls = None if tg is None else (np.full(B, tg.shape[1]) if target_lengths is None else np.clip(np.asarray(target_lengths), 0, tg.shape[1]))
    As, Fs, Us = [], [], []
    for b in range(B):
        L = int(lens[b])
        A = [list(k) for k in inf["kept"][b]] + [[] for _ in range(L - len(inf["kept"][b]))]
        F = forced_sets(m, tg[b, :int(tls[b])], L) if tg is not None else [[] for _ in range(L)]
        As.append(A), Fs.append(F), Us.append([sorted(set(a) | set(f)) for a, f in zip(A, F)])
    return m, lens, As, Fs, Us


def beam_word_la_loss_ref(inputs, transition, lexicon, lm, order, input_lengths=None, beam_size=1, beam_threshold=np.inf,
                          lm_weight=1.0, word_score=0.0, token_score=0.0, targets=None, target_lengths=None, grad_scores=None,
                          info=None, sets=None):
    """The arguments of `beam_word_loss_ref` plus `order` -> its (Z_K [B], grad_inputs, grad_transition, U)."""
    if sets is None:
        sets = la_lattice_sets(inputs, transition, lexicon, lm, order, input_lengths, beam_size, beam_threshold, lm_weight,
                               word_score, token_score, targets, target_lengths, info)
    return beam_word_loss_ref(inputs, transition, lexicon, lm, input_lengths, beam_size, beam_threshold, lm_weight, word_score,
                              token_score, targets, target_lengths, grad_scores, sets=sets)
