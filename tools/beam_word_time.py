#!/usr/bin/env python3
"""Developer probe: per-call time of beam decoding with a lexicon and a word LM composed on the fly
(torch_asg_amd.beam_decode_words) next to the token-automaton beam decoder (beam_decode_graph) on the lexicon's own graph at the
same beam in the same session -- the ratio is the cost of the pair addressing (hash table, LM walk, wider keys).  Device events
after a warm-up: the median and the spread (min .. max) of CALLS single calls.

    python tools/beam_word_time.py [T,B,N,words,successors ...]   (default: the shapes DESIGN.md section 5n reports)
    BEAMS=64,256,1024 CALLS=7                                      (environment)

The lexicon is synthetic: `words` distinct random spellings of 3 to 8 letters over N-1 tokens (token N-1 separates words).  The LM
is a synthetic bigram: every unigram, and about `successors` explicit successors per one-word history, random weights.  Emissions
are log-softmax of N(0,1).
"""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from graph_decode_time import timed  # noqa: E402

DEV = "cuda:0"
SHAPES = [(400, 64, 40, 20000, 50), (400, 64, 40, 2000, 50)]


def make_spellings(N, words, seed=0):
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < words:
        n = int(rng.integers(3, 9))
        w = rng.integers(0, N - 1, n)
        if (w[1:] == w[:-1]).any() or w.tobytes() in seen:
            continue
        seen.add(w.tobytes())
        out.append(w.tolist())
    return out


def make_lexicon(N, words, seed=0):
    return torch_asg_amd.Lexicon(make_spellings(N, words, seed), N, N - 1)


def make_bigram(V, successors, seed=0):
    """States: 0 the empty history, 1 the history <s>, 2 + w the history (w)."""
    rng = np.random.default_rng(seed)
    H = V + 2
    k = min(successors, V)
    rows = [np.arange(V)] + [np.sort(rng.choice(V, k, replace=False)) for _ in range(H - 1)]
    row = np.zeros(H + 1, np.int64)
    np.cumsum([r.size for r in rows], out=row[1:])
    word = np.concatenate(rows)
    logp = -rng.uniform(0.5, 8.0, word.size)
    backoff = np.zeros(H, np.int64)
    backoff[0] = -1
    bow = -rng.uniform(0.0, 2.0, H)
    bow[0] = 0.0
    return torch_asg_amd.WordLM(V, row, word, logp, word + 2, backoff, bow, 1, -rng.uniform(1.0, 6.0, H))


def calls(fn, n):
    """-> (median, min, max) in us of n single calls, after two warm-up calls."""
    fn()
    fn()
    ts = [timed(fn, 1) for _ in range(n)]
    return statistics.median(ts), min(ts), max(ts)


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256,1024").split(",")]
    n = int(os.environ.get("CALLS", "7"))
    whole = 1 << 40                                                       # one group
    for T, B, N, words, succ in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        lex = make_lexicon(N, words)
        lm = make_bigram(words, succ)
        c = lex.graph.compile_beam(DEV, torch.float32, 1.0, 0.0)
        print("T=%d B=%d N=%d words=%d S=%d Q=%d E=%d max_out=%d H=%d A=%d calls=%d" % (
            T, B, N, words, lex.graph.S, c["Q"], c["E"], c["max_out"], lm.H, lm.A, n), flush=True)
        for K in beams:
            plain = lambda: torch_asg_amd.beam_decode_graph(x, tr, lex.graph, il, K, max_work_bytes=whole)       # noqa: E731
            pairs = lambda: torch_asg_amd.beam_decode_words(x, tr, lex, lm, il, K, max_work_bytes=whole)         # noqa: E731
            base, lo, hi = calls(plain, n)
            print("  K=%-5d beam_decode_graph  %9.1f us (%9.1f .. %9.1f)  %7.2f us per frame" % (K, base, lo, hi, base / T), flush=True)
            med, lo, hi = calls(pairs, n)
            out = pairs()
            print("  K=%-5d beam_decode_words  %9.1f us (%9.1f .. %9.1f)  %7.2f us per frame  x%.2f  words per utterance %.1f  "
                  "finite %d/%d" % (K, med, lo, hi, med / T, med / base, float(out.word_lengths.double().mean()),
                                    int(torch.isfinite(out.scores).sum()), B), flush=True)


if __name__ == "__main__":
    main()
