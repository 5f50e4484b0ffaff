#!/usr/bin/env python3
"""Developer probe: what LM look-ahead (torch_asg_amd.WordLookahead) costs and what it buys in beam_decode_words.

Table 1, the price: per-call time of beam_decode_words without look-ahead and with order 1 and 2 at the same beam in the same
session, on the synthetic lexicons and bigram of tools/beam_word_time.py with log-softmax N(0,1) emissions.  Device events after a
warm-up: the median and the spread (min .. max) of CALLS single calls.

Table 2, the gain: word sequences sampled from the LM (from the explicit successors of the history, in proportion to exp(logp)),
spelled through the lexicon with 3 to 6 frames per token (the separator included); the emissions are the log-probabilities of a
one-hot-like distribution (0.9 on the frame's token, the rest shared) plus N(0, SIGMA^2) noise on every entry.  The search
without look-ahead at K = 4096 is the yardstick; for every smaller K the share of utterances whose `words` equal the yardstick's,
without look-ahead and with order 1 and 2.

    python tools/beam_word_la_time.py [T,B,N,words,successors ...]   (default: the shapes DESIGN.md section 5r reports)
    BEAMS=16,64,256,1024 CALLS=5 GAIN_BEAMS=8,16,32,64,128,256 UTTS=256 SIGMA=2.0,3.0 SEED=0   (environment)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from beam_word_time import calls, make_bigram, make_lexicon  # noqa: E402

DEV = "cuda:0"
SHAPES = [(400, 64, 40, 20000, 50), (400, 64, 40, 2000, 50)]
WHOLE = 1 << 40                                                               # one group


def sample_utterances(lm, spellings, T, B, N, sigma, seed):
    """-> emissions [T, B, N] float32, lengths [B]: B sampled word sequences, each cut to the last whole word within T frames."""
    rng = np.random.default_rng(seed)
    hit, miss = np.log(0.9), np.log(0.1 / (N - 1))
    x = np.full((T, B, N), miss, np.float32)
    lens = np.zeros(B, np.int64)
    for b in range(B):
        h, t = lm.start, 0
        while True:
            lo, hi = int(lm.row[h]), int(lm.row[h + 1])
            p = np.exp(lm.logp[lo:hi] - lm.logp[lo:hi].max())
            k = lo + int(rng.choice(hi - lo, p=p / p.sum()))
            toks = spellings[int(lm.word[k])] + [N - 1]
            durs = rng.integers(3, 7, len(toks))
            if t + int(durs.sum()) > T:
                break
            for tok, d in zip(toks, durs):
                x[t:t + d, b, tok] = hit
                t += int(d)
            h = int(lm.next[k])
        lens[b] = t
    x += rng.normal(0.0, sigma, x.shape).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(lens)


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "16,64,256,1024").split(",")]
    gain_beams = [int(v) for v in os.environ.get("GAIN_BEAMS", "8,16,32,64,128,256").split(",")]
    n = int(os.environ.get("CALLS", "5"))
    utts = int(os.environ.get("UTTS", "256"))
    sigmas = [float(v) for v in os.environ.get("SIGMA", "2.0,3.0").split(",")]
    seed = int(os.environ.get("SEED", "0"))
    for T, B, N, words, succ in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        lex = make_lexicon(N, words)
        lm = make_bigram(words, succ)
        las = {order: torch_asg_amd.WordLookahead(lex, lm, order) for order in (1, 2)}
        la = las[2]
        print("T=%d B=%d N=%d words=%d S=%d H=%d A=%d ranked arcs=%d levels=%d table bytes (fp32)=%d calls=%d" % (
            T, B, N, words, lex.graph.S, lm.H, lm.A, la.A, la.levels, (la.A * la.levels + la.S) * 4, n), flush=True)
        print(" table 1: time per call", flush=True)
        for K in beams:
            base = None
            for name, kw in (("plain", {}), ("order 1", dict(lookahead=las[1])), ("order 2", dict(lookahead=las[2]))):
                fn = lambda: torch_asg_amd.beam_decode_words(x, tr, lex, lm, il, K, max_work_bytes=WHOLE, **kw)      # noqa: E731
                med, lo, hi = calls(fn, n)
                base = med if base is None else base
                print("  K=%-5d %-8s %10.1f us (%10.1f .. %10.1f)  %8.2f us per frame  x%.2f" % (
                    K, name, med, lo, hi, med / T, med / base), flush=True)
        spellings = [None] * words                                          # word id -> tokens, read back from the trie
        nxt = np.asarray(lex.graph.next)
        stack = [(0, [])]
        while stack:
            node, toks = stack.pop()
            if lex.word_of_state[node] >= 0:
                spellings[int(lex.word_of_state[node])] = toks
            stack.extend((int(nxt[node, t]), toks + [int(t)]) for t in np.flatnonzero(nxt[node] >= 0) if t != N - 1)
        zero = torch.zeros(N, N, device=DEV)
        for sigma in sigmas:
            xs, ls = sample_utterances(lm, spellings, T, utts, N, sigma, seed)
            xs, ls = xs.to(DEV), ls.to(DEV)
            ref = torch_asg_amd.beam_decode_words(xs, zero, lex, lm, ls, 4096)
            print(" table 2: share of %d utterances whose words equal those of the plain search at K=4096; sigma=%.2f seed=%d, "
                  "transitions 0, %.1f words per utterance, yardstick finite %d" % (
                      utts, sigma, seed, float(ref.word_lengths.double().mean()), int(torch.isfinite(ref.scores).sum())), flush=True)
            for K in gain_beams:
                shares = []
                for kw in ({}, dict(lookahead=las[1]), dict(lookahead=las[2])):
                    out = torch_asg_amd.beam_decode_words(xs, zero, lex, lm, ls, K, **kw)
                    shares.append(float((out.words == ref.words).all(1).double().mean()))
                print("  K=%-5d plain %.3f   order 1 %.3f   order 2 %.3f" % (K, *shares), flush=True)


if __name__ == "__main__":
    main()
