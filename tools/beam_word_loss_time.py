#!/usr/bin/env python3
"""Developer probe: per-call time of the beam-pruned loss over pairs (torch_asg_amd.beam_words_full_score, forward and
forward+backward with the target forced in) next to beam_decode_words at the same beam in the same session -- the ratio is the
cost of the lattice passes on top of the search they share.  Device events after two warm-up calls: the median and the spread
(min .. max) of CALLS single calls.

    python tools/beam_word_loss_time.py [T,B,N,words,successors ...]   (default: the shape DESIGN.md section 5t reports)
    BEAMS=64,256,1024 CALLS=5                                           (environment)

Lexicon, bigram and emissions are those of tools/beam_word_time.py; the targets are random words of the lexicon, each closed by
the separator, up to 60 labels per utterance.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from beam_word_time import calls, make_bigram, make_spellings  # noqa: E402

DEV = "cuda:0"
SHAPES = [(400, 64, 40, 20000, 50)]
S = 60


def make_targets(lex_words, N, B, seed=0):
    rng = np.random.default_rng(seed)
    tg = np.zeros((B, S), np.int64)
    tl = np.zeros(B, np.int64)
    for b in range(B):
        out = []
        while True:
            w = lex_words[int(rng.integers(len(lex_words)))]
            if len(out) + len(w) + 1 > S:
                break
            out += list(w) + [N - 1]
        tg[b, :len(out)], tl[b] = out, len(out)
    return torch.from_numpy(tg).to(DEV), torch.from_numpy(tl).to(DEV)


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256,1024").split(",")]
    n = int(os.environ.get("CALLS", "5"))
    whole = 1 << 40                                                       # one group
    for T, B, N, words, succ in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV).requires_grad_(True)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV).requires_grad_(True)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        lex_words = make_spellings(N, words)                                  # the lexicon of tools/beam_word_time.py
        lex = torch_asg_amd.Lexicon(lex_words, N, N - 1)
        lm = make_bigram(words, succ)
        tg, tl = make_targets(lex_words, N, B)
        print("T=%d B=%d N=%d words=%d S=%d H=%d A=%d target labels %.1f calls=%d" % (
            T, B, N, words, lex.graph.S, lm.H, lm.A, float(tl.double().mean()), n), flush=True)
        for K in beams:
            def decode():
                return torch_asg_amd.beam_decode_words(x.detach(), tr.detach(), lex, lm, il, K, max_work_bytes=whole)

            def fwd():
                with torch.no_grad():
                    return torch_asg_amd.beam_words_full_score(x, tr, lex, lm, il, K, targets=tg, target_lengths=tl,
                                                               max_work_bytes=whole)

            def step():
                x.grad = tr.grad = None
                torch_asg_amd.beam_words_full_score(x, tr, lex, lm, il, K, targets=tg, target_lengths=tl,
                                                    max_work_bytes=whole).sum().backward()
            base, lo, hi = calls(decode, n)
            print("  K=%-5d beam_decode_words      %9.1f us (%9.1f .. %9.1f)" % (K, base, lo, hi), flush=True)
            for name, fn in (("loss forward", fwd), ("loss forward+backward", step)):
                med, lo, hi = calls(fn, n)
                print("  K=%-5d %-22s %9.1f us (%9.1f .. %9.1f)  x%.2f" % (K, name, med, lo, hi, med / base), flush=True)
            Z = fwd()
            walk = torch_asg_amd.asg.native().words_target_scores(x.detach(), tr.detach(), lex, lm, tg, tl)
            print("  K=%-5d finite Z %d/%d, accepted targets %d/%d" % (K, int(torch.isfinite(Z).sum()), B,
                                                                        int(torch.isfinite(walk).sum()), B), flush=True)


if __name__ == "__main__":
    main()
