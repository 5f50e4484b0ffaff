#!/usr/bin/env python3
"""Developer probe: what taking the sets of the beam-pruned loss over pairs from a LOOK-AHEAD search costs and what it buys
(torch_asg_amd.beam_words_full_score(..., lookahead=)).

Price: per beam, forward and forward+backward with the target forced in -- the plain loss first (the baseline: it runs the
kernels it ran before the keyword existed), then the look-ahead of order 1 and 2 -- in one session.  Device events after two
warm-up calls: the median and the spread (min .. max) of CALLS single calls, and the ratio to the plain loss at the same beam.

What it buys: the mean over the batch of Z_WIDE(plain) - Z_K for the three forms, WIDE = 1024: how far the narrow lattice's
normaliser is from the wide one's.  The gap is >= 0 only for the plain K, whose sets nest in the wide beam's; a look-ahead lattice
may hold pairs the plain wide beam dropped.  The work bytes of one call (alpha stored) are printed per beam.

    python tools/beam_word_la_loss_time.py [T,B,N,words,successors ...]   (default: the shape DESIGN.md section 5u reports)
    BEAMS=64,256 WIDE=1024 CALLS=5                                         (environment)

Lexicon, bigram, emissions and targets are those of tools/beam_word_loss_time.py.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from beam_word_loss_time import DEV, SHAPES, make_targets  # noqa: E402
from beam_word_time import calls, make_bigram, make_spellings  # noqa: E402

WHOLE = 1 << 40                                                               # one group


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256").split(",")]
    wide = int(os.environ.get("WIDE", "1024"))
    n = int(os.environ.get("CALLS", "5"))
    be = torch_asg_amd.asg.native()
    for T, B, N, words, succ in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV).requires_grad_(True)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV).requires_grad_(True)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        lex_words = make_spellings(N, words)
        lex = torch_asg_amd.Lexicon(lex_words, N, N - 1)
        lm = make_bigram(words, succ)
        tg, tl = make_targets(lex_words, N, B)
        forms = (("plain", {}), ("order 1", dict(lookahead=torch_asg_amd.WordLookahead(lex, lm, 1))),
                 ("order 2", dict(lookahead=torch_asg_amd.WordLookahead(lex, lm, 2))))
        print("T=%d B=%d N=%d words=%d S=%d H=%d A=%d target labels %.1f calls=%d" % (
            T, B, N, words, lex.graph.S, lm.H, lm.A, float(tl.double().mean()), n), flush=True)

        def score(K, kw, grad):
            with torch.set_grad_enabled(grad):
                return torch_asg_amd.beam_words_full_score(x, tr, lex, lm, il, K, targets=tg, target_lengths=tl,
                                                           max_work_bytes=WHOLE, **kw)
        z_wide = score(wide, {}, False).double()
        print(" Z_%d(plain): finite %d/%d, mean %.3f" % (wide, int(torch.isfinite(z_wide).sum()), B, float(z_wide.mean())), flush=True)
        for K in beams:
            base = {}
            for name, kw in forms:
                def fwd():
                    return score(K, kw, False)

                def step():
                    x.grad = tr.grad = None
                    score(K, kw, True).sum().backward()
                seen = []
                buf = be._buf
                be._buf = lambda nbytes, d: (seen.append(nbytes), buf(nbytes, d))[1]
                try:
                    step()
                finally:
                    del be._buf
                for what, fn in (("forward", fwd), ("forward+backward", step)):
                    med, lo, hi = calls(fn, n)
                    base.setdefault(what, med)
                    print("  K=%-5d %-8s %-17s %9.1f us (%9.1f .. %9.1f)  x%.2f of plain" % (
                        K, name, what, med, lo, hi, med / base[what]), flush=True)
                Z = fwd().double()
                print("  K=%-5d %-8s finite Z %d/%d, mean Z_%d(plain) - Z_K = %.4f (min %.4f, max %.4f), work bytes %d" % (
                    K, name, int(torch.isfinite(Z).sum()), B, wide, float((z_wide - Z).mean()), float((z_wide - Z).min()),
                    float((z_wide - Z).max()), max(seen)), flush=True)


if __name__ == "__main__":
    main()
