#!/usr/bin/env python3
"""Developer probe: per-call time of the word confidences (torch_asg_amd.beam_decode_words_confidence) next to the calls whose
kernels it is built from, at the same beam in the same session: beam_decode_words (the search it runs once) and
beam_words_full_score without targets, forward and forward+backward (the lattice passes; the confidence call replaces that
backward by a beta pass without label posteriors and (i, j) counts).  Device events after two warm-up calls: the median and the
spread (min .. max) of CALLS single calls.

    python tools/beam_word_conf_time.py [T,B,N,words,successors ...]   (default: the shape DESIGN.md section 5x reports)
    BEAMS=64,256,1024 LA_BEAMS=64,256 CALLS=5                           (environment)

Lexicon, bigram and emissions are those of tools/beam_word_time.py.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from beam_word_time import calls, make_bigram, make_spellings  # noqa: E402

DEV = "cuda:0"
SHAPES = [(400, 64, 40, 20000, 50)]


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256,1024").split(",")]
    la_beams = [int(v) for v in os.environ.get("LA_BEAMS", "64,256").split(",")]
    n = int(os.environ.get("CALLS", "5"))
    whole = 1 << 40                                                       # one group
    for T, B, N, words, succ in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV).requires_grad_(True)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV).requires_grad_(True)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        lex = torch_asg_amd.Lexicon(make_spellings(N, words), N, N - 1)       # the lexicon of tools/beam_word_time.py
        lm = make_bigram(words, succ)
        la = torch_asg_amd.WordLookahead(lex, lm, 2)
        print("T=%d B=%d N=%d words=%d S=%d H=%d A=%d calls=%d" % (T, B, N, words, lex.graph.S, lm.H, lm.A, n), flush=True)
        for K in beams:
            def decode():
                return torch_asg_amd.beam_decode_words(x.detach(), tr.detach(), lex, lm, il, K, max_work_bytes=whole)

            def fwd():
                with torch.no_grad():
                    return torch_asg_amd.beam_words_full_score(x, tr, lex, lm, il, K, max_work_bytes=whole)

            def step():
                x.grad = tr.grad = None
                torch_asg_amd.beam_words_full_score(x, tr, lex, lm, il, K, max_work_bytes=whole).sum().backward()

            def conf(tol, look=None):
                return lambda: torch_asg_amd.beam_decode_words_confidence(x.detach(), tr.detach(), lex, lm, il, K, frame_tolerance=tol,
                                                                          max_work_bytes=whole, lookahead=look)
            base, lo, hi = calls(decode, n)
            print("  K=%-5d beam_decode_words        %9.1f us (%9.1f .. %9.1f)" % (K, base, lo, hi), flush=True)
            rows = [("score forward", fwd), ("score forward+backward", step), ("confidence tol=0", conf(0)), ("confidence tol=3", conf(3))]
            if K in la_beams:
                rows += [("confidence tol=0 order 2", conf(0, la)), ("confidence tol=3 order 2", conf(3, la))]
            for name, fn in rows:
                med, lo, hi = calls(fn, n)
                print("  K=%-5d %-24s %9.1f us (%9.1f .. %9.1f)  x%.2f" % (K, name, med, lo, hi, med / base), flush=True)
            r = conf(0)()
            nw = r.word_lengths.double()
            c = r.word_confidences[r.word_frames >= 0].double()
            print("  K=%-5d finite Z %d/%d, words per utterance %.1f, mean confidence %.3f, below 0.5: %.1f%%" % (
                K, int(torch.isfinite(r.normalisers).sum()), B, float(nw.mean()), float(c.mean()) if c.numel() else 0.0,
                100.0 * float((c < 0.5).double().mean()) if c.numel() else 0.0), flush=True)


if __name__ == "__main__":
    main()
