#!/usr/bin/env python3
"""Developer probe: per-call time of the n-best word confidences (torch_asg_amd.beam_decode_words_nbest_confidence) next to the
calls it replaces, at the same beam in the same session: beam_decode_words, beam_decode_words_confidence (one-best) and
beam_decode_words_nbest at nbest 1 / 10 / 100 first, then the new call at nbest 1 / 10 / 100 with tolerance 0 and 3, then with
order-2 look-ahead at nbest 10.  Device events after two warm-up calls: the median and the spread (min .. max) of CALLS single
calls.  Per beam it also prints the cells per utterance (distinct (frame, word) among the rows' words) and how many of the word
filter's 256 bits an utterance sets: an event whose word is in no row passes the filter with about that share.

    python tools/beam_word_nbest_conf_time.py [T,B,N,words,successors ...]   (default: the shape DESIGN.md section 5y reports)
    BEAMS=64,256 CALLS=5                                                      (environment)

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
NBEST = (1, 10, 100)


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256").split(",")]
    n = int(os.environ.get("CALLS", "5"))
    whole = 1 << 40                                                       # one group
    for T, B, N, words, succ in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        lex = torch_asg_amd.Lexicon(make_spellings(N, words), N, N - 1)       # the lexicon of tools/beam_word_time.py
        lm = make_bigram(words, succ)
        la = torch_asg_amd.WordLookahead(lex, lm, 2)
        print("T=%d B=%d N=%d words=%d S=%d H=%d A=%d calls=%d" % (T, B, N, words, lex.graph.S, lm.H, lm.A, n), flush=True)
        for K in beams:
            def decode():
                return torch_asg_amd.beam_decode_words(x, tr, lex, lm, il, K, max_work_bytes=whole)

            def conf():
                return torch_asg_amd.beam_decode_words_confidence(x, tr, lex, lm, il, K, max_work_bytes=whole)

            def nbest(nb, look=None):
                return lambda: torch_asg_amd.beam_decode_words_nbest(x, tr, lex, lm, il, K, nb, max_work_bytes=whole, lookahead=look)

            def new(nb, tol, look=None):
                return lambda: torch_asg_amd.beam_decode_words_nbest_confidence(x, tr, lex, lm, il, K, nb, frame_tolerance=tol,
                                                                                max_work_bytes=whole, lookahead=look)
            base, lo, hi = calls(decode, n)
            print("  K=%-5d beam_decode_words               %9.1f us (%9.1f .. %9.1f)" % (K, base, lo, hi), flush=True)
            rows = [("confidence (one best) tol=0", conf)]
            rows += [("nbest %d" % nb, nbest(nb)) for nb in NBEST]
            rows += [("nbest confidence %d tol=%d" % (nb, tol), new(nb, tol)) for nb in NBEST for tol in (0, 3)]
            rows += [("nbest 10 order 2", nbest(10, la)), ("nbest confidence 10 tol=0 order 2", new(10, 0, la))]
            for name, fn in rows:
                med, lo, hi = calls(fn, n)
                print("  K=%-5d %-31s %9.1f us (%9.1f .. %9.1f)  x%.2f" % (K, name, med, lo, hi, med / base), flush=True)
            for nb in NBEST:
                r = new(nb, 0)()
                f, w = r.word_frames.cpu(), r.words.cpu()
                cells, bits, queries = [], [], []
                for b in range(B):
                    m = f[b] >= 0
                    cs = set(zip(f[b][m].tolist(), w[b][m].tolist()))
                    cells.append(len(cs))
                    bits.append(len({wd % 256 for _, wd in cs}))
                    queries.append(int(m.sum()))
                c = r.word_confidences[r.word_frames >= 0].double()
                print("  K=%-5d nbest %-3d rows %.1f, queries %.1f, cells %.1f (max %d), filter bits set %.1f / 256 (%.0f%% of foreign "
                      "events turned away), mean confidence %.3f" % (
                          K, nb, float(r.num_hyps.double().mean()), sum(queries) / B, sum(cells) / B, max(cells), sum(bits) / B,
                          100.0 * (1.0 - sum(bits) / B / 256.0), float(c.mean()) if c.numel() else 0.0), flush=True)


if __name__ == "__main__":
    main()
