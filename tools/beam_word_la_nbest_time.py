#!/usr/bin/env python3
"""Developer probe: per-call time of the n-best over pairs WITH LM look-ahead (torch_asg_amd.beam_decode_words_nbest(...,
lookahead=)) next to the one-best decoder with the same look-ahead (beam_decode_words(..., lookahead=), the baseline: its kernel
did not change) at the same beam in the same session, and next to the plain n-best at that beam.  Device events after a warm-up:
the median and the spread (min .. max) of CALLS single calls, and beside each row the time above the baseline -- the cost of the
n-best stage (the ends of the last set with their LM walks and one `look` per entry, the sort, one walk per hypothesis, tokens
and words).  Then the stream: BeamWordStream._result_nbest of a look-ahead stream at pos = T next to its result(final=True).

    python tools/beam_word_la_nbest_time.py [T,B,N,words,successors ...]   (default: the shape DESIGN.md section 5v reports)
    BEAMS=64,256 ORDERS=1,2 NBEST=1,10,100,K CALLS=9 ALIGN=0               (environment; K in NBEST stands for the beam size)

Lexicon, bigram and emissions are those of tools/beam_word_time.py.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from beam_word_time import calls, make_bigram, make_lexicon  # noqa: E402

DEV = "cuda:0"
SHAPES = [(400, 64, 40, 20000, 50)]


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256").split(",")]
    orders = [int(v) for v in os.environ.get("ORDERS", "1,2").split(",")]
    nbests = os.environ.get("NBEST", "1,10,100,K").split(",")
    n = int(os.environ.get("CALLS", "9"))
    align = os.environ.get("ALIGN", "0") == "1"
    whole = 1 << 40                                                       # one group
    for T, B, N, words, succ in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        lex = make_lexicon(N, words)
        lm = make_bigram(words, succ)
        print("T=%d B=%d N=%d words=%d H=%d A=%d alignments=%d calls=%d" % (T, B, N, words, lm.H, lm.A, align, n), flush=True)
        for K in beams:
            for order in orders:
                la = torch_asg_amd.WordLookahead(lex, lm, order)
                one = lambda: torch_asg_amd.beam_decode_words(x, tr, lex, lm, il, K, max_work_bytes=whole, lookahead=la)  # noqa: E731
                base, lo, hi = calls(one, n)
                print("  K=%-5d order %d beam_decode_words      %9.1f us (%9.1f .. %9.1f)" % (K, order, base, lo, hi), flush=True)
                for nb in nbests:
                    nb = K if nb == "K" else int(nb)
                    many = lambda: torch_asg_amd.beam_decode_words_nbest(x, tr, lex, lm, il, K, nb, return_alignments=align,   # noqa: E731
                                                                         max_work_bytes=whole, lookahead=la)
                    out = many()
                    med, lo, hi = calls(many, n)
                    print("  K=%-5d order %d nbest=%-5d             %9.1f us (%9.1f .. %9.1f)  above the one-best decoder %+9.1f us  "
                          "hypotheses per utterance %.1f" % (K, order, nb, med, lo, hi, med - base,
                                                             float(out.num_hyps.double().mean())), flush=True)
                s = torch_asg_amd.BeamWordStream(tr, lex, lm, B, T, K, lookahead=la)
                s.advance(x, il)
                sbase, lo, hi = calls(lambda: s.result(True), n)
                print("  K=%-5d order %d stream result at pos %d         %9.1f us (%9.1f .. %9.1f)" % (K, order, T, sbase, lo, hi),
                      flush=True)
                for nb in nbests:
                    nb = K if nb == "K" else int(nb)
                    med, lo, hi = calls(lambda: s._result_nbest(nb, True, align), n)
                    print("  K=%-5d order %d stream _result_nbest=%-5d      %9.1f us (%9.1f .. %9.1f)  above result %+9.1f us" % (
                        K, order, nb, med, lo, hi, med - sbase), flush=True)
                del s
            plain_one, lo, hi = calls(lambda: torch_asg_amd.beam_decode_words(x, tr, lex, lm, il, K, max_work_bytes=whole), n)
            print("  K=%-5d plain   beam_decode_words      %9.1f us (%9.1f .. %9.1f)" % (K, plain_one, lo, hi), flush=True)
            for nb in nbests:
                nb = K if nb == "K" else int(nb)
                med, lo, hi = calls(lambda: torch_asg_amd.beam_decode_words_nbest(x, tr, lex, lm, il, K, nb, return_alignments=align,
                                                                                  max_work_bytes=whole), n)
                print("  K=%-5d plain   nbest=%-5d             %9.1f us (%9.1f .. %9.1f)  above the one-best decoder %+9.1f us" % (
                    K, nb, med, lo, hi, med - plain_one), flush=True)


if __name__ == "__main__":
    main()
