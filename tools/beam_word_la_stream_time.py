#!/usr/bin/env python3
"""Developer probe: what LM look-ahead (torch_asg_amd.WordLookahead) costs in the streaming lexicon + word-LM beam decoder
(torch_asg_amd.BeamWordStream(..., lookahead=)), measured with device events after two warm-up samples: the median and the
spread (min .. max) of CALLS timed samples.  Per batch size and beam, first without look-ahead (the kernels as they were: the
baseline), then with order 1 and with order 2, all in one session:
  advance    a chunk of Tc = 8 and of Tc = 40 frames in mid-stream (behind 40 consumed frames);
  10 chunks  ten advances of Tc = 40 from a fresh state, timed as one block; the ratio to the baseline's block is what DESIGN.md
             section 5s holds against table 1 of section 5r;
  result     result(final=True) at pos = 40 and at pos = 400;
  one-shot   ONE beam_decode_words with the same look-ahead over the same 400 frames.
Every sample starts from a state prepared outside the timed region (reset, and the frames before the measured call).  The stream's
final result is held to the one-shot decode of the same look-ahead before a line is trusted.

    python tools/beam_word_la_stream_time.py [B,N,words,successors ...]   (default: the shapes DESIGN.md section 5s reports)
    BEAMS=64,256 CALLS=7                                                  (environment)

Lexicon and bigram are the synthetic ones of tools/beam_word_time.py; emissions are log-softmax of N(0,1); float32, max_frames 400.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from beam_stream_time import DEV, T, sample  # noqa: E402
from beam_word_time import make_bigram, make_lexicon  # noqa: E402

SHAPES = [(1, 40, 20000, 50), (64, 40, 20000, 50)]


def median(prepare, fn, n):
    """-> (median, min, max) in us of n samples, after two warm-up samples."""
    sample(prepare, fn)
    sample(prepare, fn)
    ts = [sample(prepare, fn) for _ in range(n)]
    return statistics.median(ts), min(ts), max(ts)


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256").split(",")]
    n = int(os.environ.get("CALLS", "7"))
    made = {}
    for B, N, words, succ in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        if (N, words, succ) not in made:
            lex, lm = make_lexicon(N, words), make_bigram(words, succ)
            made[(N, words, succ)] = (lex, lm, {order: torch_asg_amd.WordLookahead(lex, lm, order) for order in (1, 2)})
        lex, lm, las = made[(N, words, succ)]
        nothing = lambda: None                                                        # noqa: E731
        for K in beams:
            print("B=%d N=%d words=%d H=%d A=%d K=%d T=%d calls=%d" % (B, N, words, lm.H, lm.A, K, T, n), flush=True)
            base = {}
            for name, la in (("plain", None), ("order 1", las[1]), ("order 2", las[2])):
                s = torch_asg_amd.BeamWordStream(tr, lex, lm, B, T, K, lookahead=la)

                def at(pos):
                    def prepare():
                        s.reset()
                        for t0 in range(0, pos, 40):
                            s.advance(x[t0:t0 + 40])
                    return prepare

                def ten():
                    for t0 in range(0, T, 40):
                        s.advance(x[t0:t0 + 40])
                one = lambda: torch_asg_amd.beam_decode_words(x, tr, lex, lm, il, K, max_work_bytes=1 << 40,        # noqa: E731
                                                              lookahead=la)
                rows = [("advance Tc=8", at(40), lambda: s.advance(x[40:48])),
                        ("advance Tc=40", at(40), lambda: s.advance(x[40:80])),
                        ("10 chunks of 40", s.reset, ten)]
                for what, prepare, fn in rows:
                    med, lo, hi = median(prepare, fn, n)
                    base.setdefault(what, med)
                    print("  %-8s %-16s %10.1f (%10.1f .. %10.1f) us  x%.2f" % (name, what, med, lo, hi, med / base[what]), flush=True)
                for pos in (40, 400):
                    at(pos)()
                    what = "result pos=%d" % pos
                    med, lo, hi = median(nothing, lambda: s.result(final=True), n)
                    base.setdefault(what, med)
                    print("  %-8s %-16s %10.1f (%10.1f .. %10.1f) us  x%.2f" % (name, what, med, lo, hi, med / base[what]), flush=True)
                med, lo, hi = median(nothing, one, n)
                base.setdefault("one-shot", med)
                print("  %-8s %-16s %10.1f (%10.1f .. %10.1f) us  x%.2f" % (name, "one-shot T=400", med, lo, hi, med / base["one-shot"]),
                      flush=True)
                a, b = s.result(final=True), one()                                    # (the state holds all 400 frames)
                assert torch.equal(a.scores, b.scores) and torch.equal(a.words, b.words), "the stream and the one-shot decode differ"


if __name__ == "__main__":
    main()
