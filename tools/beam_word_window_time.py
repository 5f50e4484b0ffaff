#!/usr/bin/env python3
"""Developer probe: per-call times of windowed streaming beam decoding with a lexicon and a word LM
(torch_asg_amd.BeamWordWindowStream) next to the unbounded word stream (BeamWordStream, max_frames = 400) of the same session --
the yardstick is the parent's kernel, not the code under test.  The method of tools/beam_word_stream_time.py: device events
around single calls after two warm-ups, the median and the spread (min .. max) of CALLS timed samples, state prepared outside
the timed region.  Per batch size and beam:
  10 chunks  ten advances of Tc = 40 from a fresh state, timed as one block, at W = 128, P = 32; the same ten calls of BeamWordStream;
  result     result(final=True) at pos = 40 and at pos = 400, for both: the window's backtrace is at most W steps whatever pos;
  idle       an advance whose chunk_lengths are all 0: the fixed cost of a call (launch, the header, the padding of the outputs).
It prints the back-pointer bytes per slot of both streams and checks that both end with the same score.

    python tools/beam_word_window_time.py [B,N,words,successors ...]   (default: the shapes DESIGN.md section 5q reports)
    BEAMS=64,256 CALLS=7 WINDOW=128 EVERY=32                           (environment)

Lexicon and bigram are the synthetic ones of tools/beam_word_time.py; emissions are log-softmax of N(0,1); float32.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from beam_stream_time import DEV, T, calls  # noqa: E402
from beam_word_time import make_bigram, make_lexicon  # noqa: E402

SHAPES = [(1, 40, 20000, 50), (64, 40, 20000, 50)]


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256").split(",")]
    n = int(os.environ.get("CALLS", "7"))
    W, P = int(os.environ.get("WINDOW", "128")), int(os.environ.get("EVERY", "32"))
    made = {}
    for B, N, words, succ in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        zero = torch.zeros(B, dtype=torch.int64, device=DEV)
        if (N, words, succ) not in made:
            made[(N, words, succ)] = (make_lexicon(N, words), make_bigram(words, succ))
        lex, lm = made[(N, words, succ)]
        for K in beams:
            print("B=%d N=%d words=%d H=%d A=%d K=%d T=%d W=%d P=%d" % (B, N, words, lm.H, lm.A, K, T, W, P), flush=True)
            win = torch_asg_amd.BeamWordWindowStream(tr, lex, lm, B, W, P, K)
            un = torch_asg_amd.BeamWordStream(tr, lex, lm, B, T, K)
            print("  back-pointers per slot: window %d bytes, unbounded %d bytes" % (3 * W * K * 4, 3 * T * K * 4), flush=True)
            nothing = lambda: None                                                    # noqa: E731
            for name, s in (("window   ", win), ("unbounded", un)):
                def at(pos, s=s):
                    def prepare():
                        s.reset()
                        for t0 in range(0, pos, 40):
                            s.advance(x[t0:t0 + 40])
                    return prepare

                def ten(s=s):
                    for t0 in range(0, T, 40):
                        s.advance(x[t0:t0 + 40])
                print("  %s 10 chunks of 40   %s" % (name, calls(s.reset, ten, n)), flush=True)
                for pos in (40, 400):
                    at(pos)()
                    print("  %s result pos=%-3d    %s" % (name, pos, calls(nothing, lambda s=s: s.result(final=True), n)), flush=True)
                print("  %s idle (lengths 0)  %s" % (name, calls(at(40), lambda s=s: s.advance(x[40:80], zero), n)), flush=True)
            a, b = win.result(final=True), un.result(final=True)
            assert torch.equal(a.scores, b.scores), "the window stream and the unbounded stream differ"
            print("  committed %s of %d frames, status %s" % (a.committed.tolist()[:4], T, a.status.tolist()[:4]), flush=True)


if __name__ == "__main__":
    main()
