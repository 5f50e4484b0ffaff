#!/usr/bin/env python3
"""Developer probe: per-call times of streaming beam decoding with a lexicon and a word LM (torch_asg_amd.BeamWordStream) next to
the one-shot decoder (beam_decode_words) of the same session, measured with device events after a warm-up: the median and the
spread (min .. max) of CALLS timed samples.  Per batch size and beam:
  advance    a chunk of Tc = 8 and of Tc = 40 frames in mid-stream (behind 40 consumed frames), eager and replayed from a hipGraph;
  idle       an advance whose chunk_lengths are all 0: the fixed cost of a call (launch, the header);
  result     result(final=True) at pos = 40 and at pos = 400: the backtrace is one dependent-load chain of pos steps;
  10 chunks  ten advances of Tc = 40 from a fresh state, timed as one block, against ONE beam_decode_words over the same 400
             frames -- the yardstick is the one-shot call, not the stream's own numbers.  The expectation to confirm or refute:
             the ten advances stay within ten fixed-cost calls of the one-shot time.
Every sample starts from a state prepared outside the timed region (reset, and the frames before the measured call).

    python tools/beam_word_stream_time.py [B,N,words,successors ...]   (default: the shapes DESIGN.md section 5o reports)
    BEAMS=64,256 CALLS=9                                               (environment)

Lexicon and bigram are the synthetic ones of tools/beam_word_time.py; emissions are log-softmax of N(0,1); float32, max_frames 400.
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
    n = int(os.environ.get("CALLS", "9"))
    made = {}
    for B, N, words, succ in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        zero = torch.zeros(B, dtype=torch.int64, device=DEV)
        if (N, words, succ) not in made:
            made[(N, words, succ)] = (make_lexicon(N, words), make_bigram(words, succ))
        lex, lm = made[(N, words, succ)]
        for K in beams:
            print("B=%d N=%d words=%d H=%d A=%d K=%d T=%d" % (B, N, words, lm.H, lm.A, K, T), flush=True)
            s = torch_asg_amd.BeamWordStream(tr, lex, lm, B, T, K)
            nothing = lambda: None                                                    # noqa: E731

            def at(pos):
                def prepare():
                    s.reset()
                    for t0 in range(0, pos, 40):
                        s.advance(x[t0:t0 + 40])
                return prepare
            for Tc in (8, 40):
                chunk = x[40:40 + Tc].contiguous()
                adv = lambda: s.advance(chunk)                                        # noqa: E731
                print("  advance Tc=%-3d eager  %s" % (Tc, calls(at(40), adv, n)), flush=True)
                at(40)()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    s.advance(chunk)
                print("  advance Tc=%-3d graph  %s" % (Tc, calls(at(40), gr.replay, n)), flush=True)
            print("  idle (lengths 0) eager %s" % calls(at(40), lambda: s.advance(x[40:80], zero), n), flush=True)
            for pos in (40, 400):
                at(pos)()
                print("  result pos=%-3d        %s" % (pos, calls(nothing, lambda: s.result(final=True), n)), flush=True)

            def ten():
                for t0 in range(0, T, 40):
                    s.advance(x[t0:t0 + 40])
            print("  10 chunks of 40       %s" % calls(s.reset, ten, n), flush=True)
            one = lambda: torch_asg_amd.beam_decode_words(x, tr, lex, lm, il, K, max_work_bytes=1 << 40)      # noqa: E731
            print("  one-shot T=400        %s" % calls(nothing, one, n), flush=True)
            a, b = s.result(final=True), one()
            assert torch.equal(a.scores, b.scores) and torch.equal(a.words, b.words), "the stream and the one-shot decode differ"


if __name__ == "__main__":
    main()
