#!/usr/bin/env python3
"""Developer probe: what keeping the lattice costs a word-LM beam stream, and what a confidence from it costs
(BeamWordStream(..., keep_lattice=True).result_confidence), next to the two yardsticks of the same session that are older code:
the plain word stream's `advance` and the one-shot `beam_decode_words_confidence`.  Device events after two warm-ups: the median
and the spread (min .. max) of CALLS timed samples.  Per beam and tolerance (and, at LA_BEAMS, once more with an order-2
look-ahead), in this order:
  advance plain      a plain BeamWordStream's advance of 40 frames from a fresh state: the yardstick for the cost of keeping the
                     lattice;
  advance lattice    the lattice-keeping stream's advance of the same 40 frames;
  conf pos=40/400    result_confidence(tol) with every frame to catch up (the state prepared outside the timed region) and caught
                     up (a second call), prefix mode;
  10 + conf          ten advances of 40 frames from a fresh state plus one result_confidence(tol, final=True), timed as one block,
                     against ONE beam_decode_words_confidence over the same 400 frames: the yardstick.
The last two are also compared bit for bit.

    python tools/beam_word_stream_conf_time.py [T,B,N,words,successors ...]   (default: the workload of DESIGN.md 5n / 5x / 5ae)
    BEAMS=64,256 LA_BEAMS=64 TOLS=0,3 CALLS=5                                 (environment)

Lexicon, bigram and emissions are those of tools/beam_word_time.py.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from beam_stream_time import calls  # noqa: E402
from beam_word_time import make_bigram, make_spellings  # noqa: E402

DEV = "cuda:0"
SHAPES = [(400, 64, 40, 20000, 50)]
TC = 40
FIELDS = ("scores", "tokens", "token_lengths", "words", "word_lengths", "word_frames", "word_confidences", "normalisers")


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256").split(",")]
    la_beams = [int(v) for v in os.environ.get("LA_BEAMS", "64").split(",") if v]
    tols = [int(v) for v in os.environ.get("TOLS", "0,3").split(",")]
    n = int(os.environ.get("CALLS", "5"))
    nothing = lambda: None                                                            # noqa: E731
    for T, B, N, words, succ in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        lex = torch_asg_amd.Lexicon(make_spellings(N, words), N, N - 1)
        lm = make_bigram(words, succ)
        look = torch_asg_amd.WordLookahead(lex, lm, 2)
        print("T=%d B=%d N=%d words=%d S=%d H=%d A=%d chunk=%d calls=%d" % (T, B, N, words, lex.graph.S, lm.H, lm.A, TC, n), flush=True)
        for K, la in [(K, None) for K in beams] + [(K, look) for K in la_beams]:
            tag = "K=%-4d%s" % (K, "" if la is None else " order 2")
            plain = torch_asg_amd.BeamWordStream(tr, lex, lm, B, T, K, lookahead=la)
            s = torch_asg_amd.BeamWordStream(tr, lex, lm, B, T, K, lookahead=la, keep_lattice=True)
            print("  %s state bytes: plain %d, lattice %d" % (tag, plain._state.numel(), s._state.numel()), flush=True)
            print("  %s advance plain    40 frames       %s" % (tag, calls(plain.reset, lambda: plain.advance(x[:TC]), n)), flush=True)
            print("  %s advance lattice  40 frames       %s" % (tag, calls(s.reset, lambda: s.advance(x[:TC]), n)), flush=True)

            def feed(frames):
                def go():
                    s.reset()
                    for t0 in range(0, frames, TC):
                        s.advance(x[t0:t0 + TC])
                return go
            for tol in tols:
                for frames in (TC, T):
                    fn = lambda: s.result_confidence(tol)                             # noqa: E731
                    print("  %s tol=%d conf pos=%-3d catch-up all  %s" % (tag, tol, frames, calls(feed(frames), fn, n)), flush=True)
                    print("  %s tol=%d conf pos=%-3d caught up     %s" % (tag, tol, frames, calls(nothing, fn, n)), flush=True)

                def ten():
                    for t0 in range(0, T, TC):
                        s.advance(x[t0:t0 + TC])
                    return s.result_confidence(tol, final=True)
                one = lambda: torch_asg_amd.beam_decode_words_confidence(x, tr, lex, lm, il, K, frame_tolerance=tol,     # noqa: E731
                                                                         max_work_bytes=1 << 40, lookahead=la)
                print("  %s tol=%d 10 chunks of 40 + conf      %s" % (tag, tol, calls(s.reset, ten, n)), flush=True)
                print("  %s tol=%d one-shot confidence T=400   %s" % (tag, tol, calls(nothing, one, n)), flush=True)
                s.reset()
                a, b = ten(), one()
                for f in FIELDS:
                    assert torch.equal(getattr(a, f), getattr(b, f)), f
                nw = a.word_lengths.double()
                cf = a.word_confidences[a.word_frames >= 0].double()
                print("  %s tol=%d bit-equal to the one-shot call; finite Z %d/%d, words per utterance %.1f, mean confidence "
                      "%.3f" % (tag, tol, int(torch.isfinite(a.normalisers).sum()), B, float(nw.mean()),
                                float(cf.mean()) if cf.numel() else 0.0), flush=True)


if __name__ == "__main__":
    main()
