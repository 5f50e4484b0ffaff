#!/usr/bin/env python3
"""Developer probe: per-call times of the n-best list of the windowed word-LM beam stream (BeamWordWindowStream.result_nbest) next
to the stream's own one-best result of the same session -- the yardstick is the parent's kernel, not the code under test.  The
method of tools/beam_stream_nbest_time.py: device events around single calls after two warm-ups, the median and the spread
(min .. max) of CALLS timed samples; the state is prepared once, outside the timed region (the calls only read it), and the scratch
of every nbest is allocated by the warm-ups.  Per batch size and beam, at W = 128, P = 32 and pos = 400:
  tail     the uncommitted frames pos - base of every slot (min / median / max), which is what a row walks;
  result   BeamWordWindowStream.result(final=True) and (final=False);
  nbest    result_nbest for nbest 1 / 10 / 100, final and prefix.
It checks that row 0 of the list has the score of `result`.

    python tools/beam_word_window_nbest_time.py [B,N,words,successors ...]   (default: the shapes DESIGN.md section 5ac reports)
    BEAMS=64,256 CALLS=9 WINDOW=128 EVERY=32                                 (environment)

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
    n = int(os.environ.get("CALLS", "9"))
    W, P = int(os.environ.get("WINDOW", "128")), int(os.environ.get("EVERY", "32"))
    made = {}
    nothing = lambda: None                                                            # noqa: E731
    for B, N, words, succ in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        if (N, words, succ) not in made:
            made[(N, words, succ)] = (make_lexicon(N, words), make_bigram(words, succ))
        lex, lm = made[(N, words, succ)]
        for K in beams:
            print("B=%d N=%d words=%d H=%d A=%d K=%d pos=%d W=%d P=%d" % (B, N, words, lm.H, lm.A, K, T, W, P), flush=True)
            win = torch_asg_amd.BeamWordWindowStream(tr, lex, lm, B, W, P, K)
            for t0 in range(0, T, 40):
                win.advance(x[t0:t0 + 40])
            one = win.result(final=True)
            tail = (one.frames - one.committed).sort().values
            print("  tail pos - base: min %d median %d max %d, status %s" % (int(tail[0]), int(tail[B // 2]), int(tail[-1]),
                                                                              sorted(set(one.status.tolist()))), flush=True)
            for final in (True, False):
                name = "final " if final else "prefix"
                print("  result    %s       %s" % (name, calls(nothing, lambda: win.result(final=final), n)), flush=True)
                for nb in (1, 10, 100):
                    fn = lambda: win.result_nbest(nb, final)                          # noqa: E731
                    print("  nbest=%-3d %s       %s" % (nb, name, calls(nothing, fn, n)), flush=True)
            lst = win.result_nbest(100, True)
            assert torch.equal(lst.scores[:, 0], one.scores), "row 0 and result differ"
            print("  num_hyps at nbest=100 final: min %d max %d" % (int(lst.num_hyps.min()), int(lst.num_hyps.max())), flush=True)


if __name__ == "__main__":
    main()
