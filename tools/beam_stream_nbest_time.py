#!/usr/bin/env python3
"""Developer probe: per-call times of the n-best lists of the two token-graph beam streams (BeamStream.result_nbest,
BeamWindowStream.result_nbest) next to the stream's own one-best result and to the one-shot n-best decoder of the same session,
measured with device events after two warm-ups: the median and the spread (min .. max) of CALLS timed samples.  Per shape and
beam, in this order:
  result       BeamStream.result(final=True) at pos = 400: the kernel the stream had before, the yardstick;
  nbest        BeamStream.result_nbest for nbest 1 / 10 / 100, final and prefix, at pos = 400;
  window       the same for BeamWindowStream with W = 128 at pos = 400 (its one-best result first);
  10 + nbest   ten advances of 40 frames from a fresh state plus one result_nbest(100, final=True), timed as one block, against
               ONE beam_decode_graph_nbest over the same 400 frames.
Every sample starts from a state prepared outside the timed region; the scratch of every nbest is allocated by the warm-ups.

    python tools/beam_stream_nbest_time.py [B,N,order ...]   (default: the shapes DESIGN.md section 5ab reports)
    BEAMS=64,256 CALLS=9                                     (environment)

order 1..4 is an n-gram from a random table, as tools/graph_decode_time.py makes it; emissions are log-softmax of N(0,1).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from beam_stream_time import calls  # noqa: E402
from graph_decode_time import make_graph  # noqa: E402

DEV = "cuda:0"
SHAPES = [(1, 40, 3), (64, 40, 3), (1, 40, 4), (64, 40, 4)]
T, W = 400, 128


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256").split(",")]
    n = int(os.environ.get("CALLS", "9"))
    graphs = {}
    nothing = lambda: None                                                            # noqa: E731
    for B, N, order in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        if (N, order) not in graphs:
            graphs[(N, order)] = make_graph(N, order)
        graph = graphs[(N, order)]
        Q = graph.compile(DEV, torch.float32, 1.0, 0.0)["Q"]
        for K in beams:
            print("B=%d N=%d order=%d Q=%d K=%d T=%d W=%d" % (B, N, order, Q, K, T, W), flush=True)
            s = torch_asg_amd.BeamStream(tr, graph, B, T, K)
            w = torch_asg_amd.BeamWindowStream(tr, graph, B, W, None, K)

            def feed(z):
                z.reset()
                for t0 in range(0, T, 40):
                    z.advance(x[t0:t0 + 40])
            for z, name in ((s, "stream"), (w, "window")):
                feed(z)
                print("  %s result pos=400             %s" % (name, calls(nothing, lambda: z.result(final=True), n)), flush=True)
                for final in (True, False):
                    for nb in (1, 10, 100):
                        fn = lambda: z.result_nbest(nb, final)                        # noqa: E731
                        print("  %s nbest=%-3d %s pos=400  %s" % (name, nb, "final " if final else "prefix", calls(nothing, fn, n)),
                              flush=True)

            def ten():
                for t0 in range(0, T, 40):
                    s.advance(x[t0:t0 + 40])
                return s.result_nbest(100, True)
            print("  10 chunks of 40 + nbest=100          %s" % calls(s.reset, ten, n), flush=True)
            one = lambda: torch_asg_amd.beam_decode_graph_nbest(x, tr, graph, il, K, 100, max_work_bytes=1 << 40)    # noqa: E731
            print("  one-shot nbest=100 T=400             %s" % calls(nothing, one, n), flush=True)
            s.reset()
            a, b = ten(), one()
            assert torch.equal(a.scores, b.scores) and torch.equal(a.graph_scores, b.graph_scores) and torch.equal(a.tokens, b.tokens)
            feed(w)
            assert torch.equal(w.result_nbest(100, True).scores, a.scores), "the window's scores and the stream's differ"


if __name__ == "__main__":
    main()
