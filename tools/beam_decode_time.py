#!/usr/bin/env python3
"""Developer probe: per-call time of beam-pruned decoding with a token automaton (torch_asg_amd.beam_decode_graph) next to the
exact decoder (viterbi_decode_graph) of the same session, eager and replayed from a hipGraph, measured with device events
after a warm-up; the workspace of each, and the share of utterances whose beam score equals the exact score.

    python tools/beam_decode_time.py [T,B,N,order ...]     (default: the shapes DESIGN.md section 5i reports)
    BEAMS=64,256,1024 THRESHOLD=inf                        (environment: the beam sizes and the threshold)

order 1..4 is an n-gram from a random table, as tools/graph_decode_time.py makes it; emissions are log-softmax of N(0,1).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from graph_decode_time import make_graph, timed  # noqa: E402

DEV = "cuda:0"
SHAPES = [(400, 64, 40, 3), (400, 64, 40, 4)]


def replayed(call, reps):
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        call()
    gr.replay()
    return timed(gr.replay, reps)


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256,1024").split(",")]
    theta = float(os.environ.get("THRESHOLD", "inf"))
    from torch_asg_amd.asg import native
    be = native()
    sizes = []
    buf = be._buf
    be._buf = lambda n, d: (sizes.append(int(n)), buf(n, d))[1]          # the workspace each call asks for
    for T, B, N, order in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        graph = make_graph(N, order)
        c = graph.compile(DEV, torch.float32, 1.0, 0.0)
        whole = 1 << 40                                                   # one group: the exact call's time is not split
        exact = lambda: torch_asg_amd.viterbi_decode_graph(x, tr, graph, il, max_work_bytes=whole)      # noqa: E731
        reps = 2 if c["E"] > 10 ** 6 else 20
        want = exact()[0]
        print("T=%d B=%d N=%d order=%d Q=%d E=%d threshold=%s" % (T, B, N, order, c["Q"], c["E"], theta), flush=True)
        print("  exact       eager %10.1f us  graph %10.1f us  work %12d bytes" % (timed(exact, reps), replayed(exact, reps),
                                                                                  sizes[-1]), flush=True)
        for K in beams:
            beam = lambda: torch_asg_amd.beam_decode_graph(x, tr, graph, il, K, theta, max_work_bytes=whole)     # noqa: E731
            got = beam()[0]
            same = float((got == want).double().mean())
            print("  beam K=%-5d eager %10.1f us  graph %10.1f us  work %12d bytes  score == exact on %5.1f %% of utterances"
                  % (K, timed(beam, 20), replayed(beam, 20), sizes[-1], 100.0 * same), flush=True)


if __name__ == "__main__":
    main()
