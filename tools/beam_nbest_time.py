#!/usr/bin/env python3
"""Developer probe: per-call time of the n-best beam decoder (torch_asg_amd.beam_decode_graph_nbest) next to the one-best beam
decoder (beam_decode_graph) at the same beam in the same session, measured with device events after a warm-up: the median and
the spread (min .. max) of CALLS timed calls, and beside each row the time above beam_decode_graph -- the cost of the n-best
stage (the sort of the last set, one walk per hypothesis, the token collapse).

    python tools/beam_nbest_time.py [T,B,N,order ...]      (default: the shapes DESIGN.md section 5k reports)
    BEAMS=256,1024 NBEST=1,10,100,K CALLS=9 ALIGN=0         (environment; K in NBEST stands for the beam size)

order 1..4 is an n-gram from a random table, as tools/graph_decode_time.py makes it; emissions are log-softmax of N(0,1).
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from graph_decode_time import make_graph, timed  # noqa: E402

DEV = "cuda:0"
SHAPES = [(400, 64, 40, 4), (400, 64, 40, 3)]


def calls(fn, n):
    """-> (median, min, max) in us of n single calls, after two warm-up calls."""
    fn()
    fn()
    ts = [timed(fn, 1) for _ in range(n)]
    return statistics.median(ts), min(ts), max(ts)


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "256,1024").split(",")]
    nbests = os.environ.get("NBEST", "1,10,100,K").split(",")
    n = int(os.environ.get("CALLS", "9"))
    align = os.environ.get("ALIGN", "0") == "1"
    whole = 1 << 40                                                       # one group
    for T, B, N, order in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        graph = make_graph(N, order)
        c = graph.compile(DEV, torch.float32, 1.0, 0.0)
        print("T=%d B=%d N=%d order=%d Q=%d E=%d alignments=%d calls=%d" % (T, B, N, order, c["Q"], c["E"], align, n), flush=True)
        for K in beams:
            one = lambda: torch_asg_amd.beam_decode_graph(x, tr, graph, il, K, max_work_bytes=whole)       # noqa: E731
            base, lo, hi = calls(one, n)
            print("  K=%-5d beam_decode_graph     %9.1f us (%9.1f .. %9.1f)" % (K, base, lo, hi), flush=True)
            for nb in nbests:
                nb = K if nb == "K" else int(nb)
                many = lambda: torch_asg_amd.beam_decode_graph_nbest(x, tr, graph, il, K, nb, return_alignments=align,   # noqa: E731
                                                                     max_work_bytes=whole)
                out = many()
                med, lo, hi = calls(many, n)
                print("  K=%-5d nbest=%-5d            %9.1f us (%9.1f .. %9.1f)  above the one-best decoder %+9.1f us  "
                      "hypotheses per utterance %.1f" % (K, nb, med, lo, hi, med - base, float(out.num_hyps.double().mean())),
                      flush=True)


if __name__ == "__main__":
    main()
