#!/usr/bin/env python3
"""Developer probe: per-call times of streaming beam decoding (torch_asg_amd.BeamStream) next to the one-shot beam decoder
(beam_decode_graph) of the same session, measured with device events after a warm-up: the median and the spread (min .. max)
of CALLS timed samples.  Per shape and beam:
  advance    a chunk of Tc = 8 and of Tc = 40 frames in mid-stream (behind 40 consumed frames), eager and replayed from a hipGraph;
  idle       an advance whose chunk_lengths are all 0: the fixed cost of a call (launch, the transitions into LDS);
  result     result(final=True) at pos = 40 and at pos = 400: the backtrace is one dependent-load chain of pos steps;
  10 chunks  ten advances of Tc = 40 from a fresh state, timed as one block, against ONE beam_decode_graph over the same 400
             frames -- the yardstick is the one-shot call, not the stream's own numbers.
Every sample starts from a state prepared outside the timed region (reset, and the frames before the measured call).

    python tools/beam_stream_time.py [B,N,order ...]        (default: the shapes DESIGN.md section 5l reports)
    BEAMS=64,256 CALLS=9                                    (environment)

order 1..4 is an n-gram from a random table, as tools/graph_decode_time.py makes it; emissions are log-softmax of N(0,1).
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from graph_decode_time import make_graph  # noqa: E402

DEV = "cuda:0"
SHAPES = [(1, 40, 4), (64, 40, 4), (1, 40, 3), (64, 40, 3)]
T = 400


def sample(prepare, fn):
    prepare()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def calls(prepare, fn, n):
    """-> 'median (min .. max)' in us of n samples, after two warm-up samples."""
    sample(prepare, fn)
    sample(prepare, fn)
    ts = [sample(prepare, fn) for _ in range(n)]
    return "%9.1f (%8.1f .. %8.1f) us" % (statistics.median(ts), min(ts), max(ts))


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256").split(",")]
    n = int(os.environ.get("CALLS", "9"))
    graphs = {}
    for B, N, order in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        zero = torch.zeros(B, dtype=torch.int64, device=DEV)
        if (N, order) not in graphs:
            graphs[(N, order)] = make_graph(N, order)
        graph = graphs[(N, order)]
        Q = graph.compile(DEV, torch.float32, 1.0, 0.0)["Q"]
        for K in beams:
            print("B=%d N=%d order=%d Q=%d K=%d T=%d" % (B, N, order, Q, K, T), flush=True)
            s = torch_asg_amd.BeamStream(tr, graph, B, T, K)
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
            one = lambda: torch_asg_amd.beam_decode_graph(x, tr, graph, il, K, max_work_bytes=1 << 40)      # noqa: E731
            print("  one-shot T=400        %s" % calls(nothing, one, n), flush=True)
            a, b = s.result(final=True), one()
            assert torch.equal(a.scores, b[0]) and torch.equal(a.tokens, b[2]), "the stream and the one-shot decode differ"


if __name__ == "__main__":
    main()
