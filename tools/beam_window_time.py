#!/usr/bin/env python3
"""Developer probe: per-call times of windowed streaming beam decoding (torch_asg_amd.BeamWindowStream, W = 128, P = 32) next to
the unbounded stream (BeamStream, max_frames = 400) of the same session, measured with device events after a warm-up: the median
and the spread (min .. max) of CALLS timed samples.  Per shape and beam, for both streams:
  10 chunks  ten advances of Tc = 40 from a fresh state, timed as one block -- the unbounded stream is the yardstick;
  result     result(final=True) at pos = 400: the window's backtrace is at most W steps, the unbounded one's is pos steps;
  idle       an advance whose chunk_lengths are all 0: the fixed cost of a call;
and the bytes of back-pointers per slot of both (2 * W * K * 4 against 2 * max_frames * K * 4).
Every sample starts from a state prepared outside the timed region.

    python tools/beam_window_time.py [B,N,order ...]        (default: the shapes DESIGN.md section 5m names)
    BEAMS=64,256 CALLS=9 WINDOW=128 EVERY=32                (environment)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from beam_stream_time import DEV, SHAPES, T, calls  # noqa: E402
from graph_decode_time import make_graph  # noqa: E402


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256").split(",")]
    n = int(os.environ.get("CALLS", "9"))
    W, P = int(os.environ.get("WINDOW", "128")), int(os.environ.get("EVERY", "32"))
    graphs = {}
    for B, N, order in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        zero = torch.zeros(B, dtype=torch.int64, device=DEV)
        if (N, order) not in graphs:
            graphs[(N, order)] = make_graph(N, order)
        graph = graphs[(N, order)]
        Q = graph.compile(DEV, torch.float32, 1.0, 0.0)["Q"]
        for K in beams:
            k = min(K, max(Q, 1))
            print("B=%d N=%d order=%d Q=%d K=%d T=%d W=%d P=%d   back-pointers per slot: window %d bytes, unbounded %d bytes"
                  % (B, N, order, Q, K, T, W, P, 2 * W * k * 4, 2 * T * k * 4), flush=True)
            streams = {"window   ": torch_asg_amd.BeamWindowStream(tr, graph, B, W, P, K),
                       "unbounded": torch_asg_amd.BeamStream(tr, graph, B, T, K)}
            nothing = lambda: None                                                    # noqa: E731
            for name, s in streams.items():
                def ten(s=s):
                    for t0 in range(0, T, 40):
                        s.advance(x[t0:t0 + 40])

                def full(s=s, ten=ten):
                    s.reset()
                    ten()
                print("  %s 10 chunks of 40       %s" % (name, calls(s.reset, ten, n)), flush=True)
                full()
                print("  %s result pos=400        %s" % (name, calls(nothing, lambda s=s: s.result(final=True), n)), flush=True)

                def half(s=s):
                    s.reset()
                    s.advance(x[:40])
                print("  %s idle (lengths 0)      %s" % (name, calls(half, lambda s=s: s.advance(x[40:80], zero), n)), flush=True)
            for s in streams.values():
                s.reset()
                for t0 in range(0, T, 40):
                    s.advance(x[t0:t0 + 40])
            a, b = streams["window   "].result(final=True), streams["unbounded"].result(final=True)
            assert torch.equal(a.scores, b.scores), "the window stream and the unbounded stream differ in their scores"
            print("  committed at pos=400: %s   status: %s" % (a.committed.tolist()[:4], a.status.tolist()[:4]), flush=True)


if __name__ == "__main__":
    main()
