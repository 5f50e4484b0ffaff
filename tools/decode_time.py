#!/usr/bin/env python3
"""Developer probe: per-call time of Viterbi decoding over the full lattice (torch_asg_amd.viterbi_decode), eager and
replayed from a hipGraph, measured with device events after a warm-up.

    python tools/decode_time.py [T,B,N ...]        (default: the shapes DESIGN.md section 5f reports)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402

DEV = "cuda:0"
SHAPES = [(400, 64, 40), (400, 64, 1000), (400, 64, 3000), (2000, 32, 10000)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per call


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or SHAPES
    for T, B, N in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        call = lambda: torch_asg_amd.viterbi_decode(x, tr, il)      # noqa: E731
        big = T * B * N > 10 ** 8
        reps = 2 if big else 20
        call()
        eager = timed(call, reps)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            call()
        gr.replay()
        graph = timed(gr.replay, reps)
        print("T=%5d B=%3d N=%6d  eager %10.1f us  graph %10.1f us  (%.2f us/frame)" % (T, B, N, eager, graph, graph / T),
              flush=True)
        del gr


if __name__ == "__main__":
    main()
