#!/usr/bin/env python3
"""Developer probe: per-call time of Viterbi decoding with a token automaton (torch_asg_amd.viterbi_decode_graph) next to
the plain decoder, eager and replayed from a hipGraph, measured with device events after a warm-up.

    python tools/graph_decode_time.py [T,B,N,order ...]     (default: the shapes DESIGN.md section 5g reports)

order 0 is the one-state automaton with zero weights (the plain decoder's search); 1..4 an n-gram from a random table.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402

DEV = "cuda:0"
SHAPES = [(400, 64, 40, 0), (400, 64, 40, 2), (400, 64, 40, 3), (400, 64, 40, 4)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per call


def make_graph(N, order, seed=0):
    if order == 0:
        return torch_asg_amd.TokenGraph(np.zeros((1, N), np.int64), np.zeros((1, N)), np.zeros(1))
    rng = np.random.default_rng(seed)
    size = (N + 1,) * (order - 1) if order > 1 else None
    return torch_asg_amd.TokenGraph.from_ngram(np.log(rng.dirichlet(np.ones(N + 1), size=size)))


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or SHAPES
    for T, B, N, order in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        graph = make_graph(N, order)
        c = graph.compile(DEV, torch.float32, 1.0, 0.0)
        work = T * B * c["Q"] * 4 + 2 * c["Q"] * B * 4 + 256
        call = lambda: torch_asg_amd.viterbi_decode_graph(x, tr, graph, il, max_work_bytes=work)      # noqa: E731
        reps = 2 if c["E"] > 10 ** 6 else 20
        call()
        eager = timed(call, reps)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            call()
        gr.replay()
        graph_us = timed(gr.replay, reps)
        del gr
        line = "T=%4d B=%3d N=%3d order=%d Q=%6d E=%8d  eager %10.1f us  graph %10.1f us  (%.2f us/frame)" % (
            T, B, N, order, c["Q"], c["E"], eager, graph_us, graph_us / T)
        from torch_asg_amd.asg import native
        for flag, name in ((16, "streaming"), (32, "resident")):
            one = lambda: native().viterbi_decode_graph(x, tr, graph, il, 1.0, 0.0, work, flag)      # noqa: E731
            one()
            line += "  %s %.1f us" % (name, timed(one, reps))
        if order == 0:
            plain = timed(lambda: torch_asg_amd.viterbi_decode(x, tr, il), reps)
            line += "  viterbi_decode eager %.1f us" % plain
        print(line, flush=True)


if __name__ == "__main__":
    main()
