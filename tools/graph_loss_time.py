#!/usr/bin/env python3
"""Developer probe: per-call time of the ASG loss composed with a token automaton (forward + backward of
torch_asg_amd.GraphFullScore, the full-graph part of graph_asg_loss) on each route, measured with device events after a warm-up.

    python tools/graph_loss_time.py [T,B,N,order ...]     (default: the shapes DESIGN.md section 5h reports)

order 0 is the one-state automaton with zero weights (ASGLoss's full lattice); 1..4 an n-gram from a random table.  A route
the graph does not fit (the resident one beyond 128 KiB of vectors) is reported as "-".
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from torch_asg_amd import _lib  # noqa: E402

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
        tr = torch.randn(N, N, generator=g).to(DEV).requires_grad_(True)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV).requires_grad_(True)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        graph = make_graph(N, order)
        c = graph.compile(DEV, torch.float32, 1.0, 0.0)
        big = T * B * c["Q"] * 4 + 256
        fits = 2 * c["Q"] * 4 <= 128 * 1024
        cols = []
        for name, fl in (("resident", _lib.FLAG_GRAPH_LOSS_RESIDENT), ("streaming", _lib.FLAG_GRAPH_LOSS_STREAMING)):
            if name == "resident" and not fits:
                cols.append("%s %10s" % (name, "-"))
                continue

            def fwd():
                with torch.no_grad():
                    torch_asg_amd.GraphFullScore.apply(x.detach(), tr.detach(), graph, il, 1.0, 0.0, big, fl)

            def step():
                torch_asg_amd.GraphFullScore.apply(x, tr, graph, il, 1.0, 0.0, big, fl).sum().backward()
            reps = 2 if c["E"] > 10 ** 6 else 10
            step()
            fwd()
            f_us, s_us = timed(fwd, reps), timed(step, reps)
            cols.append("%s fwd %9.1f us  fwd+bwd %9.1f us" % (name, f_us, s_us))
        print("T=%4d B=%3d N=%3d order=%d Q=%6d E=%8d  %s" % (T, B, N, order, c["Q"], c["E"], "  |  ".join(cols)), flush=True)


if __name__ == "__main__":
    main()
