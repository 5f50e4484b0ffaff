#!/usr/bin/env python3
"""Time the beam-pruned graph loss in ONE session: forward and forward+backward of
`beam_graph_full_score` at T = 400, B = 64, N = 40 for a trigram and a 4-gram at K = 64 / 256 / 1024, beside the exact
`graph_full_score` on the same automata and `beam_decode_graph` at the same K.  Device events after a warm-up; medians and the
min .. max spread over --reps repetitions.  One JSON line per row.

    python tools/beam_loss_time.py [--reps 7] [--orders 3,4] [--beams 64,256,1024] [--no-exact] [--profile]

--profile runs one warm step of the 4-gram at K = 256 and nothing else (for a kernel trace taken in a run of its own)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_asg_amd  # noqa: E402

DEV = "cuda:0"


def ngram(N, order, seed):
    rng = np.random.default_rng(seed)
    return torch_asg_amd.TokenGraph.from_ngram(np.log(rng.dirichlet(np.ones(N + 1), size=(N + 1,) * (order - 1))))


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--orders", default="3,4")
    ap.add_argument("--beams", default="64,256,1024")
    ap.add_argument("--no-exact", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    T, B, N = 400, 64, 40
    g = torch.Generator().manual_seed(0)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV).requires_grad_(True)
    tr = (0.5 * torch.randn(N, N, generator=g)).to(DEV).requires_grad_(True)
    tg = torch.randint(0, N, (B, 60), generator=g).to(DEV)
    tl = torch.full((B,), 60, dtype=torch.int64, device=DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)

    def beam_fwd(graph, K):
        with torch.no_grad():
            torch_asg_amd.beam_graph_full_score(x, tr, graph, il, K, targets=tg, target_lengths=tl)

    def beam_step(graph, K):
        x.grad = tr.grad = None
        torch_asg_amd.beam_graph_full_score(x, tr, graph, il, K, targets=tg, target_lengths=tl).sum().backward()

    def exact_fwd(graph):
        with torch.no_grad():
            torch_asg_amd.graph_full_score(x, tr, graph, il, max_work_bytes=8 << 30)

    def exact_step(graph):
        x.grad = tr.grad = None
        torch_asg_amd.graph_full_score(x, tr, graph, il, max_work_bytes=8 << 30).sum().backward()

    if a.profile:
        graph = ngram(N, 4, 4)
        beam_step(graph, 256)
        beam_step(graph, 256)
        torch.cuda.synchronize()
        return
    for order in [int(o) for o in a.orders.split(",")]:
        graph = ngram(N, order, order)
        Q = graph.compile(DEV, torch.float32)["Q"]
        if not a.no_exact:
            for name, fn in (("exact forward", exact_fwd), ("exact forward+backward", exact_step)):
                print(json.dumps({"order": order, "Q": Q, "what": name, **timed(lambda: fn(graph), a.reps)}), flush=True)
        for K in [int(k) for k in a.beams.split(",")]:
            rows = (("beam forward", lambda: beam_fwd(graph, K)), ("beam forward+backward", lambda: beam_step(graph, K)),
                    ("beam_decode_graph", lambda: torch_asg_amd.beam_decode_graph(x.detach(), tr.detach(), graph, il, K)))
            for name, fn in rows:
                print(json.dumps({"order": order, "Q": Q, "K": K, "what": name, **timed(fn, a.reps)}), flush=True)


if __name__ == "__main__":
    main()
