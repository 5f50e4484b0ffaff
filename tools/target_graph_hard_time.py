#!/usr/bin/env python3
"""Timing of `target_graph_viterbi_score` forward + backward with 5ai's protocol: float32, T = 400, B = 64,
N = 40, device events around 200 calls after 20 warm ones, three passes with the cases alternating.

    python tools/target_graph_hard_time.py [OUT.txt]

(a) chains of 30 nodes and (b) prefix trees of four alternatives of about 30 labels; for both, the hard step against the soft
step (`target_graph_score` forward + backward) and against `target_graph_viterbi`, and the hard forward without a gradient,
on the same inputs."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch_asg_amd as A  # noqa: E402

T, B, N, S, DEV = 400, 64, 40, 30, "cuda:0"


def timed(fn, calls=200, warm=20):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls


def main():
    rng = np.random.default_rng(0)
    g = torch.Generator().manual_seed(0)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV).requires_grad_(True)
    tr = (0.5 * torch.randn(N, N, generator=g)).to(DEV).requires_grad_(True)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)
    gs = torch.linspace(-1.0, 2.0, B, device=DEV)
    walk = lambda n: np.cumsum(rng.integers(1, N, n)) % N                   # neighbouring labels distinct
    chains = A.TargetGraphs.from_targets(torch.from_numpy(np.stack([walk(S) for _ in range(B)])).to(DEV),
                                         torch.full((B,), S, dtype=torch.int64, device=DEV), N)
    alts = []                                                               # a sequence, and three that leave it somewhere
    for b in range(B):
        base = walk(S)
        alts.append([base] + [np.r_[base[:cut], (base[cut - 1] + walk(S - cut)) % N] for cut in rng.integers(1, S, 3)])
    trees = A.TargetGraphs.from_alternatives(alts, N)

    def step(score, graphs):
        def fn():
            x.grad = tr.grad = None
            Z = score(x, tr, graphs, il)
            Z.backward(gs)
            return Z.detach(), x.grad, tr.grad
        return fn

    def plain(fn, graphs):
        def run():
            with torch.no_grad():
                return fn(x, tr, graphs, il)
        return run
    cases = []
    for tag, graphs in (("(a) chains", chains), ("(b) prefix trees of 4", trees)):
        cases += [(tag + ", target_graph_viterbi_score fwd + bwd", step(A.target_graph_viterbi_score, graphs)),
                  (tag + ", target_graph_score fwd + bwd", step(A.target_graph_score, graphs)),
                  (tag + ", target_graph_viterbi", plain(A.target_graph_viterbi, graphs)),
                  (tag + ", target_graph_viterbi_score fwd, no gradient", plain(A.target_graph_viterbi_score, graphs))]
    lines = ["T=%d B=%d N=%d float32; chains of %d nodes; trees: Kmax=%d Emax=%d, mean nodes %.1f"
             % (T, B, N, S, trees.Kmax, trees.Emax, np.mean([len(gr[0]) for gr in trees.graphs]))]
    for tag, graphs in (("chains", chains), ("trees", trees)):
        one, two = [[v.clone() for v in step(A.target_graph_viterbi_score, graphs)()] for _ in range(2)]
        r = plain(A.target_graph_viterbi, graphs)()
        hot = torch.zeros(T, B, N, device=DEV).scatter_(2, r.labels.t().unsqueeze(2), gs.expand(T, B).unsqueeze(2))
        lines.append("%s: scores equal target_graph_viterbi's: %s; grad_inputs is the one-hot of its labels: %s; equal bits over two "
                     "steps: %s" % (tag, torch.equal(one[0], r.scores), torch.equal(one[1], hot),
                                    all(torch.equal(u, v) for u, v in zip(one, two))))
    for p in range(3):
        for name, fn in cases:
            lines.append("pass %d  %-68s %7.1f us" % (p, name, timed(fn)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
