#!/usr/bin/env python3
"""Timing of `target_graph_confidence` with 5ai's protocol: float32, T = 400, B = 64, N = 40, device events
around 200 calls after 20 warm ones, three passes with the cases alternating.

    python tools/target_graph_conf_time.py [OUT.txt]

(a) chains of 30 nodes, (b) prefix trees of four alternatives of about 30 labels.  Each at frame_tolerance 0 and 2, beside
`target_graph_viterbi` and `target_graph_score` forward + backward on the same inputs; the last lines give the call as a
ratio of the sum of those two (the median of the passes)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch_asg_amd as A  # noqa: E402
from target_graph_viterbi_time import B, DEV, N, S, T, timed  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    g = torch.Generator().manual_seed(0)
    x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
    tr = (0.5 * torch.randn(N, N, generator=g)).to(DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)
    walk = lambda n: np.cumsum(rng.integers(1, N, n)) % N                   # neighbouring labels distinct
    chains = A.TargetGraphs.from_alternatives([[walk(S)] for _ in range(B)], N)
    alts = []                                                               # a sequence, and three that leave it somewhere
    for b in range(B):
        base = walk(S)
        alts.append([base] + [np.r_[base[:cut], (base[cut - 1] + walk(S - cut)) % N] for cut in rng.integers(1, S, 3)])
    trees = A.TargetGraphs.from_alternatives(alts, N)
    xg, trg, ones = x.clone().requires_grad_(True), tr.clone().requires_grad_(True), torch.ones(B, device=DEV)

    def train(graphs):
        xg.grad = trg.grad = None
        A.target_graph_score(xg, trg, graphs, il).backward(ones)
    cases = []
    for tag, graphs in (("(a) chains", chains), ("(b) trees of 4", trees)):
        cases += [(tag, "confidence tol 0", lambda graphs=graphs: A.target_graph_confidence(x, tr, graphs, il, 0)),
                  (tag, "confidence tol 2", lambda graphs=graphs: A.target_graph_confidence(x, tr, graphs, il, 2)),
                  (tag, "viterbi", lambda graphs=graphs: A.target_graph_viterbi(x, tr, graphs, il)),
                  (tag, "score forward + backward", lambda graphs=graphs: train(graphs))]
    r = A.target_graph_confidence(x, tr, trees, il, 0)
    lines = ["T=%d B=%d N=%d float32; chains of %d nodes; trees: Kmax=%d Emax=%d, mean nodes %.1f"
             % (T, B, N, S, trees.Kmax, trees.Emax, np.mean([len(gr[0]) for gr in trees.graphs])),
             "trees: alternative posteriors sum to 1 within %.1e; lowest token confidence %.3f, mean %.3f"
             % ((r.alternative_posteriors.sum(1) - 1).abs().max().item(), r.token_confidences[r.tokens >= 0].min().item(),
                r.token_confidences[r.tokens >= 0].mean().item())]
    us = {}
    for p in range(3):
        for tag, name, fn in cases:
            us.setdefault((tag, name), []).append(timed(fn))
            lines.append("pass %d  %-16s %-26s %7.1f us" % (p, tag, name, us[tag, name][-1]))
    for tag in ("(a) chains", "(b) trees of 4"):
        med = {name: float(np.median(v)) for (t, name), v in us.items() if t == tag}
        both = med["viterbi"] + med["score forward + backward"]
        lines.append("%-16s confidence / (viterbi + score forward + backward): tol 0 %.2f, tol 2 %.2f"
                     % (tag, med["confidence tol 0"] / both, med["confidence tol 2"] / both))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
