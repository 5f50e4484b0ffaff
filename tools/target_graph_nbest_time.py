#!/usr/bin/env python3
"""Timing of `target_graph_nbest` with 5aj's protocol: float32, T = 400, B = 64, N = 40, device events around
200 calls after 20 warm ones, three passes with the cases alternating.

    python tools/target_graph_nbest_time.py [OUT.txt]

(a) chains of 30 nodes, (b) prefix trees of four alternatives of about 30 labels.  Each at nbest 1, 4 and Kmax, beside
`target_graph_viterbi` on the same inputs; for (b) also four `viterbi_align` calls plus a sort, the only route to the ranking
before.  The last lines give the medians of the passes.  With ASG_HIP_LIB set the run measures that library (a build whose
best-path unit is an earlier text, to see whether sharing the forward moved it)."""
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
    tl = torch.full((B,), S, dtype=torch.int64, device=DEV)
    walk = lambda n: np.cumsum(rng.integers(1, N, n)) % N                   # neighbouring labels distinct
    chains = A.TargetGraphs.from_alternatives([[walk(S)] for _ in range(B)], N)
    alts = []                                                               # a sequence, and three that leave it somewhere
    for b in range(B):
        base = walk(S)
        alts.append([base] + [np.r_[base[:cut], (base[cut - 1] + walk(S - cut)) % N] for cut in rng.integers(1, S, 3)])
    trees = A.TargetGraphs.from_alternatives(alts, N)
    at = [torch.from_numpy(np.stack([alts[b][j] for b in range(B)])).to(DEV) for j in range(4)]

    def four():
        return torch.stack([A.viterbi_align(x, at[j], tr, il, tl)[0] for j in range(4)], 1).sort(1, descending=True)
    cases = []
    for tag, graphs in (("(a) chains", chains), ("(b) trees of 4", trees)):
        cases += [(tag, "nbest %d" % nb, lambda graphs=graphs, nb=nb: A.target_graph_nbest(x, tr, graphs, il, nb))
                  for nb in (1, 4, graphs.Kmax)]
        cases.append((tag, "viterbi", lambda graphs=graphs: A.target_graph_viterbi(x, tr, graphs, il)))
    cases.append(("(b) trees of 4", "four viterbi_align + sort", four))
    r, one, top = A.target_graph_nbest(x, tr, trees, il, 4), A.target_graph_viterbi(x, tr, trees, il), four()
    lines = ["T=%d B=%d N=%d float32; chains of %d nodes; trees: Kmax=%d Emax=%d, mean nodes %.1f; library: %s"
             % (T, B, N, S, trees.Kmax, trees.Emax, np.mean([len(gr[0]) for gr in trees.graphs]),
                os.path.basename(os.environ.get("ASG_HIP_LIB", "") or "the package's")),
             "trees, nbest 4: row 0 equals target_graph_viterbi: %s; scores equal the sorted four: %s, alternatives its order: %s"
             % (torch.equal(r.scores[:, 0], one.scores) and torch.equal(r.tokens[:, 0], one.tokens),
                torch.equal(r.scores, top.values), torch.equal(r.alternatives, top.indices))]
    us = {}
    for p in range(3):
        for tag, name, fn in cases:
            us.setdefault((tag, name), []).append(timed(fn))
            lines.append("pass %d  %-16s %-26s %7.1f us" % (p, tag, name, us[tag, name][-1]))
    for (tag, name), v in us.items():
        lines.append("median  %-16s %-26s %7.1f us  (spread %.1f)" % (tag, name, float(np.median(v)), max(v) - min(v)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
