#!/usr/bin/env python3
"""Timing of `target_graph_viterbi` with 5ai's protocol: float32, T = 400, B = 64, N = 40, device events around
200 calls after 20 warm ones, three passes with the cases alternating.

    python tools/target_graph_viterbi_time.py [OUT.txt]

(a) chains of 30 nodes: against `viterbi_align` and against `target_graph_score` without a gradient, on the same inputs;
(b) prefix trees of four alternatives of about 30 labels: against four `viterbi_align` calls plus the argmax."""
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
    x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
    tr = (0.5 * torch.randn(N, N, generator=g)).to(DEV)
    il = torch.full((B,), T, dtype=torch.int64, device=DEV)
    walk = lambda n: np.cumsum(rng.integers(1, N, n)) % N                   # neighbouring labels distinct
    tg = torch.from_numpy(np.stack([walk(S) for _ in range(B)])).to(DEV)
    tl = torch.full((B,), S, dtype=torch.int64, device=DEV)
    chains = A.TargetGraphs.from_targets(tg, tl, N)
    alts = []                                                               # a sequence, and three that leave it somewhere
    for b in range(B):
        base = walk(S)
        seqs = [base]
        for cut in rng.integers(1, S, 3):
            seqs.append(np.r_[base[:cut], (base[cut - 1] + walk(S - cut)) % N])
        alts.append(seqs)
    trees = A.TargetGraphs.from_alternatives(alts, N)
    at = [torch.from_numpy(np.stack([alts[b][j] for b in range(B)])).to(DEV) for j in range(4)]

    def four():
        return torch.stack([A.viterbi_align(x, at[j], tr, il, tl)[0] for j in range(4)]).argmax(0)

    def score():
        with torch.no_grad():
            return A.target_graph_score(x, tr, chains, il)
    cases = [("(a) chains, target_graph_viterbi", lambda: A.target_graph_viterbi(x, tr, chains, il)),
             ("(a) chains, viterbi_align", lambda: A.viterbi_align(x, tg, tr, il, tl)),
             ("(a) chains, target_graph_score forward", score),
             ("(b) prefix trees of 4, target_graph_viterbi", lambda: A.target_graph_viterbi(x, tr, trees, il)),
             ("(b) prefix trees of 4, four viterbi_align + argmax", four)]
    r, va = A.target_graph_viterbi(x, tr, chains, il), A.viterbi_align(x, tg, tr, il, tl)
    rt = A.target_graph_viterbi(x, tr, trees, il)
    lines = ["T=%d B=%d N=%d float32; chains of %d nodes; trees: Kmax=%d Emax=%d, mean nodes %.1f"
             % (T, B, N, S, trees.Kmax, trees.Emax, np.mean([len(gr[0]) for gr in trees.graphs])),
             "chains: scores equal viterbi_align's: %s, nodes equal its positions: %s; trees: alternatives equal the argmax of four: %s"
             % (torch.equal(r.scores, va[0]), torch.equal(r.nodes, va[1]), torch.equal(rt.alternatives, four()))]
    for p in range(3):
        for name, fn in cases:
            lines.append("pass %d  %-58s %7.1f us" % (p, name, timed(fn)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
