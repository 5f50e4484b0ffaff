#!/usr/bin/env python3
"""Timing and float32 accuracy of `target_graph_final_scores` with 5ai's protocol: float32, T = 400, B = 64,
N = 40, device events around 200 calls after 20 warm ones, three passes with the cases alternating.

    python tools/target_graph_final_time.py [OUT.txt]

(a) chains of 30 nodes and (b) prefix trees of four alternatives of about 30 labels; for both, the forward alone and forward +
backward with a signed gradient per final node, beside `target_graph_score` forward + backward on the same inputs and, for
the trees, the only route there was before: one `FAC` forward + backward per alternative on the same emissions, autograd
adding the four gradients.  Then the error of the float32 call against the float64 call on the same inputs, next to the same
figure for `target_graph_score`."""
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
    ga = torch.randn(B, 4, generator=g).to(DEV)                             # a signed weight per alternative
    tgt = [torch.from_numpy(np.stack([alts[b][a] for b in range(B)])).to(DEV) for a in range(4)]
    tl = torch.full((B,), S, dtype=torch.int64, device=DEV)

    def grads(xx, tt, graphs, fn, gr):
        xx.grad = tt.grad = None
        out = fn(xx, tt, graphs, il)
        out.backward(gr)
        return out.detach(), xx.grad, tt.grad

    def final_grad(graphs, dtype=torch.float32):                            # [B,Kmax]: ga on the alternatives' finals
        af = graphs.alternative_final_on(DEV)
        return torch.zeros(B, graphs.Kmax, device=DEV, dtype=dtype).scatter_(1, af, ga[:, :af.shape[1]].to(dtype))

    def four_fac():
        x.grad = tr.grad = None
        sc = torch.stack([A.FAC.apply(tr, x, tgt[a], il, tl) for a in range(4)], 1)
        sc.backward(ga)
        return sc.detach(), x.grad, tr.grad

    def plain(graphs):
        def run():
            with torch.no_grad():
                return A.target_graph_final_scores(x, tr, graphs, il)
        return run
    cases = []
    for tag, graphs in (("(a) chains", chains), ("(b) prefix trees of 4", trees)):
        gf = final_grad(graphs)
        cases += [(tag + ", target_graph_final_scores fwd, no gradient", plain(graphs)),
                  (tag + ", target_graph_final_scores fwd + bwd", lambda graphs=graphs, gf=gf: grads(x, tr, graphs, A.target_graph_final_scores, gf)),
                  (tag + ", target_graph_score fwd + bwd", lambda graphs=graphs: grads(x, tr, graphs, A.target_graph_score, gs))]
    cases.append(("(b) four FAC fwd + bwd, gradients added by autograd", four_fac))
    lines = ["T=%d B=%d N=%d float32; chains of %d nodes; trees: Kmax=%d Emax=%d, mean nodes %.1f"
             % (T, B, N, S, trees.Kmax, trees.Emax, np.mean([len(gr[0]) for gr in trees.graphs]))]
    one, two = [[v.clone() for v in grads(x, tr, trees, A.target_graph_final_scores, final_grad(trees))] for _ in range(2)]
    fac = [v.clone() for v in four_fac()]
    alt = one[0].gather(1, trees.alternative_final_on(DEV))
    rel = lambda u, v: float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max())))
    lines.append("trees: equal bits over two steps: %s; against four FAC calls, scaled max error: scores %.2e grad_inputs %.2e "
                 "grad_transition %.2e" % (all(torch.equal(u, v) for u, v in zip(one, two)), rel(alt, fac[0]), rel(one[1], fac[1]),
                                           rel(one[2], fac[2])))
    xd, td = x.detach().double().requires_grad_(True), tr.detach().double().requires_grad_(True)
    for tag, graphs in (("chains", chains), ("trees", trees)):             # float32 against float64 on the same inputs
        for name, fn, g32, g64 in (("target_graph_final_scores", A.target_graph_final_scores, final_grad(graphs), final_grad(graphs, torch.float64)),
                                   ("target_graph_score", A.target_graph_score, gs, gs.double())):
            lo = [v.clone() for v in grads(x, tr, graphs, fn, g32)]
            hi = grads(xd, td, graphs, fn, g64)
            fin = torch.isfinite(hi[0])
            lines.append("float32 against float64, %s, %s: scaled max error (max |x - ref| / max(1, max |ref|)): scores %.2e "
                         "grad_inputs %.2e grad_transition %.2e; the -inf patterns agree: %s"
                         % (tag, name, rel(lo[0][fin], hi[0][fin]), rel(lo[1], hi[1]), rel(lo[2], hi[2]),
                            torch.equal(fin, torch.isfinite(lo[0]))))
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
