#!/usr/bin/env python3
"""Developer probe: per-call time of the token confidences (torch_asg_amd.beam_decode_graph_confidence) next to the calls whose
kernels it is built from, at the same beam in the same session: beam_decode_graph (the search it runs once) and
beam_graph_full_score without targets, forward and forward+backward (the lattice passes; the confidence call replaces that
backward by a beta pass without label posteriors and (i, j) counts).  Device events after two warm-up calls: the median and the
spread (min .. max) of CALLS single calls.

    python tools/beam_conf_time.py [T,B,N,order[,scale] ...]   (default: the shapes DESIGN.md section 5z reports)
    BEAMS=64,256,1024 CALLS=5                                   (environment)

The n-grams are those of tools/beam_loss_time.py (a random table of the given order); emissions are log-softmax of N(0,1);
transitions are `scale` * N(0,1), scale 1 by default (5i's workload, whose best path sits on the largest self-transition: two to
four tokens per utterance).  A small scale gives a hypothesis of many tokens, so that a window is open at most frames.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from beam_loss_time import ngram  # noqa: E402
from beam_word_time import calls  # noqa: E402

DEV = "cuda:0"
SHAPES = [(400, 64, 40, 3), (400, 64, 40, 4)]


def main():
    shapes = [tuple(float(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256,1024").split(",")]
    n = int(os.environ.get("CALLS", "5"))
    whole = 1 << 40                                                       # one group
    for shape in shapes:
        T, B, N, order = (int(v) for v in shape[:4])
        scale = float(shape[4]) if len(shape) > 4 else 1.0
        g = torch.Generator().manual_seed(0)
        tr = (scale * torch.randn(N, N, generator=g)).to(DEV).requires_grad_(True)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV).requires_grad_(True)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        graph = ngram(N, order, order)
        c = graph.compile_beam(DEV, torch.float32, 1.0, 0.0)
        print("T=%d B=%d N=%d order=%d Q=%d E=%d transitions x%g calls=%d" % (T, B, N, order, c["Q"], c["E"], scale, n), flush=True)
        for K in beams:
            def decode():
                return torch_asg_amd.beam_decode_graph(x.detach(), tr.detach(), graph, il, K, max_work_bytes=whole)

            def fwd():
                with torch.no_grad():
                    return torch_asg_amd.beam_graph_full_score(x, tr, graph, il, K, max_work_bytes=whole)

            def step():
                x.grad = tr.grad = None
                torch_asg_amd.beam_graph_full_score(x, tr, graph, il, K, max_work_bytes=whole).sum().backward()

            def conf(tol):
                return lambda: torch_asg_amd.beam_decode_graph_confidence(x.detach(), tr.detach(), graph, il, K, frame_tolerance=tol,
                                                                          max_work_bytes=whole)
            base, lo, hi = calls(decode, n)
            print("  K=%-5d beam_decode_graph        %9.1f us (%9.1f .. %9.1f)" % (K, base, lo, hi), flush=True)
            for name, fn in (("score forward", fwd), ("score forward+backward", step), ("confidence tol=0", conf(0)),
                             ("confidence tol=3", conf(3))):
                med, lo, hi = calls(fn, n)
                print("  K=%-5d %-24s %9.1f us (%9.1f .. %9.1f)  x%.2f" % (K, name, med, lo, hi, med / base), flush=True)
            r = conf(0)()
            nt = r.token_lengths.double()
            cf = r.token_confidences[r.token_frames >= 0].double()
            print("  K=%-5d finite Z %d/%d, tokens per utterance %.1f, mean confidence %.3f, below 0.5: %.1f%%" % (
                K, int(torch.isfinite(r.normalisers).sum()), B, float(nt.mean()), float(cf.mean()) if cf.numel() else 0.0,
                100.0 * float((cf < 0.5).double().mean()) if cf.numel() else 0.0), flush=True)


if __name__ == "__main__":
    main()
