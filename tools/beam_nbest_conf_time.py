#!/usr/bin/env python3
"""Developer probe: per-call time of the token confidences of every row of the n-best list
(torch_asg_amd.beam_decode_graph_nbest_confidence) next to the calls it replaces or is built from, at the same beam in the same
session and in this order: beam_decode_graph (the search it runs once), beam_decode_graph_nbest at nbest 10,
beam_decode_graph_confidence at tolerance 0 and 3, then the new call at nbest 1 / 10 / 100 and tolerance 0 / 3.  The last column is
the new call over the one-best confidence call at the same tolerance; `two calls` is beam_decode_graph_nbest plus
beam_decode_graph_confidence, what a user ran before.  Device events after two warm-up calls: the median and the spread
(min .. max) of CALLS single calls.

    python tools/beam_nbest_conf_time.py [T,B,N,order[,scale] ...]   (default: the shapes DESIGN.md section 5aa reports)
    BEAMS=64,256,1024 CALLS=5                                         (environment)

The workload is tools/beam_conf_time.py's: a random n-gram table of the given order, emissions log-softmax of N(0,1),
transitions `scale` * N(0,1); scale 0.1 gives a hypothesis of about 61 tokens, so that a window is open at most frames.
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
SHAPES = [(400, 64, 40, 3), (400, 64, 40, 4), (400, 64, 40, 3, 0.1)]


def main():
    shapes = [tuple(float(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256,1024").split(",")]
    n = int(os.environ.get("CALLS", "5"))
    whole = 1 << 40                                                       # one group
    for shape in shapes:
        T, B, N, order = (int(v) for v in shape[:4])
        scale = float(shape[4]) if len(shape) > 4 else 1.0
        g = torch.Generator().manual_seed(0)
        tr = (scale * torch.randn(N, N, generator=g)).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        graph = ngram(N, order, order)
        c = graph.compile_beam(DEV, torch.float32, 1.0, 0.0)
        print("T=%d B=%d N=%d order=%d Q=%d E=%d transitions x%g calls=%d" % (T, B, N, order, c["Q"], c["E"], scale, n), flush=True)
        for K in beams:
            def decode():
                return torch_asg_amd.beam_decode_graph(x, tr, graph, il, K, max_work_bytes=whole)

            def nbest10():
                return torch_asg_amd.beam_decode_graph_nbest(x, tr, graph, il, K, 10, max_work_bytes=whole)

            def conf(tol):
                return lambda: torch_asg_amd.beam_decode_graph_confidence(x, tr, graph, il, K, frame_tolerance=tol, max_work_bytes=whole)

            def rows(nb, tol):
                return lambda: torch_asg_amd.beam_decode_graph_nbest_confidence(x, tr, graph, il, K, nb, frame_tolerance=tol,
                                                                               max_work_bytes=whole)
            base, lo, hi = calls(decode, n)
            print("  K=%-5d beam_decode_graph            %9.1f us (%9.1f .. %9.1f)" % (K, base, lo, hi), flush=True)
            nb10, lo, hi = calls(nbest10, n)
            print("  K=%-5d n-best 10                    %9.1f us (%9.1f .. %9.1f)  x%.2f" % (K, nb10, lo, hi, nb10 / base), flush=True)
            one = {}
            for tol in (0, 3):
                one[tol], lo, hi = calls(conf(tol), n)
                print("  K=%-5d confidence tol=%d             %9.1f us (%9.1f .. %9.1f)  x%.2f  two calls %9.1f us" % (
                    K, tol, one[tol], lo, hi, one[tol] / base, one[tol] + nb10), flush=True)
            for nb in (1, 10, 100):
                for tol in (0, 3):
                    med, lo, hi = calls(rows(nb, tol), n)
                    print("  K=%-5d rows nbest=%-3d tol=%d         %9.1f us (%9.1f .. %9.1f)  x%.2f  %+8.1f us over the one-best call, "
                          "x%.3f of the two calls" % (K, nb, tol, med, lo, hi, med / base, med - one[tol], med / (one[tol] + nb10)),
                          flush=True)
            r = rows(10, 0)()
            live = r.token_frames >= 0
            cf = r.token_confidences[live].double()
            print("  K=%-5d finite Z %d/%d, rows %.1f, tokens per row %.1f, mean confidence %.3f, below 0.5: %.1f%%" % (
                K, int(torch.isfinite(r.normalisers).sum()), B, float(r.num_hyps.double().mean()),
                float(live.sum()) / max(1.0, float(r.num_hyps.sum())), float(cf.mean()) if cf.numel() else 0.0,
                100.0 * float((cf < 0.5).double().mean()) if cf.numel() else 0.0), flush=True)


if __name__ == "__main__":
    main()
