#!/usr/bin/env python3
"""Developer probe: what keeping the lattice costs a beam stream, and what a confidence from it costs
(BeamStream(..., keep_lattice=True).result_confidence), next to the two yardsticks of the same session that are older code: the
plain stream's `advance` and the one-shot `beam_decode_graph_confidence`.  Device events after two warm-ups: the median and the
spread (min .. max) of CALLS timed samples.  Per beam and tolerance, in this order:
  advance plain      a plain BeamStream's advance of 40 frames from a fresh state: the yardstick for the cost of keeping the lattice;
  advance lattice    the lattice-keeping stream's advance of the same 40 frames;
  conf pos=40/400    result_confidence(tol) with every frame to catch up (the state prepared outside the timed region) and caught
                     up (a second call), prefix mode;
  10 + conf          ten advances of 40 frames from a fresh state plus one result_confidence(tol, final=True), timed as one block,
                     against ONE beam_decode_graph_confidence over the same 400 frames: the yardstick.
The last two are also compared bit for bit.

    python tools/beam_stream_conf_time.py [T,B,N,order ...]   (default: the trigram workload of DESIGN.md sections 5z and 5ad)
    BEAMS=64,256 TOLS=0,3 CALLS=5                              (environment)

The n-gram is tools/beam_loss_time.py's (a random table of the given order); emissions are log-softmax of N(0,1), transitions
N(0,1): tools/beam_conf_time.py's workload.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch_asg_amd  # noqa: E402
from beam_loss_time import ngram  # noqa: E402
from beam_stream_time import calls  # noqa: E402

DEV = "cuda:0"
SHAPES = [(400, 64, 40, 3)]
TC = 40


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256").split(",")]
    tols = [int(v) for v in os.environ.get("TOLS", "0,3").split(",")]
    n = int(os.environ.get("CALLS", "5"))
    nothing = lambda: None                                                            # noqa: E731
    for T, B, N, order in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        il = torch.full((B,), T, dtype=torch.int64, device=DEV)
        graph = ngram(N, order, order)
        c = graph.compile_beam(DEV, torch.float32, 1.0, 0.0)
        print("T=%d B=%d N=%d order=%d Q=%d E=%d chunk=%d calls=%d" % (T, B, N, order, c["Q"], c["E"], TC, n), flush=True)
        for K in beams:
            plain = torch_asg_amd.BeamStream(tr, graph, B, T, K)
            s = torch_asg_amd.BeamStream(tr, graph, B, T, K, keep_lattice=True)
            print("  K=%-4d state bytes: plain %d, lattice %d" % (K, plain._state.numel(), s._state.numel()), flush=True)
            print("  K=%-4d advance plain    40 frames       %s" % (K, calls(plain.reset, lambda: plain.advance(x[:TC]), n)), flush=True)
            print("  K=%-4d advance lattice  40 frames       %s" % (K, calls(s.reset, lambda: s.advance(x[:TC]), n)), flush=True)

            def feed(frames):
                def go():
                    s.reset()
                    for t0 in range(0, frames, TC):
                        s.advance(x[t0:t0 + TC])
                return go
            for tol in tols:
                for frames in (TC, T):
                    fn = lambda: s.result_confidence(tol)                             # noqa: E731
                    print("  K=%-4d tol=%d conf pos=%-3d catch-up all  %s" % (K, tol, frames, calls(feed(frames), fn, n)), flush=True)
                    print("  K=%-4d tol=%d conf pos=%-3d caught up     %s" % (K, tol, frames, calls(nothing, fn, n)), flush=True)

                def ten():
                    for t0 in range(0, T, TC):
                        s.advance(x[t0:t0 + TC])
                    return s.result_confidence(tol, final=True)
                one = lambda: torch_asg_amd.beam_decode_graph_confidence(x, tr, graph, il, K, frame_tolerance=tol,     # noqa: E731
                                                                         max_work_bytes=1 << 40)
                print("  K=%-4d tol=%d 10 chunks of 40 + conf      %s" % (K, tol, calls(s.reset, ten, n)), flush=True)
                print("  K=%-4d tol=%d one-shot confidence T=400   %s" % (K, tol, calls(nothing, one, n)), flush=True)
                s.reset()
                a, b = ten(), one()
                for f in ("scores", "tokens", "token_lengths", "token_frames", "token_confidences", "normalisers"):
                    assert torch.equal(getattr(a, f), getattr(b, f)), f
                nt = a.token_lengths.double()
                cf = a.token_confidences[a.token_frames >= 0].double()
                print("  K=%-4d tol=%d bit-equal to the one-shot call; finite Z %d/%d, tokens per utterance %.1f, mean confidence "
                      "%.3f" % (K, tol, int(torch.isfinite(a.normalisers).sum()), B, float(nt.mean()),
                                float(cf.mean()) if cf.numel() else 0.0), flush=True)


if __name__ == "__main__":
    main()
