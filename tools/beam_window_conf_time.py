#!/usr/bin/env python3
"""Developer probe: what the lattice ring costs a window stream (BeamWindowStream(..., keep_lattice=True).advance: the search
with its keep hooks, the catch-up and the pull of every committing attempt), next to the two yardsticks of the same session that
are older code: the plain window stream's `advance`, and the growing lattice stream's `advance` plus one `result_confidence`.
Device events after two warm-ups: the median and the spread (min .. max) of CALLS timed samples.  Per beam and tolerance:
  10 chunks plain window      ten advances of 40 frames from a fresh plain BeamWindowStream(window=128, commit_every=32);
  10 chunks lattice window    the same ten advances of the lattice-keeping stream (max_chunk = 40), confidences included;
  10 chunks growing + conf    ten advances of BeamStream(keep_lattice=True) plus one result_confidence(tol): one alpha and ONE
                              beta pass over the 400 frames;
and what the run committed: tokens and committing attempts per utterance, the mean confidence, the slots with a forced commit.

    python tools/beam_window_conf_time.py [T,B,N,order ...]   (default: the trigram workload of DESIGN.md sections 5z and 5ag)
    BEAMS=64,256 TOLS=0,3 CALLS=5                              (environment)
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
TC, W, P = 40, 128, 32


def main():
    shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if "," in a] or SHAPES
    beams = [int(v) for v in os.environ.get("BEAMS", "64,256").split(",")]
    tols = [int(v) for v in os.environ.get("TOLS", "0,3").split(",")]
    n = int(os.environ.get("CALLS", "5"))
    for T, B, N, order in shapes:
        g = torch.Generator().manual_seed(0)
        tr = torch.randn(N, N, generator=g).to(DEV)
        x = torch.log_softmax(torch.randn(T, B, N, generator=g), -1).to(DEV)
        graph = ngram(N, order, order)
        c = graph.compile_beam(DEV, torch.float32, 1.0, 0.0)
        print("T=%d B=%d N=%d order=%d Q=%d E=%d chunk=%d window=%d commit_every=%d calls=%d"
              % (T, B, N, order, c["Q"], c["E"], TC, W, P, n), flush=True)
        for K in beams:
            plain = torch_asg_amd.BeamWindowStream(tr, graph, B, W, P, K)

            def ten(s):
                def go():
                    return [s.advance(x[t0:t0 + TC]) for t0 in range(0, T, TC)]
                return go
            print("  K=%-4d 10 chunks plain window            %s" % (K, calls(plain.reset, ten(plain), n)), flush=True)
            for tol in tols:
                s = torch_asg_amd.BeamWindowStream(tr, graph, B, W, P, K, keep_lattice=True, frame_tolerance=tol, max_chunk=TC)
                grow = torch_asg_amd.BeamStream(tr, graph, B, T, K, keep_lattice=True)
                print("  K=%-4d tol=%d state bytes: plain %d, lattice window %d, growing lattice %d"
                      % (K, tol, plain._state.numel(), s._state.numel(), grow._state.numel()), flush=True)
                print("  K=%-4d tol=%d 10 chunks lattice window    %s" % (K, tol, calls(s.reset, ten(s), n)), flush=True)

                def grown():
                    for t0 in range(0, T, TC):
                        grow.advance(x[t0:t0 + TC])
                    return grow.result_confidence(tol)
                print("  K=%-4d tol=%d 10 chunks growing + conf    %s" % (K, tol, calls(grow.reset, grown, n)), flush=True)
                s.reset()
                plain.reset()
                outs, pouts = ten(s)(), ten(plain)()
                for a, b in zip(outs, pouts):                                             # the five plain outputs: the same bytes
                    for f in b._fields:
                        assert torch.equal(getattr(a, f), getattr(b, f)), f
                nt = sum(o.token_lengths.double() for o in outs)
                att = sum((o.token_lengths > 0).double() for o in outs)                   # (calls that committed: >= 1 attempt each)
                cf = torch.cat([o.token_confidences[o.token_frames >= 0].double() for o in outs])
                st = s.result().status
                print("  K=%-4d tol=%d committed tokens per utterance %.1f in %.1f committing calls, mean confidence %.3f, "
                      "forced slots %d/%d" % (K, tol, float(nt.mean()), float(att.mean()), float(cf.mean()) if cf.numel() else 0.0,
                                              int((st & 1).sum()), B), flush=True)


if __name__ == "__main__":
    main()
