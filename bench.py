#!/usr/bin/env python3
"""bench.py -- utterances/s of the ASG forward+backward hot path on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--mode graph|eager] [--launch single|streams|serial]
                    [--graph-steps G] [--dump-outputs DIR] [--full [--no-extra] [--no-cpu-baseline] [--no-pmc]]
                    [--config cfg3|cfg5]

One "step" = ASGLoss(inputs, targets, input_lengths, target_lengths) + loss.backward() on one batch of
synthetic utterances already resident in HBM (SURVEY.md 8d inputs: cfg 3, T=400 B=64 N=40 L=30, fp32).
With N > 1 (launched by torch.distributed.run, one rank per GPU) every rank owns its own B=64 shard of a
B=64*N batch (= cfg 4 at N=8), and the step ends with the single RCCL all-reduce of transition.grad
(SURVEY.md 8e): weak scaling, no other collective.

Timing.  After W warm-up steps, ONE block of EXACTLY K steps is timed between barrier + synchronize fences;
`ms_per_step` is that block / K.  In graph mode G consecutive steps (default: the largest divisor of K up to 10) are
captured into ONE hipGraph and the block replays it K/G times: every step's kernels run in full, back to back on the
stream, as inside a training loop whose host runs ahead of the GPU.  The inputs are drawn from fixed seeds, so the same
arguments give the same inputs in every run; `--dump-outputs DIR` writes what the last timed step computed (loss,
grad_inputs, grad_transition) as DIR/<name>.npy.

Rank 0 prints ONE JSON line.  A plain run carries the driver's contract fields, `config` and `timing` only.  With
`--full` it also carries
  timing.repeated_blocks -- the K-step block repeated (each repetition fenced the same way) until ~0.25 s of steps have
                  run: median / min / max block, since K steps of this workload are a millisecond or two
  roofline     -- dominant kernel (the fused recursion + assembly kernel): algorithmic bytes / its measured duration
  cpu_baseline -- the reference's own compiled CPU path (oracle/_ref) timed on this box's host cores (N=1 only)
  extra        -- (N=1 only) the other BASELINE.json configurations timed in the same process: cfg 2, cfg 4 on one GPU
                  (B=512), B=4096, the evaluation route, eager (no hipGraph) cfg 3, and cfg 5 (large alphabet) with its own
                  roofline object measured live
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch                      # noqa: E402
import torch.distributed as dist  # noqa: E402

T, B, N, L = 400, 64, 40, 30          # BASELINE.json configs[2] ("cfg 3"), per GPU
HBM_PEAK_GBS = 8000.0                 # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec
TARGET_TIMED_S = 0.25                 # wall time the repeated K-step blocks should add up to
DUMP_MAX_ELEMS = 1 << 21              # --dump-outputs: a larger array is written as a fixed seeded sample of this many elements


def algorithmic_bytes(T, B, N, L, w=4):
    """read inputs once + write grad_inputs once; Tr + grad_Tr; targets, lengths, loss."""
    return 2 * T * B * N * w + 2 * N * N * w + B * (8 * L + 16 + w)


def synth(seed, device, T=T, B=B, N=N, L=L, variable=False):
    """SURVEY.md 8(d) draw order (tests/util.py::synth): transition, inputs, targets, then the lengths."""
    g = torch.Generator().manual_seed(seed)
    transition = torch.rand(N, N, generator=g)
    inputs = torch.randn(T, B, N, generator=g)
    targets = torch.randint(0, N, (B, L), generator=g)
    if variable:
        il = torch.randint(T // 2, T + 1, (B,), generator=g)
        tl = torch.randint(max(1, L // 2), L + 1, (B,), generator=g)
    else:
        il = torch.full((B,), T, dtype=torch.int64)
        tl = torch.full((B,), L, dtype=torch.int64)
    return [t.to(device) for t in (transition, inputs, targets, il, tl)]


def cpu_baseline(budget_s=24.0):
    """Time the reference CPU path on this host: the real reference C++ (oracle/_ref) when present,
    else the plain-C oracle port.  Bounded sample of the SAME workload (cfg 3 batches).

    The reference is op-dispatch-bound, so on a many-core host its default thread count is
    far from its best; a small sweep over thread counts is timed and the BEST one is reported (cores = that
    thread count), the others are listed in `sample`."""
    tr, x, tg, il, tl = synth(0, "cpu")
    ncpu = os.cpu_count() or 1
    try:
        from oracle import ref_runner
        if not ref_runner.available():
            raise RuntimeError("no _ref")
        kind = "reference"

        def step():
            ref_runner.asg_loss(x, tg, tr, il, tl, "mean")

        def set_threads(n):
            torch.set_num_threads(n)
            os.environ["OMP_NUM_THREADS"] = str(n)
    except Exception:
        from oracle import asg_oracle as orc
        kind = "port"
        xn, tgn, trn, iln, tln = x.numpy(), tg.numpy(), tr.numpy(), il.numpy(), tl.numpy()

        def step():
            orc.asg_loss(xn, tgn, trn, iln, tln, "mean")

        def set_threads(n):
            import ctypes
            try:
                ctypes.CDLL("libgomp.so.1").omp_set_num_threads(int(n))
            except Exception:
                pass
    default_threads = torch.get_num_threads()
    cands = sorted({n for n in (8, 16, 32, default_threads) if 1 <= n <= ncpu})
    results = {}
    per = budget_s / len(cands)
    for n in cands:
        set_threads(n)
        step()                               # warm-up
        t0 = time.perf_counter()
        reps = 0
        while reps < 2 or (time.perf_counter() - t0 < per and reps < 50):
            step()
            reps += 1
        results[n] = ((time.perf_counter() - t0) / reps, reps)
    set_threads(default_threads)
    best = min(results, key=lambda n: results[n][0])
    dt, reps = results[best]
    return {"value": B / dt, "unit": "utterances/s", "cores": int(best), "kind": kind,
            "ms_per_step": dt * 1e3,
            "sample": "fwd+bwd passes over the cfg-3 batch (T=%d B=%d N=%d L=%d fp32), 1 warm-up + >=2 timed reps per "
                      "thread count, %s, host cpu_count=%d; ms/step by threads: %s (default threads=%d)"
                      % (T, B, N, L, "oracle/_ref = the reference's C++ CPU path built -fopenmp -Ofast"
                         if kind == "reference" else "oracle/asg_oracle.c (OpenMP)", ncpu,
                         ", ".join("%d:%.0f" % (n, results[n][0] * 1e3) for n in cands), default_threads)}


# ------------------------------------------------------------------------------------------------ timing helpers
def graph_steps_for(steps, requested=0):
    g = requested if requested > 0 else max(q for q in range(1, 11) if steps % q == 0)
    return g if steps % g == 0 else 1


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def dump_outputs(path, arrays):
    """--dump-outputs: every tensor of `arrays` as <path>/<name>.npy in its own dtype (float32 / float64).  A tensor of more than
    DUMP_MAX_ELEMS elements is written as <name>_sample.npy: the elements at the same seeded flat indices in every run."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach()
        if t.dtype not in (torch.float32, torch.float64):
            t = t.float()
        if t.numel() > DUMP_MAX_ELEMS:
            idx = torch.randint(0, t.numel(), (DUMP_MAX_ELEMS,), generator=torch.Generator().manual_seed(0))
            t = t.reshape(-1)[idx.to(t.device)]
            name += "_sample"
        np.save(os.path.join(path, name + ".npy"), t.cpu().numpy())


def capture_steps(one_step, gsteps, after_step=None, relaxed=False):
    """A hipGraph of `gsteps` consecutive steps (warmed up on a side stream first, replayed once)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            one_step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local" if relaxed else "global"):
        for _ in range(gsteps):
            one_step()
            if after_step is not None:
                after_step()
    g.replay()
    torch.cuda.synchronize()
    return g


def timed_blocks(step_group, groups_per_block, fence, agree=None, target_s=TARGET_TIMED_S, max_blocks=400):
    """Blocks of groups_per_block step groups, each fenced on both sides; returns the list of block seconds.
    `agree` (multi-rank runs) maps this rank's first block time to one value all ranks share, so that every rank runs
    the same number of blocks (and of barriers)."""
    fence()
    t0 = time.perf_counter()
    for _ in range(groups_per_block):
        step_group()
    fence()
    first = time.perf_counter() - t0
    nblocks = int(min(max_blocks, max(3, target_s / max(agree(first) if agree else first, 1e-6))))
    out = [first]
    for _ in range(nblocks - 1):
        fence()
        t0 = time.perf_counter()
        for _ in range(groups_per_block):
            step_group()
        fence()
        out.append(time.perf_counter() - t0)
    return out


def time_small_config(name, T_, B_, N_, L_, variable, steps, eval_route=False, eager=False, launch="single"):
    """One of the small-alphabet configurations on cuda:0: graph replay (or eager) of forward+backward, or of the
    evaluation route (beta recursions only, no gradient).  Same block protocol as the headline."""
    import torch_asg_amd
    dev = torch.device("cuda", torch.cuda.current_device())
    tr, x, tg, il, tl = synth(7, dev, T_, B_, N_, L_, variable)
    m = torch_asg_amd.ASGLoss(N_, reduction="mean", launch_mode=launch).to(dev)
    with torch.no_grad():
        m.transition.copy_(tr)
    if eval_route:
        m.eval()

        def one_step():
            with torch.no_grad():
                return m(x, tg, il, tl)
    else:
        x.requires_grad_(True)

        def one_step():
            m.transition.grad = None
            x.grad = None
            loss = m(x, tg, il, tl)
            loss.backward()
            return loss
    gsteps = 1 if eager else graph_steps_for(steps)
    if eager:
        for _ in range(5):
            one_step()
        group = one_step
    else:
        # the public helper: `gsteps` consecutive module(...) + loss.backward() recorded into one hipGraph
        group = torch_asg_amd.graphed(m, (x, tg, il, tl), steps=gsteps).graph.replay
    for _ in range(3):
        group()
    blocks = timed_blocks(group, steps // gsteps, torch.cuda.synchronize, target_s=0.12)
    ms = median(blocks) / steps * 1e3
    out = {}
    if launch == "streams":
        # what the library does with launch_mode='streams' (csrc/asg_api.hip::run_forward): eager calls fork the aligned lattice
        # onto a side HIP stream (event fork / join: the reference's arrangement, streamlined_fast_gpu.cpp:121-129,220-225);
        # while the caller's stream is being captured the small path records both lattices on that one stream instead
        # (cross-queue edges of a replayed graph cost more than these short kernels' overlap saves)
        forced = os.environ.get("ASG_FORK_IN_CAPTURE")
        forks = eager or forced == "1"
        out["overlap"] = ("fork: full-lattice chains on the caller's stream, aligned chains on a side HIP stream, event fork/join"
                          if forks else "inline (capturing): both lattices recorded on the caller's stream, no fork -- this is the "
                                        "`serial` arrangement in one call; the fork/join overlap is timed in `cfg3_streams_eager`")
    out.update({"workload": "%s: T=%d B=%d N=%d L=%d fp32%s, %s" % (
                name, T_, B_, N_, L_, ", variable lengths" if variable else "",
                "evaluation route (beta recursions, no gradient)" if eval_route else "forward+backward"),
            "step_mode": "eager" if eager else "graph (%d steps per replay)" % gsteps,
            "ms_per_step": ms, "utt_s": B_ / (ms * 1e-3), "steps": steps, "timed_blocks": len(blocks),
            "algorithmic_bytes": algorithmic_bytes(T_, B_, N_, L_),
            "step_achieved_gbs": algorithmic_bytes(T_, B_, N_, L_) / (ms * 1e-3) / 1e9})
    return out


CFG5 = dict(T=2000, B=32, N=10000, L=60)      # BASELINE.json configs[4]: large alphabet, variable lengths


def measure_cfg5(steps, warmup, dump_dir=None):
    """The large-alphabet workload on the generic kernels (csrc/asg_generic_step.hip, asg_generic_grad.hip).  A step is ASGLoss forward + backward
    on one batch (eager: a step is ~0.4 s of GPU time, launch overhead is nothing).  dump_dir: --dump-outputs of the last timed step.
    The reference cannot run this size at all: fully_connected_lattice.cpp:77 allocates a [T-1,B,N,N] tensor = 25.6 TB."""
    import torch_asg_amd
    from torch_asg_amd import asg as asg_mod
    T5, B5, N5, L5 = CFG5["T"], CFG5["B"], CFG5["N"], CFG5["L"]
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(0)     # drawn on the device: 2.6 GB of emissions
    tr = torch.rand(N5, N5, generator=g, device=dev)
    x = torch.randn(T5, B5, N5, generator=g, device=dev).requires_grad_(True)
    tg = torch.randint(0, N5, (B5, L5), generator=g, device=dev)
    il = torch.randint(T5 // 2, T5 + 1, (B5,), generator=g, device=dev)
    tl = torch.randint(max(1, L5 // 2), L5 + 1, (B5,), generator=g, device=dev)
    m = torch_asg_amd.ASGLoss(N5, reduction="mean").to(dev)
    with torch.no_grad():
        m.transition.copy_(tr)

    def one_step():
        m.transition.grad = None
        x.grad = None
        loss = m(x, tg, il, tl)
        loss.backward()
        return loss

    for _ in range(max(warmup, 1)):
        one_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = one_step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dump_dir:
        dump_outputs(dump_dir, {"loss": loss, "grad_inputs": x.grad, "grad_transition": m.transition.grad})
    # dominant kernel: the recursion over frames (alpha of frame n and beta of frame len-1-n together): forward alone
    # between HIP events / (T - 1) frame steps
    be = asg_mod.native()
    xd, trd = x.detach(), m.transition.detach()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    be.forward(xd, tg, trd, il, tl, 0)
    torch.cuda.synchronize()
    e0.record()
    be.forward(xd, tg, trd, il, tl, 0)
    e1.record()
    torch.cuda.synchronize()
    fwd_ms = e0.elapsed_time(e1)
    frame_steps = T5 - 1
    kern_ms = fwd_ms / frame_steps
    w = 4
    a_alg_step = 2 * N5 * N5 * w + 2 * 2 * B5 * N5 * w        # one frame, both directions: E and F once, vectors in/out
    a_alg = 3 * (T5 - 1) * N5 * N5 * w + 2 * T5 * B5 * N5 * w      # alpha, beta and gradient passes over Tr
    ms_per_step = dt / steps * 1e3
    achieved = a_alg_step / (kern_ms * 1e-3) / 1e9
    traffic5, traffic5_src = committed_traffic(("r06_pmc_cfg5.json", "r05_pmc_cfg5.json"))
    del x, tr, m
    torch.cuda.empty_cache()
    return {
        "workload": "cfg5: T=%d B=%d N=%d L=%d fp32, variable input/target lengths, ASGLoss(reduction=mean) "
                    "forward+backward on the generic (large-alphabet) kernels" % (T5, B5, N5, L5),
        "step_mode": "eager", "steps": steps, "warmup": max(warmup, 1),
        "ms_per_step": ms_per_step, "utt_s": B5 * steps / dt, "loss": float(loss.detach()),
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                     "traffic": traffic5, "traffic_source": traffic5_src, "traffic_measured_in_run": False,
                     "kernel": "the full-lattice recursion, one frame of alpha AND beta for the whole batch per step: the "
                               "row- and column-normalised transition matrices streamed once each per frame",
                     "kernel_ms": kern_ms, "kernel_timing": "HIP events around the forward launch sequence / (T-1) frame steps "
                                                            "(includes the aligned chains and the prologue: < 2 %)",
                     "algorithmic_bytes_per_launch": a_alg_step,
                     "step_algorithmic_bytes": a_alg, "step_achieved": a_alg / (ms_per_step * 1e-3) / 1e9,
                     "note": "A_alg(step) = 3 (T-1) N^2 w + 2 T B N w (SURVEY.md 8d: alpha, beta, gradient passes over Tr; the "
                             "gradient pass here is ONE tiled contraction on the matrix cores that reads Tr once: this formulation "
                             "moves 2 (T-1) N^2 w + N^2 w + 2 T B N w)"},
        "cpu_baseline_note": "the reference cannot run cfg 5 (fully_connected_lattice.cpp:77: 25.6 TB of path_contrib)",
    }


def csrc_sha16():
    """Fingerprint of the kernel sources a counter reading belongs to: sha256 over csrc/*.hip|*.h|*.inc and include/asg_hip.h
    (names and contents, sorted) -- .git does not travel to the GPU box, file contents do."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(ROOT, "torch_asg_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "torch_asg_amd", "csrc", "*.h")) +
                   glob.glob(os.path.join(ROOT, "torch_asg_amd", "csrc", "*.inc")) + [os.path.join(ROOT, "include", "asg_hip.h")])
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def committed_traffic(names, key="dominant_kernel_hbm_bytes_per_launch"):
    """HBM bytes per launch of the dominant kernel from a committed PMC collection (profiles/<tag>_pmc_*.json), and where it came from.
    A file that records the sources it was taken at (`csrc_sha16`) is only used when they are THIS tree's sources: a stale number
    is returned as None with the reason in the source string, never silently."""
    here = csrc_sha16()
    for name in names:
        path = os.path.join(ROOT, "profiles", name)
        if os.path.exists(path):
            try:
                with open(path) as f:
                    d = json.load(f)
                sha, commit = d.get("csrc_sha16"), d.get("commit")
                tag = "profiles/%s (csrc %s%s)" % (name, sha or "unrecorded", ", commit %s" % commit if commit else "")
                if sha is not None and sha != here:
                    return None, tag + " -- STALE: this tree's csrc is %s; re-collect with `python bench.py --pmc-only`" % here
                return float(d[key]), tag
            except Exception:
                pass
    return None, None


PMC_KERNELS = (("fused_fwd_kernel", "dominant_kernel"), ("fused_bwd_kernel", "backward_kernel"))


def collect_pmc_traffic(timeout_s=170):
    """roofline.traffic measured where it is reported: the two counter passes MI355X_MICROARCH.md prescribes -- `rocprofv3 --pmc FETCH_SIZE`
    and `rocprofv3 --pmc WRITE_SIZE`, separate runs, --kernel-trace only -- over tools/pmc_probe.py (a 256 MiB device copy for calibration,
    then 10 eager cfg-3 steps), per launch of the two fused kernels, with the guide's gfx950 correction (FETCH_SIZE x2; the copy of the
    same run is reported so that the factor can be checked).  Returns the dict that also goes to profiles/<tag>_pmc_cfg3.json, or raises."""
    import collections
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        raise RuntimeError("rocprofv3 not found")
    raw = {}
    cal = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="asg_pmc_", dir="/tmp")
        try:
            env = dict(os.environ, TMPDIR="/tmp")
            r = subprocess.run([rocprof, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--",
                                sys.executable, os.path.join(ROOT, "tools", "pmc_probe.py")], cwd="/tmp", env=env,
                               stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=timeout_s / 2)
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                raise RuntimeError("rocprofv3 --pmc %s failed (exit %d): %s" % (counter, r.returncode, r.stderr.decode()[-300:]))
            per = collections.defaultdict(list)
            with open(files[0]) as fh:
                for row in csv.DictReader(fh):
                    if row["Counter_Name"] == counter:
                        per[row["Kernel_Name"]].append(float(row["Counter_Value"]))
            for key, label in PMC_KERNELS:
                v = [x for k, vals in per.items() if key in k for x in vals]
                if not v:
                    raise RuntimeError("no %s launch in the %s pass" % (key, counter))
                raw[(label, counter)] = (sum(v) / len(v), len(v))
            c = [x for k, vals in per.items() if "copyBuffer" in k for x in vals]
            cal[counter] = max(c) if c else None
        finally:
            shutil.rmtree(d, ignore_errors=True)
    out = {"csrc_sha16": csrc_sha16(), "collected_unix": int(time.time()),
           "source": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes, --kernel-trace only) -- python tools/pmc_probe.py "
                     "(10 eager cfg-3 steps; averages per launch); collected by bench.py::collect_pmc_traffic",
           "note": "FETCH_SIZE doubled (gfx950 counts 128-B requests as 64 B: MI355X_MICROARCH.md, HBM); WRITE_SIZE as read; both in KB",
           "calibration_copy_256MiB_raw_kb": {"FETCH_SIZE": cal.get("FETCH_SIZE"), "WRITE_SIZE": cal.get("WRITE_SIZE"), "expected": 262144.0}}
    for _, label in PMC_KERNELS:
        fr, n = raw[(label, "FETCH_SIZE")]
        wr, _ = raw[(label, "WRITE_SIZE")]
        out[label + "_fetch_bytes"] = fr * 2 * 1024
        out[label + "_write_bytes"] = wr * 1024
        out[label + "_hbm_bytes_per_launch"] = fr * 2 * 1024 + wr * 1024
        out[label + "_launches_averaged"] = n
    a = algorithmic_bytes(T, B, N, L)
    out["step_hbm_bytes"] = out["dominant_kernel_hbm_bytes_per_launch"] + out["backward_kernel_hbm_bytes_per_launch"]
    out["algorithmic_bytes_per_step"] = a
    out["step_traffic_over_algorithmic"] = out["step_hbm_bytes"] / a
    try:                                   # scratch copy that `gpurun` merges back (tools/collect_profiles.sh files it under profiles/)
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "pmc_cfg3.json"), "w") as fh:
            json.dump(out, fh, indent=1)
    except OSError:
        pass
    return out


def run_cfg5(args, real_stdout):
    """`--config cfg5`: the large-alphabet workload as the headline of the line (same JSON contract)."""
    torch.cuda.set_device(0)
    r = measure_cfg5(args.steps, args.warmup, args.dump_outputs)
    out = {
        "metric": "utterances/sec fwd+bwd, T=2000 B=32 N=10000 (cfg 5, large alphabet); achieved HBM GB/s vs roofline",
        "value": r["utt_s"], "unit": "utterances/s", "n_gpus": 1, "steps": args.steps, "warmup": r["warmup"],
        "ms_per_step": r["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": r["workload"], "global_batch": CFG5["B"], "T": CFG5["T"], "N": CFG5["N"], "L": CFG5["L"],
                   "step_mode": "eager", "parallelism": "single GPU"},
        "roofline": r["roofline"], "cpu_baseline": None, "cpu_baseline_note": r["cpu_baseline_note"], "loss": r["loss"],
    }
    sys.stdout.flush()
    os.write(real_stdout, (json.dumps(out) + "\n").encode())


def extras(args):
    """The other BASELINE.json configurations, timed in this process (N = 1 only)."""
    ex = {}

    def attempt(key, fn):
        try:
            ex[key] = fn()
        except Exception as e:            # an extra must never cost the headline line
            ex[key] = {"error": "%s: %s" % (type(e).__name__, e)}
        torch.cuda.synchronize()

    attempt("cfg2", lambda: time_small_config("cfg2", 150, 16, 30, 20, False, 100))
    attempt("cfg4_one_gpu", lambda: time_small_config("cfg4 on one GPU", 400, 512, 40, 30, False, 50))
    # not a BASELINE config: the batch size at which the stand-alone route's throughput levels off (round-3 verdict, item 1)
    attempt("batch_4096", lambda: time_small_config("T=400 N=40 L=30 at B=4096 on one GPU (not a BASELINE config)", 400, 4096, 40, 30, False, 20))
    attempt("cfg3_eval", lambda: time_small_config("cfg3", T, B, N, L, False, 100, eval_route=True))
    attempt("cfg3_eager", lambda: time_small_config("cfg3", T, B, N, L, False, 100, eager=True))
    attempt("cfg3_streams", lambda: time_small_config("cfg3, launch_mode=streams", T, B, N, L, False, 50, launch="streams"))
    # the same mode where its fork / join really overlaps the two lattices: eager launches (BASELINE.json configs[2])
    attempt("cfg3_streams_eager", lambda: time_small_config("cfg3, launch_mode=streams", T, B, N, L, False, 50, eager=True, launch="streams"))
    # not a BASELINE config: the shape letter-based speech models give the criterion (a few dozen labels, targets of
    # hundreds of positions, ~10 s of frames) -- S > 64 leaves the fused step for the long-target kernels
    attempt("long_targets", lambda: time_small_config("long targets (not a BASELINE config)", 1000, 64, 40, 200, True, 20))
    # not a BASELINE config either: a word-piece sized alphabet (between cfg 3's 40 labels and cfg 5's 10^4) -- the matrix
    # stays in the registers of a cluster of workgroups for all frames (fwd_cluster_kernel)
    attempt("alphabet_512", lambda: time_small_config("512 labels (not a BASELINE config)", 400, 64, 512, 30, True, 10))
    # and a sub-word sized one that takes a launch per frame (fwd_step_kernel: 48-row tiles here, 252 workgroups) -- verdict r4, Missing #4
    attempt("alphabet_3000", lambda: time_small_config("3000 labels (not a BASELINE config)", 400, 64, 3000, 30, True, 4))
    attempt("cfg5", lambda: measure_cfg5(3, 1))
    return ex


def full_measurements(args, be, step_group, gsteps, fence, use_dist, dev, x, tg, il, tl, loss_mod):
    """--full, on every rank: the headline's K-step block repeated, and the dominant kernel's duration."""
    def agree(v):
        if not use_dist:
            return v
        t = torch.tensor([v], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    blocks = timed_blocks(step_group, args.steps // gsteps, fence, agree)
    if use_dist:
        tb = torch.tensor(blocks, dtype=torch.float64, device=dev)
        dist.all_reduce(tb, op=dist.ReduceOp.MAX)          # every block: the slowest rank's time
        blocks = [float(v) for v in tb.tolist()]

    # ---- dominant-kernel duration, measured live with HIP events on the launch stream: a hipGraph holding ONLY that
    # kernel launch, replayed back to back between one pair of HIP events (launch gaps inside a graph are ~1 us); this is
    # the number that tracks rocprofv3's kernel time.  Fallback: event pairs around single eager launches.
    from torch_asg_amd import _lib as lib_mod
    lflags = {"streams": lib_mod.FLAG_STREAMS, "single": lib_mod.FLAG_SINGLE_LAUNCH, "serial": 0}[args.launch]
    xd = x.detach()
    trd = loss_mod.transition.detach()
    fused_step = args.launch == "single"      # ASGLoss' default route: recursions AND gradient assembly in one launch

    def dominant_launch():
        if fused_step:
            be.loss_forward(xd, tg, trd, il, tl, "mean", lflags)
        else:
            be.forward(xd, tg, trd, il, tl, lflags)

    for _ in range(5):
        dominant_launch()
    torch.cuda.synchronize()
    nk = min(max(args.steps, 20), 200)
    try:
        per_graph = 25
        kg = capture_steps(dominant_launch, per_graph)
        for _ in range(3):
            kg.replay()
        torch.cuda.synchronize()
        reps = []
        for _ in range(max(nk // per_graph, 8)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            kg.replay()
            e1.record()
            torch.cuda.synchronize()
            reps.append(e0.elapsed_time(e1) / per_graph)
        kern_ms_med = median(reps)
        kern_ms_avg = sum(reps) / len(reps)
        kern_method = "HIP events around a hipGraph of %d consecutive launches of this kernel only, per launch" % per_graph
    except Exception as e:
        sys.stderr.write("[bench] single-kernel graph timing failed (%s); eager event pairs\n" % (e,))
        ev_pairs = []
        for _ in range(nk):
            torch.cuda._sleep(400000)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dominant_launch()
            e1.record()
            ev_pairs.append((e0, e1))
        torch.cuda.synchronize()
        kern_ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev_pairs)
        kern_ms_avg = sum(kern_ms) / len(kern_ms)
        kern_ms_med = kern_ms[len(kern_ms) // 2]
        kern_method = "HIP events around single eager launches (includes ~3 us of dispatch)"
    return {"repeated_blocks": {"protocol": "the K-step block repeated, each repetition between barrier + synchronize fences, until "
                                            "~%.2f s of steps have run" % TARGET_TIMED_S,
                                "timed_blocks": len(blocks), "first_block_ms": blocks[0] * 1e3, "min_block_ms": min(blocks) * 1e3,
                                "median_block_ms": median(blocks) * 1e3, "max_block_ms": max(blocks) * 1e3,
                                "median_ms_per_step": median(blocks) / args.steps * 1e3, "total_timed_s": sum(blocks)},
            "fused_step": fused_step, "kern_ms_med": kern_ms_med, "kern_ms_avg": kern_ms_avg, "kern_method": kern_method}


def full_roofline(args, full, ms_per_step, world):
    """--full, rank 0: the `roofline` object of the headline (counter passes for its traffic unless --no-pmc)."""
    fused_step, kern_ms_med = full["fused_step"], full["kern_ms_med"]
    a_alg = algorithmic_bytes(T, B, N, L)
    achieved = a_alg / (kern_ms_med * 1e-3) / 1e9
    traffic, traffic_source, traffic_live, pmc = None, None, False, None
    if fused_step and world == 1 and not args.no_pmc:
        try:
            pmc = collect_pmc_traffic()
            traffic, traffic_live = pmc["dominant_kernel_hbm_bytes_per_launch"], True
            traffic_source = ("measured by this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE (two passes of tools/pmc_probe.py) "
                              "at csrc %s" % pmc["csrc_sha16"])
        except Exception as e:
            sys.stderr.write("[bench] counter passes failed (%s: %s); falling back to the committed collection\n" % (type(e).__name__, e))
    if fused_step and traffic is None:
        traffic, traffic_source = committed_traffic(("r06_pmc_cfg3.json", "r05_pmc_cfg3.json"))
    return {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
            "traffic_measured_in_run": traffic_live,
            "traffic_detail": None if pmc is None else {k: pmc[k] for k in (
                "dominant_kernel_fetch_bytes", "dominant_kernel_write_bytes", "backward_kernel_hbm_bytes_per_launch",
                "step_hbm_bytes", "step_traffic_over_algorithmic", "calibration_copy_256MiB_raw_kb")},
            "kernel": "fused_fwd_kernel (all four recursions of every utterance AND the gradient assembly in "
                      "one launch: three workgroups per utterance)"
                      if fused_step else "asg_forward launches (recursion kernels)",
            "kernel_ms": kern_ms_med, "kernel_ms_avg": full["kern_ms_avg"], "kernel_timing": full["kern_method"],
            "algorithmic_bytes_per_launch": a_alg,
            "step_achieved": a_alg / (ms_per_step * 1e-3) / 1e9,
            "note": "serial-latency-bound scan: 400 dependent steps x 64 utterances; see DESIGN.md",
            # what actually bounds the dominant kernel: T-1 dependent recursion steps at the LDS-broadcast floor of
            # this formulation (117 ns measured for the recursion wavefront alone)
            "latency_floor": {"dependent_steps": T - 1, "ns_per_step": 117.0,
                              "floor_ms": (T - 1) * 117.0e-6,
                              "frac_of_kernel": (T - 1) * 117.0e-6 / kern_ms_med} if fused_step else None}


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(n, real_stdout):
    """`python bench.py --gpus N` without a launcher: re-run this command line under torch.distributed.run (one rank per
    GPU, rendezvous on 127.0.0.1), pass rank 0's JSON line through, fail loudly if the ranks did not all finish."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["ASG_BENCH_SELF_LAUNCHED"] = "1"
    p = subprocess.run(cmd, stdout=subprocess.PIPE, env=env)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    if p.returncode != 0 or len(lines) != 1:
        raise SystemExit("bench.py: the %d-rank run failed (exit code %d, %d JSON lines)" % (n, p.returncode, len(lines)))
    os.write(real_stdout, (lines[0] + "\n").encode())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--mode", choices=["graph", "eager"], default="graph")
    ap.add_argument("--launch", choices=["single", "streams", "serial"], default="single")
    ap.add_argument("--graph-steps", type=int, default=0, help="steps per captured hipGraph (0 = largest divisor of --steps <= 10)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything besides the headline: repeated timed blocks, the dominant kernel's roofline, the "
                         "CPU baseline and the other configurations (`extra`)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip `cpu_baseline`")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the `extra` object (the other configurations)")
    ap.add_argument("--no-pmc", action="store_true",
                    help="with --full: do not run the two rocprofv3 counter passes that measure roofline.traffic (N=1 only; ~40 s); the "
                         "committed collection is used if it belongs to this tree's sources")
    ap.add_argument("--pmc-only", action="store_true", help="run only those two passes, print their JSON (-> profiles/<tag>_pmc_cfg3.json)")
    ap.add_argument("--force-dist", action="store_true", help="init the process group even with one rank (testing)")
    ap.add_argument("--dry-run", action="store_true",
                    help="parse the arguments and the launcher's environment, print the plan as JSON, touch no GPU (tests)")
    ap.add_argument("--config", choices=["cfg3", "cfg5"], default="cfg3",
                    help="cfg3 = BASELINE.json's headline workload (default); cfg5 = the large-alphabet workload, 1 GPU")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    # keep stdout clean for the ONE JSON line: anything libraries print (RCCL banners etc.) goes to stderr
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    if args.pmc_only:
        os.write(real_stdout, (json.dumps(collect_pmc_traffic(), indent=1) + "\n").encode())
        return
    if args.config == "cfg5":
        if "--steps" not in sys.argv:
            args.steps = 3
        if "--warmup" not in sys.argv:
            args.warmup = 1
        return run_cfg5(args, real_stdout)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher -- one rank per GPU under torch.distributed.run on this node
        return self_launch(args.gpus, real_stdout)
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("bench.py --gpus %d was started by a launcher with WORLD_SIZE=%d: launch with --nproc-per-node %d "
                         "(or without a launcher: bench.py then starts its own ranks)" % (args.gpus, world, args.gpus))
    if args.dry_run:
        gs = graph_steps_for(args.steps, args.graph_steps) if args.mode == "graph" else 1
        joined = 1
        if world > 1:        # prove that every rank the launcher started reaches a collective (gloo: no GPU is touched)
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group("gloo", rank=rank, world_size=world)
            one = torch.ones(1, dtype=torch.int64)
            dist.all_reduce(one)
            joined = int(one.item())
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            os.write(real_stdout, (json.dumps({"dry_run": True, "world": world, "gpus": args.gpus, "steps": args.steps,
                                               "warmup": args.warmup, "mode": args.mode, "steps_per_graph": gs,
                                               "global_batch": B * world, "uses_dist": world > 1 or args.force_dist,
                                               "ranks_joined": joined, "n_gpus": joined,
                                               "collective": ("rccl all_reduce(transition.grad), %d rank(s)" % world)
                                                             if (world > 1 or args.force_dist) else "none (one process)",
                                               "self_launched": os.environ.get("ASG_BENCH_SELF_LAUNCHED") == "1",
                                               "master": os.environ.get("MASTER_ADDR", "127.0.0.1")}) + "\n").encode())
        return
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    import torch_asg_amd
    from torch_asg_amd import asg as asg_mod

    tr, x, tg, il, tl = synth(1000 + rank, dev)          # every rank: its own B=64 shard
    loss_mod = torch_asg_amd.ASGLoss(N, reduction="mean", launch_mode=args.launch).to(dev)
    with torch.no_grad():
        loss_mod.transition.copy_(synth(0, dev)[0])      # replicated transition matrix
    x.requires_grad_(True)
    global_batch = B * world

    be = asg_mod.native()
    # local mean over B times 1/world == mean over the global batch (equal shards); the factor enters as the
    # incoming gradient of backward(), i.e. inside the kernels, not as extra elementwise launches
    gscale = torch.full((), 1.0 / world, device=dev)

    def one_step():
        loss_mod.transition.grad = None
        x.grad = None
        loss = loss_mod(x, tg, il, tl)
        loss.backward(gscale)
        return loss

    def sync_grads():
        if use_dist:
            dist.all_reduce(loss_mod.transition.grad, op=dist.ReduceOp.SUM)   # the one collective of the step

    gsteps = graph_steps_for(args.steps, args.graph_steps) if args.mode == "graph" else 1

    # ---- optional hipGraph capture of the compute part of the step (static shapes)
    graph = None
    graph_has_collective = False
    mode = args.mode
    if mode == "graph":
        try:
            for _ in range(2):
                one_step()
            torch.cuda.synchronize()
            sync_grads()                  # the communicator exists (and has run once) before anything is captured
            torch.cuda.synchronize()
            # torch_asg_amd.graphed IS the captured step (the same helper a user calls): static buffers, the 1/world factor
            # as the gradient handed to backward, G consecutive steps per hipGraph
            if use_dist and gsteps > 1:
                try:                     # the all-reduce inside the graph, so that G steps stay one replay
                    # thread_local: RCCL's watchdog thread polls events while this thread captures
                    graph = torch_asg_amd.graphed(loss_mod, (x, tg, il, tl), steps=gsteps, grad_scale=gscale,
                                                  after_step=sync_grads, capture_error_mode="thread_local")
                    graph_has_collective = True
                except Exception as e:
                    sys.stderr.write("[bench] could not capture the all-reduce (%s); one step per graph\n" % (e,))
                    gsteps = 1
                    graph = None
            if graph is None:
                graph = torch_asg_amd.graphed(loss_mod, (x, tg, il, tl), steps=gsteps, grad_scale=gscale)
        except Exception as e:           # capture unsupported in this environment: fall back, say so
            sys.stderr.write("[bench] hipGraph capture failed (%s); running eager\n" % (e,))
            graph = None
            mode = "eager"
            gsteps = 1

    last = {}

    def step_group():                    # gsteps steps
        if graph is not None:
            graph()                      # GraphedStep.__call__: nothing to copy in, one hipGraph replay
            if not graph_has_collective:
                sync_grads()
        else:
            last["loss"] = one_step()
            sync_grads()

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup // gsteps):
        step_group()
    for _ in range(args.warmup % gsteps):      # the rest of the W warm-up steps, one at a time
        one_step()
        sync_grads()

    # ---- the headline: ONE block of exactly `steps` steps (gsteps divides steps), fenced on both sides
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps // gsteps):
        step_group()
    fence()
    dt = time.perf_counter() - t0
    ranks_joined = 1
    if use_dist:
        tb = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tb, op=dist.ReduceOp.MAX)          # the slowest rank's time
        dt = float(tb.item())
        rj = torch.ones(1, dtype=torch.int64, device=dev)
        dist.all_reduce(rj)                                # ranks that ran every timed step and got here
        ranks_joined = int(rj.item())
        if ranks_joined != world:
            raise SystemExit("bench.py: %d of %d ranks reached the end of the timed region" % (ranks_joined, world))
    if args.dump_outputs and rank == 0:
        if graph is not None:
            dump_outputs(args.dump_outputs, {"loss": graph.loss, "grad_inputs": graph.inputs_grad,
                                             "grad_transition": loss_mod.transition.grad})
        else:
            dump_outputs(args.dump_outputs, {"loss": last["loss"], "grad_inputs": x.grad, "grad_transition": loss_mod.transition.grad})

    if args.full:
        full = full_measurements(args, be, step_group, gsteps, fence, use_dist, dev, x, tg, il, tl, loss_mod)
    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        value = global_batch * args.steps / dt
        out = {
            "metric": "utterances/sec fwd+bwd, T=400 B=64 N=40; achieved HBM GB/s vs roofline",
            "value": value,
            "unit": "utterances/s",
            "n_gpus": ranks_joined,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": "cfg3 per GPU: T=%d B=%d N=%d L=%d fp32, full lengths, ASGLoss(reduction=mean) "
                                   "forward+backward%s" % (T, B, N, L, "" if world == 1 else
                                                            "; global batch %d sharded over %d GPUs, one RCCL "
                                                            "all-reduce of transition.grad per step" % (global_batch, world)),
                       "global_batch": global_batch, "per_gpu_batch": B, "T": T, "N": N, "L": L,
                       "step_mode": mode if mode != "graph" else "graph (torch_asg_amd.graphed: %d consecutive steps per hipGraph replay)" % gsteps,
                       "launch_mode": args.launch,
                       "overlap": {"single": "one launch: the four recursions of every utterance (full alpha / beta on two workgroups, both aligned "
                                             "chains on a third) run concurrently on three compute units, gradient assembly inside the "
                                             "same launch -- the full and force-aligned passes overlap without streams; the reference's "
                                             "stream arrangement is launch_mode='streams' (extra.cfg3_streams / cfg3_streams_eager)",
                                   "streams": "full-lattice passes on the caller's stream, aligned passes on a side HIP stream (fork/join); "
                                              "inside a hipGraph the small path records both on one stream",
                                   "serial": "separate launches on one stream"}[args.launch],
                       "collective": ("rccl all_reduce(transition.grad), %d rank(s)" % world) if use_dist else "none (one process)",
                       "graph_has_collective": bool(graph_has_collective),
                       "launcher": "self (bench.py started its ranks)" if os.environ.get("ASG_BENCH_SELF_LAUNCHED") == "1"
                                   else ("torch.distributed.run" if world > 1 else "none"),
                       "parallelism": "batch-sharded x%d" % world},
            "timing": {"protocol": "one block of exactly `steps` steps after `warmup` steps, between barrier + synchronize fences; "
                                   "ms_per_step and value come from that block",
                       "block_ms": dt * 1e3},
        }
        if args.full:
            out["timing"]["repeated_blocks"] = full["repeated_blocks"]
            out["roofline"] = full_roofline(args, full, ms_per_step, world)
            if world == 1 and not args.no_extra:
                out["extra"] = extras(args)
            if world == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline()
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
