"""Cost and gain of rank-aware wrench steps (SRBDQP_FLAG_RANK_AWARE) on device-buffer solves, fp64, QP solves/s, three cases:
  healthy    a configs[1]-like mixed-gait batch (N = 10) on the general kernel (KERNEL_WRENCH), with and without the flag: the SAME QPs, no step takes the new
             coordinates -- the cost of the flag on a healthy fleet;
  n20        an N = 20 double-support batch, with and without the flag: the same;
  tandem     N = 10, feet in tandem on every step (exactly collinear contact points: an unflagged general kernel rejects every QP): the flagged general kernel
             against the dense 4-wave kernel (KERNEL_COMPACT, max_contacts_per_step = 4), the only other kernel that solves these QPs.
Kernel time of each call from SRBDQP_FLAG_TIMING and srbdqp_last_kernel_ms (restart passes included), the variants of a case interleaved call by call, median
over REPS calls after three warm-up rounds, spread = (max - min) / median.  No pass / fail threshold: the numbers go to profiles/ and DESIGN.md.
    python tools/rank_aware_bench.py [--reps 21] [--batch 4096]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np
import torch

from g1_locomotion_amd import BatchMPC, _lib, synth
import benchlib as bl

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--batch", type=int, default=4096)
args = ap.parse_args()


def tandem_batch(B, N, seed):
    """Double support on every step with the right foot on the line of the left one (tests/scenarios.py collinear_contacts, eps = 0)."""
    import scenarios as sc
    x0, xr, ft, ct = synth.synthetic_batch(B, N, seed=seed, schedule="double")
    for b in range(B):
        ft[b] = sc.collinear_contacts(ft[b], ct[b], 0.0, "tandem")
    return x0, xr, ft, ct


def case(tag, N, data, variants):
    """variants: name -> BatchMPC keywords; the first one is the base the others are compared with."""
    B = data[0].shape[0]
    engs = {k: BatchMPC(horizon=N, timing=True, **kw) for k, kw in variants.items()}
    ms, its = bl.kernel_ms(engs, *bl.batch_buffers(*data), args.reps)
    base = float(np.median(ms[next(iter(engs))]))
    for k, e in engs.items():
        med = float(np.median(ms[k]))
        print(f"{tag:8s} B={B} N={N} fp64 {k:22s} {e.kernel_name():20s} {med:8.3f} ms kernel  {B / med / 1e3:7.3f} M QP/s  spread {(max(ms[k]) - min(ms[k])) / med * 100:4.1f} %  "
              f"vs first: {(med / base - 1) * 100:+6.2f} %  mean iters {its[k][0]:6.1f}  solved {its[k][1]}  rejected {its[k][2]}", flush=True)
        e.close()


print(f"rank_aware_bench: {torch.cuda.get_device_name(0)}  reps={args.reps}  {_lib.load().srbdqp_version().decode()}", flush=True)
W = _lib.KERNEL_WRENCH
case("healthy", 10, synth.synthetic_batch(args.batch, 10, seed=11, schedule="mixed"), {"general": dict(kernel=W), "general rank-aware": dict(kernel=W, rank_aware=True)})
case("n20", 20, synth.synthetic_batch(args.batch, 20, seed=11, schedule="double"), {"general": dict(kernel=W), "general rank-aware": dict(kernel=W, rank_aware=True)})
case("tandem", 10, tandem_batch(args.batch, 10, 11), {"dense 4-wave": dict(kernel=_lib.KERNEL_COMPACT, max_contacts_per_step=4),
                                                     "general rank-aware": dict(kernel=W, rank_aware=True), "general (rejects)": dict(kernel=W)})
