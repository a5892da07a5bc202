"""Cost of contact normals (srbdqp_set_contact_normals) on device-buffer solves, B = 4096, fp64, double support: the general kernel without normals
(KERNEL_WRENCH: wrench_f64_n<N>), the MODE = 4 instantiation with every normal e_z (the SAME QPs: the cost of the path alone) and with tilted normals (one
per foot, tilt up to 0.35 rad as in tests/test_gpu_contact_normals.py: other QPs, other iteration counts).  Kernel time of each call from SRBDQP_FLAG_TIMING
and srbdqp_last_kernel_ms (restart passes included), the variants interleaved call by call, median over REPS calls; the occupancy of the instantiations is
in the build log (tools/resource_table.py).
    python tools/normals_bench.py [--reps 21] [--horizons 10]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np
import torch

from g1_locomotion_amd import BatchMPC, _lib, synth
import benchlib as bl

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--horizons", type=int, nargs="+", default=[10])
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--schedule", default="double")
args = ap.parse_args()
dev = bl.dev


def tilted(B, N, seed, max_tilt=0.35):
    rng = np.random.default_rng(seed)
    tilt, az = rng.uniform(0.0, max_tilt, (B, 1, 2)), rng.uniform(-np.pi, np.pi, (B, 1, 2))
    n = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], -1)
    return np.repeat(np.broadcast_to(n, (B, N, 2, 3)), 2, axis=2).reshape(B, N, 12).copy()


def case(B, N, schedule):
    buf = bl.batch_buffers(*synth.synthetic_batch(B, N, seed=11, schedule=schedule))
    flat = np.zeros((B, N, 4, 3)); flat[..., 2] = 1.0
    nrm = {"normals e_z": torch.from_numpy(flat.reshape(B, N, 12)).to(dev), "normals tilted": torch.from_numpy(tilted(B, N, 12)).to(dev)}
    engs = {k: BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH, timing=True) for k in ("no normals", "normals e_z", "normals tilted")}
    for k, v in nrm.items():
        engs[k].set_contact_normals(v)
    ms, its = bl.kernel_ms(engs, *buf, args.reps)
    base = float(np.median(ms["no normals"]))
    for k, e in engs.items():
        med = float(np.median(ms[k]))
        print(f"B={B} N={N} fp64 {schedule:7s} {k:15s} {e.kernel_name():20s} {med:8.3f} ms kernel  {B / med / 1e3:7.3f} M QP/s  spread {(max(ms[k]) - min(ms[k])) / med * 100:4.1f} %  "
              f"vs no normals: {(med / base - 1) * 100:+6.2f} %  mean iters {its[k][0]:6.1f}  solved {its[k][1]}", flush=True)
        e.close()


print(f"normals_bench: {torch.cuda.get_device_name(0)}  reps={args.reps}  {_lib.load().srbdqp_version().decode()}", flush=True)
for N in args.horizons:
    case(args.batch, N, args.schedule)
