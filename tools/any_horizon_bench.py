"""Cost of a live horizon (SRBDQP_FLAG_ANY_HORIZON) on device-buffer solves: for each tabulated N* in {8, 10, 12, 16, 20, 24} and the schedules double and
mixed, horizon N* itself on the general kernel without the flag (KERNEL_WRENCH: the MODE = 0 instantiation), horizon N* - 1 with the flag (the MODE = 3
instantiation for the same N*, one step less of everything) and horizon N* - 3 beside it (which should fall roughly with n_g).  B = 4096, fp64, the
automatic rho restart of each horizon.  Every line is the median of REPS timed blocks of K calls (wall clock around torch.cuda.synchronize()), the three
horizons interleaved block by block; the acceptance line is  median(N* - 1) / median(N*) <= 1 + spread,  spread = the larger (max - min) / median of
the two.
    python tools/any_horizon_bench.py [--reps 7] [--k 20] [--nstar 8 10 ...]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import torch

from g1_locomotion_amd import BatchMPC, _lib, synth
import benchlib as bl

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--nstar", type=int, nargs="*", default=[8, 10, 12, 16, 20, 24])
args = ap.parse_args()


def case(nstar, schedule):
    B = args.batch
    runs, engs, iters = {}, {}, {}
    for n in (nstar, nstar - 1, nstar - 3):
        d, u, st, iters[n] = bl.batch_buffers(*synth.synthetic_batch(B, n, seed=11, schedule=schedule))
        engs[n] = BatchMPC(horizon=n, kernel=_lib.KERNEL_WRENCH)       # (the wrapper sets the flag for n outside the tabulated set, and only then)
        runs[n] = bl.device_call(engs[n], d, u, st, iters[n])
    med, spread = bl.wall_clock(runs, args.reps, args.k)
    mean_it = {n: float(it.float().mean()) for n, it in iters.items()}  # (every call of a horizon solves the same QPs)
    names = {n: e.kernel_name() for n, e in engs.items()}
    for e in engs.values():
        e.close()
    for n in runs:
        print(f"N*={nstar:2d} {schedule:6s} n={n:2d} {names[n]:20s} {med[n] * 1e3:8.3f} ms/call  {B / med[n] / 1e6:7.3f} M QP/s  spread {spread[n] * 100:4.1f} %  "
              f"mean iters {mean_it[n]:5.1f}  vs n={nstar}: {med[n] / med[nstar]:6.3f}", flush=True)
    ratio, line = med[nstar - 1] / med[nstar], 1.0 + max(spread[nstar], spread[nstar - 1])
    print(f"N*={nstar:2d} {schedule:6s} acceptance: median(n={nstar - 1}) / median(n={nstar}) = {ratio:.3f} <= {line:.3f}: {'ok' if ratio <= line else 'MISSED'}", flush=True)
    return ratio <= line


print(f"any_horizon_bench: {torch.cuda.get_device_name(0)}  B={args.batch} reps={args.reps} k={args.k}  {_lib.load().srbdqp_version().decode()}", flush=True)
ok = [case(ns, s) for ns in args.nstar for s in ("double", "mixed")]
print(f"{sum(ok)} of {len(ok)} cases inside the acceptance line", flush=True)
