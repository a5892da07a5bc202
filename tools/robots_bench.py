"""Cost of per-QP robot records (srbdqp_set_robots) on device-buffer solves: the general kernel without records (KERNEL_WRENCH), with one record per QP
equal to the config (the MODE = 2 instantiation on the SAME QPs: the cost of the path alone) and with drawn records (a heterogeneous fleet: other QPs,
other iteration counts); for single support also the one-wave kernel AUTO picks without records -- what a single-support fleet gives up by setting
records.  B = 4096, N = 10, fp64, double / mixed / single support, and a configs[4]-shaped ragged fleet over the horizons the records support (N in
{8, 12, 16}: N = 24 is refused).  Records are drawn as in tests/test_gpu_robots.py; every line is the median of REPS timed blocks of K calls (wall
clock around torch.cuda.synchronize()), the variants interleaved block by block.
    python tools/robots_bench.py [--reps 7] [--k 20]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch

from g1_locomotion_amd import BatchMPC, RaggedMPC, _lib, synth
from g1_locomotion_amd.mpc import robots_array

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--k", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda", 0)


def draw(B, seed):
    cfg = _lib.default_config()
    rng = np.random.default_rng(seed)
    return robots_array(B, mass=cfg.mass * rng.uniform(0.7, 1.5, B), inertia=np.array(list(cfg.inertia)) * rng.uniform(0.6, 1.6, (B, 3)),
                        mu=rng.uniform(0.3, 1.0, B), fz_min=rng.uniform(0.0, 20.0, B), fz_max=rng.uniform(150.0, 1200.0, B))


def timed(run):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(args.k):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / args.k


def compare(label, B, runs):
    """runs: {name: callable}; interleaved blocks, median per name."""
    for r in runs.values():
        for _ in range(3):
            r()
    ts = {n: [] for n in runs}
    for _ in range(args.reps):
        for n, r in runs.items():
            ts[n].append(timed(r))
    med = {n: float(np.median(v)) for n, v in ts.items()}
    spread = {n: (max(v) - min(v)) / med[n] for n, v in ts.items()}
    names = list(runs)
    base = med[names[0]]
    for n in names:
        print(f"{label:34s} {n:22s} {med[n] * 1e3:8.3f} ms/call  {B / med[n] / 1e6:7.3f} M QP/s  spread {spread[n] * 100:4.1f} %  "
              f"vs {names[0]}: {(med[n] / base - 1) * 100:+6.2f} %", flush=True)


def batch_case(schedule, B=4096, N=10):
    x0, xr, ft, ct = synth.synthetic_batch(B, N, seed=11, schedule=schedule)
    d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (x0, xr, ft, ct.astype(np.uint8))]
    u = torch.empty((B, N, 12), dtype=torch.float64, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev); it = torch.empty(B, dtype=torch.int32, device=dev)
    engs = dict(general=BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH), uniform=BatchMPC(horizon=N), drawn=BatchMPC(horizon=N), auto=BatchMPC(horizon=N, max_contacts_per_step=2))
    recs = dict(uniform=torch.from_numpy(robots_array(B)).to(dev), drawn=torch.from_numpy(draw(B, 12)).to(dev))
    for k, v in recs.items():
        engs[k].set_robots(v)

    def mk(e):
        return lambda: e.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(),
                                      status=st.data_ptr(), iters=it.data_ptr())
    runs = {"general (no records)": mk(engs["general"]), "records = config": mk(engs["uniform"]), "records drawn": mk(engs["drawn"])}
    if schedule == "single":                      # (AUTO with the single-support bound, as bench.py runs configs[1]: the one-wave kernel)
        runs["AUTO, bound 2 (no records)"] = mk(engs["auto"])
    else:
        engs.pop("auto").close()
    compare(f"B={B} N={N} fp64 {schedule}", B, runs)
    names = {n: e.kernel_name() for n, e in engs.items()}
    for e in engs.values():
        e.close()
    print(f"{'':34s} kernels: {names}", flush=True)


def ragged_case(B=16384, HZ=(8, 12, 16)):
    rng = np.random.default_rng(4)
    Nq = rng.choice(HZ, size=B).astype(np.int32)
    x0 = np.empty((B, 13)); xr, ft, ct = [], [], []
    by, pos = {}, {N: 0 for N in HZ}
    for N in HZ:
        idx = np.where(Nq == N)[0]
        by[N] = synth.synthetic_batch(len(idx), N, seed=40 + N, schedule="mixed")
    for b in range(B):
        N = int(Nq[b]); a, b_, c, d_ = by[N]; i = pos[N]; pos[N] += 1
        x0[b] = a[i]; xr.append(b_[i]); ft.append(c[i].reshape(N, 12)); ct.append(d_[i].reshape(N, 4))
    xr, ft, ct = np.concatenate(xr), np.concatenate(ft), np.concatenate(ct).astype(np.uint8)
    rows = int(Nq.sum())
    d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (x0, xr, ft, ct)]
    u = torch.empty((rows, 12), dtype=torch.float64, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev); it = torch.empty(B, dtype=torch.int32, device=dev)
    plain, uni, rec = RaggedMPC(horizons=HZ), RaggedMPC(horizons=HZ), RaggedMPC(horizons=HZ)
    r_uni, r_rec = torch.from_numpy(robots_array(B)).to(dev), torch.from_numpy(draw(B, 13)).to(dev)
    uni.set_robots(r_uni)
    rec.set_robots(r_rec)

    def mk(e):
        return lambda: e.solve_device(B, Nq, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(),
                                      status=st.data_ptr(), iters=it.data_ptr())
    compare(f"ragged B={B} N in {HZ} mixed", B, {"general (no records)": mk(plain), "records = config": mk(uni), "records drawn": mk(rec)})
    plain.close(); uni.close(); rec.close()


print(f"robots_bench: {torch.cuda.get_device_name(0)}  reps={args.reps} k={args.k}  {_lib.load().srbdqp_version().decode()}", flush=True)
for s in ("double", "mixed", "single"):
    batch_case(s)
ragged_case()
