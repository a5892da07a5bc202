"""Cost of per-QP cost weights (srbdqp_set_weights) on device-buffer solves: the general kernel without weights (KERNEL_WRENCH), with one record per QP
equal to the config (the MODE = 6 instantiation on the SAME QPs: the cost of the path alone) and with drawn weights (other QPs, other iteration counts).
B = 4096, N = 10, fp64, double / mixed / single support, and a ragged fleet of 16,384 QPs over N in {8, 12, 16}: the rows of tools/robots_bench.py.
Weights are drawn as in tests/weights_twin.py; every line is the median of REPS timed blocks of K calls (wall clock around torch.cuda.synchronize()), the
variants interleaved block by block.

The baseline runs on the library given with --baseline-lib (a libsrbdqp.so built from the parent commit, loaded beside this tree's through ctypes: the two
share the process's HIP runtime and nothing else); without the option it is this tree's own KERNEL_WRENCH handle.
    python tools/weights_bench.py [--reps 7] [--k 20] [--baseline-lib PATH]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np
import torch

from g1_locomotion_amd import BatchMPC, RaggedMPC, _lib, synth
from g1_locomotion_amd.mpc import weights_array
import benchlib as bl

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--baseline-lib", default=None)
args = ap.parse_args()
dev = bl.dev
BASE = "general (no weights" + (", parent lib)" if args.baseline_lib else ")")


def draw(B, seed):
    cfg = _lib.default_config()
    rng = np.random.default_rng(seed)
    q = np.array(list(cfg.q_diag)) * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 13)))
    return weights_array(B, q_diag=q, r_diag=cfg.r_diag * np.exp(rng.uniform(np.log(0.1), np.log(10.0), B)))


parent = bl.Parent(args.baseline_lib) if args.baseline_lib else None


def compare(label, B, runs):
    bl.compare(label, B, runs, args.reps, args.k, 32, "baseline")


def batch_case(schedule, B=4096, N=10):
    d, u, st, it = bl.batch_buffers(*synth.synthetic_batch(B, N, seed=11, schedule=schedule))
    engs = dict(uniform=BatchMPC(horizon=N), drawn=BatchMPC(horizon=N))
    if not parent:
        engs["general"] = BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH)
    recs = dict(uniform=torch.from_numpy(weights_array(B)).to(dev), drawn=torch.from_numpy(draw(B, 12)).to(dev))
    for k, v in recs.items():
        engs[k].set_weights(v)

    def mk(e):
        return bl.device_call(e, d, u, st, it)
    if parent:
        hp = parent.batch(N, _lib.KERNEL_WRENCH)
        base = lambda: parent.lib.srbdqp_solve_batch_device_f64(hp, B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), None, None, None,
                                                                u.data_ptr(), None, None, st.data_ptr(), it.data_ptr(), None)
        assert base() == _lib.OK
    else:
        base = mk(engs["general"])
    compare(f"B={B} N={N} fp64 {schedule}", B, {BASE: base, "weights = config": mk(engs["uniform"]), "weights drawn": mk(engs["drawn"])})
    names = {n: e.kernel_name() for n, e in engs.items()}
    for e in engs.values():
        e.close()
    if parent:
        parent.lib.srbdqp_destroy(hp)
    print(f"{'':34s} kernels: {names}", flush=True)


def ragged_case(B=16384, HZ=(8, 12, 16)):
    Nq, d, u, st, it = bl.ragged_fleet(B, HZ)
    uni, rec = RaggedMPC(horizons=HZ), RaggedMPC(horizons=HZ)
    plain = None if parent else RaggedMPC(horizons=HZ)
    r_uni, r_rec = torch.from_numpy(weights_array(B)).to(dev), torch.from_numpy(draw(B, 13)).to(dev)
    uni.set_weights(r_uni)
    rec.set_weights(r_rec)

    def mk(e):
        return bl.device_call(e, d, u, st, it, Nq=Nq)
    if parent:
        hp = parent.ragged(HZ)
        base = lambda: parent.lib.srbdqp_solve_ragged_device_f64(hp, B, Nq.ctypes.data, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                                                 u.data_ptr(), None, st.data_ptr(), it.data_ptr(), None)
        assert base() == _lib.OK
    else:
        base = mk(plain)
    compare(f"ragged B={B} N in {HZ} mixed", B, {BASE: base, "weights = config": mk(uni), "weights drawn": mk(rec)})
    torch.cuda.synchronize()
    uni.close(); rec.close()
    if parent:
        parent.lib.srbdqp_ragged_destroy(hp)
    else:
        plain.close()


print(f"weights_bench: {torch.cuda.get_device_name(0)}  reps={args.reps} k={args.k}  {_lib.load().srbdqp_version().decode()}"
      + (f"  baseline: {args.baseline_lib} ({parent.lib.srbdqp_version().decode()})" if parent else ""), flush=True)
for s in ("double", "mixed", "single"):
    batch_case(s)
ragged_case()
