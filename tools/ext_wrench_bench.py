"""Cost of the external wrench (srbdqp_set_external_wrench) on device-buffer solves: the general kernel without a wrench (KERNEL_WRENCH), with a zero wrench
(the MODE = 7 instantiation on the SAME QPs: the cost of the path alone) and with a drawn wrench (other QPs, other iteration counts).
B = 4096, N = 10, fp64, double / mixed / single support, and a ragged fleet of 16,384 QPs over N in {8, 12, 16}: the rows of tools/weights_bench.py.
Wrenches are drawn as in tests/ext_wrench_twin.py; every line is the median of REPS timed blocks of K calls (wall clock around torch.cuda.synchronize()),
the variants interleaved block by block.

The baseline runs on the library given with --baseline-lib (a libsrbdqp.so built from the parent commit, loaded beside this tree's through ctypes: the two
share the process's HIP runtime and nothing else); without the option it is this tree's own KERNEL_WRENCH handle.
    python tools/ext_wrench_bench.py [--reps 7] [--k 20] [--baseline-lib PATH]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np
import torch

from g1_locomotion_amd import BatchMPC, RaggedMPC, _lib, synth
import benchlib as bl

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--baseline-lib", default=None)
args = ap.parse_args()
dev = bl.dev
BASE = "general (no wrench" + (", parent lib)" if args.baseline_lib else ")")


def draw(shape, seed):
    """A constant push per QP (torque +-4 N m, force +-40 N) plus a per-row part (+-1 N m, +-10 N); shape = (B, N) or, on a ragged fleet, its row counts."""
    rng = np.random.default_rng(seed)
    amp_c, amp_s = np.array([4.0] * 3 + [40.0] * 3), np.array([1.0] * 3 + [10.0] * 3)
    if isinstance(shape, tuple):
        B, N = shape
        return rng.uniform(-1.0, 1.0, (B, 1, 6)) * amp_c + rng.uniform(-1.0, 1.0, (B, N, 6)) * amp_s
    const = np.repeat(rng.uniform(-1.0, 1.0, (len(shape), 6)) * amp_c, shape, axis=0)
    return const + rng.uniform(-1.0, 1.0, (int(np.sum(shape)), 6)) * amp_s


parent = bl.Parent(args.baseline_lib) if args.baseline_lib else None


def compare(label, B, runs):
    bl.compare(label, B, runs, args.reps, args.k, 32, "baseline")


def batch_case(schedule, B=4096, N=10):
    d, u, st, it = bl.batch_buffers(*synth.synthetic_batch(B, N, seed=11, schedule=schedule))
    engs = dict(zero=BatchMPC(horizon=N), drawn=BatchMPC(horizon=N))
    if not parent:
        engs["general"] = BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH)
    recs = dict(zero=torch.zeros((B, N, 6), dtype=torch.float64, device=dev), drawn=torch.from_numpy(draw((B, N), 12)).to(dev))
    for k, v in recs.items():
        engs[k].set_external_wrench(v)

    def mk(e):
        return bl.device_call(e, d, u, st, it)
    if parent:
        hp = parent.batch(N, _lib.KERNEL_WRENCH)
        base = lambda: parent.lib.srbdqp_solve_batch_device_f64(hp, B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), None, None, None,
                                                                u.data_ptr(), None, None, st.data_ptr(), it.data_ptr(), None)
        assert base() == _lib.OK
    else:
        base = mk(engs["general"])
    compare(f"B={B} N={N} fp64 {schedule}", B, {BASE: base, "zero wrench": mk(engs["zero"]), "wrench drawn": mk(engs["drawn"])})
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
    rows = int(Nq.sum())
    r_uni, r_rec = torch.zeros((rows, 6), dtype=torch.float64, device=dev), torch.from_numpy(draw(Nq, 13)).to(dev)
    uni.set_external_wrench(r_uni)
    rec.set_external_wrench(r_rec)

    def mk(e):
        return bl.device_call(e, d, u, st, it, Nq=Nq)
    if parent:
        hp = parent.ragged(HZ)
        base = lambda: parent.lib.srbdqp_solve_ragged_device_f64(hp, B, Nq.ctypes.data, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                                                 u.data_ptr(), None, st.data_ptr(), it.data_ptr(), None)
        assert base() == _lib.OK
    else:
        base = mk(plain)
    compare(f"ragged B={B} N in {HZ} mixed", B, {BASE: base, "zero wrench": mk(uni), "wrench drawn": mk(rec)})
    torch.cuda.synchronize()
    uni.close(); rec.close()
    if parent:
        parent.lib.srbdqp_ragged_destroy(hp)
    else:
        plain.close()


print(f"ext_wrench_bench: {torch.cuda.get_device_name(0)}  reps={args.reps} k={args.k}  {_lib.load().srbdqp_version().decode()}"
      + (f"  baseline: {args.baseline_lib} ({parent.lib.srbdqp_version().decode()})" if parent else ""), flush=True)
for s in ("double", "mixed", "single"):
    batch_case(s)
ragged_case()
