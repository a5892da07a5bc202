"""Cost of per-QP cost weights (srbdqp_set_weights) on device-buffer solves: the general kernel without weights (KERNEL_WRENCH), with one record per QP
equal to the config (the MODE = 6 instantiation on the SAME QPs: the cost of the path alone) and with drawn weights (other QPs, other iteration counts).
B = 4096, N = 10, fp64, double / mixed / single support, and a ragged fleet of 16,384 QPs over N in {8, 12, 16}: the rows of tools/robots_bench.py.
Weights are drawn as in tests/weights_twin.py; every line is the median of REPS timed blocks of K calls (wall clock around torch.cuda.synchronize()), the
variants interleaved block by block.

The baseline runs on the library given with --baseline-lib (a libsrbdqp.so built from the parent commit, loaded beside this tree's through ctypes: the two
share the process's HIP runtime and nothing else); without the option it is this tree's own KERNEL_WRENCH handle.
    python tools/weights_bench.py [--reps 7] [--k 20] [--baseline-lib PATH]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch

from g1_locomotion_amd import BatchMPC, RaggedMPC, _lib, synth
from g1_locomotion_amd.mpc import weights_array

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--baseline-lib", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
BASE = "general (no weights" + (", parent lib)" if args.baseline_lib else ")")


def draw(B, seed):
    cfg = _lib.default_config()
    rng = np.random.default_rng(seed)
    q = np.array(list(cfg.q_diag)) * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 13)))
    return weights_array(B, q_diag=q, r_diag=cfg.r_diag * np.exp(rng.uniform(np.log(0.1), np.log(10.0), B)))


class Parent:
    """The few calls of the C-ABI the baseline needs, on another build of the library."""
    def __init__(self, path):
        _lib.load()                                                  # (this tree's library first: it maps the HIP runtime both use)
        self.lib = C.CDLL(path)
        H, p = C.c_void_p, C.c_void_p
        self.lib.srbdqp_create.argtypes = [C.POINTER(_lib.Config), C.POINTER(H)]
        self.lib.srbdqp_ragged_create.argtypes = [C.POINTER(_lib.Config), C.c_void_p, C.c_int32, C.POINTER(H)]
        self.lib.srbdqp_destroy.argtypes = self.lib.srbdqp_ragged_destroy.argtypes = [H]
        self.lib.srbdqp_solve_batch_device_f64.argtypes = [H, C.c_int32] + [p] * 13
        self.lib.srbdqp_solve_ragged_device_f64.argtypes = [H, C.c_int32] + [p] * 10
        self.lib.srbdqp_version.restype = C.c_char_p

    def batch(self, N, kernel):
        cfg = _lib.default_config()
        cfg.horizon, cfg.kernel = N, kernel
        h = C.c_void_p()
        assert self.lib.srbdqp_create(C.byref(cfg), C.byref(h)) == _lib.OK
        return h

    def ragged(self, HZ):
        cfg = _lib.default_config()
        hz = np.asarray(HZ, np.int32)
        h = C.c_void_p()
        assert self.lib.srbdqp_ragged_create(C.byref(cfg), hz.ctypes.data, len(hz), C.byref(h)) == _lib.OK
        return h


parent = Parent(args.baseline_lib) if args.baseline_lib else None


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
        print(f"{label:34s} {n:32s} {med[n] * 1e3:8.3f} ms/call  {B / med[n] / 1e6:7.3f} M QP/s  spread {spread[n] * 100:4.1f} %  "
              f"vs baseline: {(med[n] / base - 1) * 100:+6.2f} %", flush=True)


def batch_case(schedule, B=4096, N=10):
    x0, xr, ft, ct = synth.synthetic_batch(B, N, seed=11, schedule=schedule)
    d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (x0, xr, ft, ct.astype(np.uint8))]
    u = torch.empty((B, N, 12), dtype=torch.float64, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev); it = torch.empty(B, dtype=torch.int32, device=dev)
    engs = dict(uniform=BatchMPC(horizon=N), drawn=BatchMPC(horizon=N))
    if not parent:
        engs["general"] = BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH)
    recs = dict(uniform=torch.from_numpy(weights_array(B)).to(dev), drawn=torch.from_numpy(draw(B, 12)).to(dev))
    for k, v in recs.items():
        engs[k].set_weights(v)

    def mk(e):
        return lambda: e.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(),
                                      status=st.data_ptr(), iters=it.data_ptr())
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
    uni, rec = RaggedMPC(horizons=HZ), RaggedMPC(horizons=HZ)
    plain = None if parent else RaggedMPC(horizons=HZ)
    r_uni, r_rec = torch.from_numpy(weights_array(B)).to(dev), torch.from_numpy(draw(B, 13)).to(dev)
    uni.set_weights(r_uni)
    rec.set_weights(r_rec)

    def mk(e):
        return lambda: e.solve_device(B, Nq, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(),
                                      status=st.data_ptr(), iters=it.data_ptr())
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
