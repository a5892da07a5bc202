"""What the side-input benches share (robots_bench.py, weights_bench.py, normals_bench.py, rank_aware_bench.py, any_horizon_bench.py): device buffers for a
synthetic batch or a ragged fleet, the two measuring loops, and a second build of the library to measure against."""
import ctypes as C
import time

import numpy as np
import torch

from g1_locomotion_amd import _lib, synth

dev = torch.device("cuda", 0)


def batch_buffers(x0, xr, ft, ct):
    """Device copies of a batch's inputs d = [x0, x_ref, foot, contact] and outputs u (the shape of foot), status, iters."""
    B = x0.shape[0]
    d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (x0, xr, ft, ct.astype(np.uint8))]
    u = torch.empty(ft.shape, dtype=torch.float64, device=dev)
    return d, u, torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)


def device_call(e, d, u, st, it, Nq=None):
    """-> the device-buffer solve of those buffers on engine e (a RaggedMPC with the horizons Nq), as a callable."""
    B, head = len(st), () if Nq is None else (Nq,)
    return lambda: e.solve_device(B, *head, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), status=st.data_ptr(), iters=it.data_ptr())


def ragged_fleet(B=16384, HZ=(8, 12, 16)):
    """A mixed-gait fleet with horizons drawn from HZ, packed step-major in the caller's order -> (N_per_qp, d, u, status, iters)."""
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
    return (Nq,) + batch_buffers(x0, np.concatenate(xr), np.concatenate(ft), np.concatenate(ct))


def wall_clock(runs, reps, k):
    """runs: {name: callable}.  Three warm-up calls each, then `reps` rounds of one timed block of k calls per name (wall clock around
    torch.cuda.synchronize()), the names interleaved block by block -> ({name: median s/call}, {name: (max - min) / median})."""
    for r in runs.values():
        for _ in range(3):
            r()
    ts = {n: [] for n in runs}
    for _ in range(reps):
        for n, r in runs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(k):
                r()
            torch.cuda.synchronize()
            ts[n].append((time.perf_counter() - t) / k)
    med = {n: float(np.median(v)) for n, v in ts.items()}
    return med, {n: (max(v) - min(v)) / med[n] for n, v in ts.items()}


def compare(label, B, runs, reps, k, width, vs):
    """wall_clock(runs), one line per name against the first."""
    med, spread = wall_clock(runs, reps, k)
    base = med[next(iter(runs))]
    for n in runs:
        print(f"{label:34s} {n:{width}s} {med[n] * 1e3:8.3f} ms/call  {B / med[n] / 1e6:7.3f} M QP/s  spread {spread[n] * 100:4.1f} %  "
              f"vs {vs}: {(med[n] / base - 1) * 100:+6.2f} %", flush=True)


def kernel_ms(engs, d, u, st, it, reps):
    """engs: {name: BatchMPC(timing=True)} on one set of buffers.  Three warm-up rounds, then `reps` rounds of one call per name, interleaved call by call:
    srbdqp_last_kernel_ms of every call (restart passes included) -> ({name: [ms]}, {name: (mean iters, solved, rejected) of its last call})."""
    calls = {n: device_call(e, d, u, st, it) for n, e in engs.items()}
    ms, its = {n: [] for n in engs}, {}
    for r in range(reps + 3):
        for n, e in engs.items():
            calls[n]()
            e.synchronize()
            if r >= 3:
                ms[n].append(e.last_kernel_ms())
            its[n] = (float(it.float().mean()), int((st == _lib.SOLVED).sum()), int((st < 0).sum()))
    return ms, its


class Parent:
    """The few calls of the C-ABI a baseline needs, on another build of the library (loaded beside this tree's through ctypes: the two share the process's
    HIP runtime and nothing else)."""
    def __init__(self, path):
        _lib.load()                                                  # (this tree's library first: it maps the HIP runtime both use)
        self.lib = C.CDLL(path)
        for name in ("srbdqp_create", "srbdqp_ragged_create", "srbdqp_destroy", "srbdqp_ragged_destroy", "srbdqp_solve_batch_device_f64",
                     "srbdqp_solve_ragged_device_f64", "srbdqp_version"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]

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
