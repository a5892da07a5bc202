"""What the external wrench costs the single robot's control loop, per call, on the GPU box.

  python tools/staged_wrench_latency.py [--calls 10000] [--parent PATH/libsrbdqp.so] [--last parent|this] [--out FILE]

One QP at N = 10, full double support (the reference's own contact pattern), with a drawn wrench.  p50 / p99 of the host's wall clock around one call -- every
call returns with its results in host memory -- for
  (a) srbdqp_update_f64, no wrench;
  (b) srbdqp_update_wrench_f64;
  (c) MPC.update(external_wrench=) on the default route: the host setter, a host-buffer batch solve of B = 1, the setter again;
  (d) MPC(staged_wrench=True).update(external_wrench=);
  (a_parent) srbdqp_update_f64 on another build of the library (--parent: the parent commit's), in the same process, against
  (a_own_handle) (a) on a handle of this build that never makes a wrench call, as the parent's is.  THE ORDER IN WHICH HANDLES ARE MADE COUNTS: the handle a
  process made last answers 1.2 - 1.3 us sooner than any earlier one, whichever build it is on (measured with a copy of one build under two names).  So the
  two handles are made last, side by side, in the order --last says, and a comparison of two builds is two runs, one per order: like against like is
  a_own_handle of --last this against a_parent of --last parent (both last), and the other two (both second to last);
and, to tell apart what (b) - (a) is made of, (b_zero): (b) with an all-zero block, (a)'s QP bit for bit, with its iteration count.
`calls` calls per row in all, in ten blocks per row, the rows interleaved block by block and their order rotated from block to block (what the box does
meanwhile, and what ran just before, meet every row alike); 200 warm-up calls per row first.  The results of (b) and (d) are held against (c)'s before the timing starts.  Prints one JSON object; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

N = 10


def pct(ts):
    ts = np.asarray(ts) * 1e6
    return {"p50_us": round(float(np.percentile(ts, 50)), 2), "p99_us": round(float(np.percentile(ts, 99)), 2), "min_us": round(float(ts.min()), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10000)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--last", choices=("parent", "this"), default="parent")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime for the process)
    import srbd_oracle as orc
    from g1_locomotion_amd import BatchMPC, MPC, _lib
    x0, xr, ft, ct = orc.synthetic_batch(1, N, seed=99, schedule="double")
    rng = np.random.default_rng(7)
    w = np.concatenate([rng.uniform(-4, 4, (1, 3)) + rng.uniform(-1, 1, (N, 3)), rng.uniform(-40, 40, (1, 3)) + rng.uniform(-10, 10, (N, 3))], axis=1)
    x0c, ctl, ftl = x0[0].reshape(13, 1), ct[0].astype(np.uint8), ft[0].copy()
    rows, info = {}, {}

    # (a), (b): the two C calls with every argument bound to the staging arrays
    eng = BatchMPC(horizon=N)
    st, ew = eng.stage(), eng.stage_ext_wrench()
    st["x0"][0], st["x_ref"][0], st["foot"][0], st["contact"][0], ew[0] = x0[0], xr[0], ft[0], ct[0] != 0, w
    P = lambda v: C.c_void_p(v.ctypes.data)
    raw = _lib.load_raw()
    h = C.c_void_p(eng._h.value)
    args_a = (h, P(st["x0"][0]), P(st["x_ref"][0]), P(st["foot"][0]), P(st["contact"][0]), None, P(st["u"][0]), None, P(st["x"][0]), None, None)
    fn_b, _, args_b = eng.bind_update_wrench()
    rows["a_update_f64"] = lambda: raw.srbdqp_update_f64(*args_a)
    rows["b_update_wrench_f64"] = lambda: fn_b(*args_b)
    eng0 = BatchMPC(horizon=N)                                      # (b_zero: a handle of its own -- its staged wrench array stays zero)
    s0 = eng0.stage()
    s0["x0"][0], s0["x_ref"][0], s0["foot"][0], s0["contact"][0] = x0[0], xr[0], ft[0], ct[0] != 0
    fn_0, _, args_0 = eng0.bind_update_wrench()
    rows["b_zero_wrench"] = lambda: fn_0(*args_0)

    # (c), (d): the Python object on its two routes
    mpcs = {"c_mpc_update_default_route": MPC(horizon=N), "d_mpc_update_staged_wrench": MPC(horizon=N, staged_wrench=True)}
    for m in mpcs.values():
        m.init_matrices()
        m.x_ref_hor[:] = xr[0]
    for name, m in mpcs.items():
        rows[name] = (lambda m: lambda: m.update(ctl, ftl, None, x_current=x0c, external_wrench=w))(m)

    # (a) on the parent's build
    def second_build(path):
        """Another build of the library beside this tree's, a handle on it with the QP staged -> (library, handle, its staging arrays, the bound call)."""
        lib = C.CDLL(os.path.abspath(path))
        for name in ("srbdqp_create", "srbdqp_destroy", "srbdqp_stage_ptrs", "srbdqp_update_f64", "srbdqp_kernel_name"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        cfg = _lib.default_config()
        cfg.horizon = N
        hp = C.c_void_p()
        assert lib.srbdqp_create(C.byref(cfg), C.byref(hp)) == _lib.OK
        sp = _lib.Stage()
        assert lib.srbdqp_stage_ptrs(hp, C.byref(sp)) == _lib.OK
        for addr, v in ((sp.x0, x0[0]), (sp.x_ref, xr[0]), (sp.foot, ft[0])):
            C.memmove(addr, np.ascontiguousarray(v, np.float64).ctypes.data, v.size * 8)
        C.memmove(sp.contact, np.ascontiguousarray(ct[0] != 0, np.uint8).ctypes.data, 4 * N)
        vp = lambda p: C.c_void_p(p)
        args_p = (hp, vp(sp.x0), vp(sp.x_ref), vp(sp.foot), vp(sp.contact), None, vp(sp.u), None, vp(sp.x), None, None)
        return lib, hp, sp, lambda: lib.srbdqp_update_f64(*args_p)

    parent = None
    def own_handle():
        e1 = BatchMPC(horizon=N)                                    # (plain calls only)
        s1 = e1.stage()
        s1["x0"][0], s1["x_ref"][0], s1["foot"][0], s1["contact"][0] = x0[0], xr[0], ft[0], ct[0] != 0
        args_1 = (C.c_void_p(e1._h.value), P(s1["x0"][0]), P(s1["x_ref"][0]), P(s1["foot"][0]), P(s1["contact"][0]), None, P(s1["u"][0]), None, P(s1["x"][0]), None, None)
        rows["a_own_handle"] = lambda: raw.srbdqp_update_f64(*args_1)
        return e1

    # the two handles that are compared, made last and side by side
    if a.parent and a.last == "this":
        parent, hp, sp, rows["a_parent_update_f64"] = second_build(a.parent)
    eng1 = own_handle()
    if a.parent and a.last == "parent":
        parent, hp, sp, rows["a_parent_update_f64"] = second_build(a.parent)

    # warm-up, and the results before any timing
    for r in rows.values():
        for _ in range(200):
            r()
    assert rows["a_update_f64"]() == 0 and int(st["status"][0]) == 1
    info["a_kernel"], info["a_iters"] = eng.kernel_name(), int(st["iters"][0])
    u_plain = st["u"][0].copy()
    info["b_zero_equals_a_bitwise"], info["b_zero_iters"] = bool(np.array_equal(s0["u"][0], u_plain) and np.array_equal(s0["x"][0], st["x"][0])), int(s0["iters"][0])
    if parent:
        up = np.ctypeslib.as_array((C.c_double * (12 * N)).from_address(sp.u)).reshape(N, 12)
        info["a_parent_kernel"] = parent.srbdqp_kernel_name(hp).decode()
        info["a_parent_equals_a_bitwise"] = bool(np.array_equal(up, u_plain))
    assert rows["b_update_wrench_f64"]() == 0 and int(st["status"][0]) == 1
    info["b_kernel"], info["b_iters"], info["launch_path_of_a"] = eng.kernel_name(), int(st["iters"][0]), eng.batch1_launch_path()
    u_b = st["u"][0].copy()
    u_c = mpcs["c_mpc_update_default_route"].update(ctl, ftl, None, x_current=x0c, external_wrench=w)[0]
    u_d = mpcs["d_mpc_update_staged_wrench"].update(ctl, ftl, None, x_current=x0c, external_wrench=w)[0]
    info["c_kernel"] = mpcs["c_mpc_update_default_route"]._engine.kernel_name()
    info["max_du_b_vs_c_N"] = float(np.abs(u_b[0] - u_c.reshape(-1)).max())
    info["max_du_d_vs_c_N"] = float(np.abs(u_d - u_c).max())
    info["wrench_moves_u0_by_N"] = float(np.abs(u_b[0] - u_plain[0]).max())
    assert info["max_du_b_vs_c_N"] < 2e-3 and info["max_du_d_vs_c_N"] < 2e-3 and info["wrench_moves_u0_by_N"] > 1.0, info

    blocks, per = 10, max(1, a.calls // 10)
    ts = {n: [] for n in rows}
    names = list(rows)
    for blk in range(blocks):
        for n in names[blk % len(names):] + names[:blk % len(names)]:
            r = rows[n]
            for _ in range(per):
                t = time.perf_counter()
                r()
                ts[n].append(time.perf_counter() - t)
    out = {"qp": f"N = {N}, full double support, one QP", "handle_made_last": a.last if a.parent else "this", "calls_per_row": blocks * per, **info, "rows": {n: pct(v) for n, v in ts.items()}}
    p50 = {n: out["rows"][n]["p50_us"] for n in rows}
    out["b_over_a"] = round(p50["b_update_wrench_f64"] / p50["a_update_f64"], 4)
    out["b_below_c"] = bool(p50["b_update_wrench_f64"] < p50["c_mpc_update_default_route"])
    if parent:
        out["a_minus_a_parent_us"] = round(p50["a_update_f64"] - p50["a_parent_update_f64"], 2)
        out["a_own_handle_minus_a_parent_us"] = round(p50["a_own_handle"] - p50["a_parent_update_f64"], 2)
        parent.srbdqp_destroy(hp)
    for m in mpcs.values():
        m.close()
    eng.close(); eng0.close(); eng1.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
