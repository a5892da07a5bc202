"""What sloped ground costs the single robot's control loop, per call, on the GPU box -- and whether the calls that existed have moved.

  python tools/staged_normals_latency.py [--calls 10000] [--parent PATH/libsrbdqp.so] [--own PATH/other_copy.so] [--last parent|this] [--out FILE]

One QP at N = 10, full double support (the reference's own contact pattern), with drawn contact normals (one per foot and step, tilt up to 0.35 rad).  p50 / p99
of the host's wall clock around one call -- every call returns with its results in host memory -- for
  (a) srbdqp_update_f64, flat ground;
  (b) srbdqp_update_normals_f64 with the drawn normals, and (b_flat) with (0, 0, 1) everywhere -- (a)'s QP to rounding: the price of the form;
  (c) MPC.update(contact_normals=) on the default route: the host setter, a host-buffer batch solve of B = 1, the setter again;
  (d) MPC(staged_normals=True).update(contact_normals=);
and, for the calls that existed, on two handles MADE LAST, side by side (tools/staged_wrench_latency.py has why: the handle a process made last answers 1.2 us
sooner than any earlier one, whichever build it is on), each with a plain and a wrench call:
  (a_own_handle, w_own_handle) srbdqp_update_f64 and srbdqp_update_wrench_f64 on a handle of this build that never makes a normals call
  (a_parent, w_parent)         the same two on another build of the library (--parent: the parent commit's), in the same process.
--last says which of the two is made last; a comparison of two builds is two runs, one per order: like against like is *_own_handle of --last this against
*_parent of --last parent (both last), and the other two (both second to last).  --own PATH puts the "own" handle on a second build too (a COPY of the parent's
library under another name): the same two runs then show what the comparison reads when nothing differs -- the margin.
`calls` calls per row in all, in ten blocks per row, the rows interleaved block by block and their order rotated from block to block; 200 warm-up calls per row
first.  The results of (b) and (d) are held against (c)'s before the timing starts.  Prints one JSON object; --out also writes it to a file."""
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
    ap.add_argument("--own", default=None)
    ap.add_argument("--last", choices=("parent", "this"), default="parent")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime for the process)
    import srbd_oracle as orc
    from g1_locomotion_amd import BatchMPC, MPC, _lib
    x0, xr, ft, ct = orc.synthetic_batch(1, N, seed=99, schedule="double")
    rng = np.random.default_rng(7)
    tilt, az = rng.uniform(0.0, 0.35, (N, 2)), rng.uniform(-np.pi, np.pi, (N, 2))
    nr = np.repeat(np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], -1), 2, axis=1).reshape(N, 12)   # (heel and toe of a foot share its normal)
    w = np.concatenate([rng.uniform(-4, 4, (1, 3)) + rng.uniform(-1, 1, (N, 3)), rng.uniform(-40, 40, (1, 3)) + rng.uniform(-10, 10, (N, 3))], axis=1)
    x0c, ctl, ftl = x0[0].reshape(13, 1), ct[0].astype(np.uint8), ft[0].copy()
    rows, info = {}, {}
    P = lambda v: C.c_void_p(v.ctypes.data)
    raw = _lib.load_raw()

    def staged(e):
        s = e.stage()
        s["x0"][0], s["x_ref"][0], s["foot"][0], s["contact"][0] = x0[0], xr[0], ft[0], ct[0] != 0
        return s, (C.c_void_p(e._h.value), P(s["x0"][0]), P(s["x_ref"][0]), P(s["foot"][0]), P(s["contact"][0]), None, P(s["u"][0]), None, P(s["x"][0]), None, None)

    # (a), (b): the two C calls with every argument bound to the staging arrays
    eng = BatchMPC(horizon=N)
    st, args_a = staged(eng)
    eng.stage_contact_normals()[0] = nr
    fn_b, _, args_b = eng.bind_update_normals()
    rows["a_update_f64"] = lambda: raw.srbdqp_update_f64(*args_a)
    rows["b_update_normals_f64"] = lambda: fn_b(*args_b)
    eng0 = BatchMPC(horizon=N)                                      # (b_flat: a handle of its own -- its staged normals array stays (0, 0, 1))
    s0, _ = staged(eng0)
    fn_0, _, args_0 = eng0.bind_update_normals()
    rows["b_flat_normals"] = lambda: fn_0(*args_0)

    # (c), (d): the Python object on its two routes
    mpcs = {"c_mpc_update_default_route": MPC(horizon=N), "d_mpc_update_staged_normals": MPC(horizon=N, staged_normals=True)}
    for m in mpcs.values():
        m.init_matrices()
        m.x_ref_hor[:] = xr[0]
    for name, m in mpcs.items():
        rows[name] = (lambda m: lambda: m.update(ctl, ftl, None, x_current=x0c, contact_normals=nr))(m)

    def second_build(path, tag):
        """Another build of the library beside this tree's, a handle on it with the QP and a wrench staged; its plain and its wrench call as rows a_<tag>, w_<tag>
        -> (library, handle, its staging arrays)."""
        lib = C.CDLL(os.path.abspath(path))
        for name in ("srbdqp_create", "srbdqp_destroy", "srbdqp_stage_ptrs", "srbdqp_update_f64", "srbdqp_kernel_name", "srbdqp_stage_ext_wrench", "srbdqp_update_wrench_f64"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        cfg = _lib.default_config()
        cfg.horizon = N
        hp = C.c_void_p()
        assert lib.srbdqp_create(C.byref(cfg), C.byref(hp)) == _lib.OK
        sp = _lib.Stage()
        assert lib.srbdqp_stage_ptrs(hp, C.byref(sp)) == _lib.OK
        ew = C.c_void_p()
        assert lib.srbdqp_stage_ext_wrench(hp, C.byref(ew)) == _lib.OK
        for addr, v in ((sp.x0, x0[0]), (sp.x_ref, xr[0]), (sp.foot, ft[0]), (ew.value, w)):
            C.memmove(addr, np.ascontiguousarray(v, np.float64).ctypes.data, v.size * 8)
        C.memmove(sp.contact, np.ascontiguousarray(ct[0] != 0, np.uint8).ctypes.data, 4 * N)
        vp = lambda p: C.c_void_p(p)
        ins = (hp, vp(sp.x0), vp(sp.x_ref), vp(sp.foot), vp(sp.contact), None)
        outs = (vp(sp.u), None, vp(sp.x), None, None)
        rows["a_" + tag] = lambda: lib.srbdqp_update_f64(*ins, *outs)
        rows["w_" + tag] = lambda: lib.srbdqp_update_wrench_f64(*ins, ew, *outs)
        return lib, hp, sp

    seconds = []

    def own_handle():
        if a.own:
            seconds.append(second_build(a.own, "own_handle"))
            return None
        e1 = BatchMPC(horizon=N)                                    # (plain and wrench calls only)
        s1, args_1 = staged(e1)
        e1.stage_ext_wrench()[0] = w
        fn_w, _, args_w = e1.bind_update_wrench()
        rows["a_own_handle"] = lambda: raw.srbdqp_update_f64(*args_1)
        rows["w_own_handle"] = lambda: fn_w(*args_w)
        return e1

    # the two handles that are compared, made last and side by side
    parent = None
    if a.parent and a.last == "this":
        parent = second_build(a.parent, "parent")
    eng1 = own_handle()
    if a.parent and a.last == "parent":
        parent = second_build(a.parent, "parent")

    # warm-up, and the results before any timing
    for r in rows.values():
        for _ in range(200):
            r()
    assert rows["a_update_f64"]() == 0 and int(st["status"][0]) == 1
    info["a_kernel"], info["a_iters"], info["launch_path_of_a"] = eng.kernel_name(), int(st["iters"][0]), eng.batch1_launch_path()
    u_plain = st["u"][0].copy()
    info["b_flat_iters"], info["max_du_b_flat_vs_a_N"] = int(s0["iters"][0]), float(np.abs(s0["u"][0] - u_plain).max())
    if parent:
        lib, hp, sp = parent
        assert rows["a_parent"]() == 0
        up = np.ctypeslib.as_array((C.c_double * (12 * N)).from_address(sp.u)).reshape(N, 12)
        info["a_parent_kernel"] = lib.srbdqp_kernel_name(hp).decode()
        info["a_parent_equals_a_bitwise"] = bool(np.array_equal(up, u_plain))
        assert rows["w_parent"]() == 0
        info["w_parent_kernel"] = lib.srbdqp_kernel_name(hp).decode()
        u_wp = up.copy()
        if eng1 is not None:
            assert rows["w_own_handle"]() == 0
            info["w_parent_equals_w_own_bitwise"] = bool(np.array_equal(u_wp, eng1.stage()["u"][0]))
    assert rows["b_update_normals_f64"]() == 0 and int(st["status"][0]) == 1
    info["b_kernel"], info["b_iters"] = eng.kernel_name(), int(st["iters"][0])
    u_b = st["u"][0].copy()
    u_c = mpcs["c_mpc_update_default_route"].update(ctl, ftl, None, x_current=x0c, contact_normals=nr)[0]
    u_d = mpcs["d_mpc_update_staged_normals"].update(ctl, ftl, None, x_current=x0c, contact_normals=nr)[0]
    info["c_kernel"], info["d_kernel"] = (mpcs[k]._engine.kernel_name() for k in mpcs)
    info["max_du_b_vs_c_N"] = float(np.abs(u_b[0] - u_c.reshape(-1)).max())
    info["max_du_d_vs_c_N"] = float(np.abs(u_d - u_c).max())
    info["normals_move_u0_by_N"] = float(np.abs(u_b[0] - u_plain[0]).max())
    assert info["max_du_b_vs_c_N"] < 2e-3 and info["max_du_d_vs_c_N"] < 2e-3 and info["max_du_b_flat_vs_a_N"] < 1e-6, info

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
    out = {"qp": f"N = {N}, full double support, one QP", "handle_made_last": a.last if a.parent else "this", "own_handle_on": a.own or "this build",
           "calls_per_row": blocks * per, **info, "rows": {n: pct(v) for n, v in ts.items()}}
    p50 = {n: out["rows"][n]["p50_us"] for n in rows}
    out["b_over_c"] = round(p50["b_update_normals_f64"] / p50["c_mpc_update_default_route"], 4)
    out["b_below_c"] = bool(p50["b_update_normals_f64"] < p50["c_mpc_update_default_route"])
    out["b_flat_over_a"] = round(p50["b_flat_normals"] / p50["a_update_f64"], 4)
    if parent:
        out["a_own_handle_minus_a_parent_us"] = round(p50["a_own_handle"] - p50["a_parent"], 2)
        out["w_own_handle_minus_w_parent_us"] = round(p50["w_own_handle"] - p50["w_parent"], 2)
    for lib, hp, sp in seconds + ([parent] if parent else []):
        lib.srbdqp_destroy(hp)
    for m in mpcs.values():
        m.close()
    eng.close(); eng0.close()
    if eng1 is not None:
        eng1.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
