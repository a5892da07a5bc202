"""What a side input of the call -- an external wrench, contact normals on sloped ground -- costs the single robot's control loop, per call, on the GPU box; and
whether the calls that existed have moved.

  python tools/staged_side_latency.py --kind wrench|normals [--calls 10000] [--parent PATH/libsrbdqp.so] [--own PATH/other_copy.so] [--last parent|this] [--out FILE]

One QP at N = 10, full double support (the reference's own contact pattern), with a drawn wrench, or with drawn contact normals (one per foot and step, tilt up to
0.35 rad).  p50 / p99 of the host's wall clock around one call -- every call returns with its results in host memory -- for
  (a) srbdqp_update_f64: no wrench, flat ground;
  (b) srbdqp_update_wrench_f64 / srbdqp_update_normals_f64 with the drawn input, and (b_zero_wrench / b_flat_normals) with an all-zero block / (0, 0, 1)
      everywhere -- (a)'s QP bit for bit / to rounding: the price of the form;
  (c) MPC.update(external_wrench= / contact_normals=) on the default route: the host setter, a host-buffer batch solve of B = 1, the setter again;
  (d) MPC(staged_wrench=True / staged_normals=True).update(...);
and, for the calls that existed, on two handles MADE LAST, side by side: one of this build ("own handle") and one of another build of the library (--parent:
the parent commit's), in the same process.  THE ORDER IN WHICH HANDLES ARE MADE COUNTS: the handle a process made last answers 1.2 - 1.3 us sooner than any
earlier one, whichever build it is on (measured with a copy of one build under two names).  So --last says which of the two is made last, and a comparison of two
builds is two runs, one per order: like against like is *_own_handle of --last this against *_parent of --last parent (both last), and the other two (both second
to last).  --own PATH puts the "own" handle on a second build too (a COPY of the parent's library under another name): the same two runs then show what the
comparison reads when nothing differs -- the margin.  The rows on those two handles:
  --kind wrench   (a_own_handle, a_parent_update_f64): srbdqp_update_f64 alone -- handles that never make a wrench call;
  --kind normals  (a_own_handle, w_own_handle, n_own_handle; a_parent, w_parent, n_parent): srbdqp_update_f64, srbdqp_update_wrench_f64 and
                  srbdqp_update_normals_f64 (the n_ rows where the other build has that call; profiles/r21_staged_normals_latency.json predates them: its
                  handles never made a normals call).
`calls` calls per row in all, in ten blocks per row, the rows interleaved block by block and their order rotated from block to block (what the box does
meanwhile, and what ran just before, meet every row alike); 200 warm-up calls per row first.  The results of (b) and (d) are held against (c)'s -- the setter's
route -- before the timing starts.  Prints one JSON object; --out also writes it to a file.  The rows and keys of a kind are those of
profiles/r20_staged_wrench_latency.json / profiles/r21_staged_normals_latency.json."""
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

# per kind: MPC's keyword and flag, BatchMPC's two methods, the row names, and the calls the two compared handles make (plain, wrench, normals)
KINDS = {
    "wrench": dict(keyword="external_wrench", flag="staged_wrench", stage="stage_ext_wrench", bind="bind_update_wrench", b_row="b_update_wrench_f64",
                   neutral_row="b_zero_wrench", parent_row="a_parent_update_f64", compared="a"),
    "normals": dict(keyword="contact_normals", flag="staged_normals", stage="stage_contact_normals", bind="bind_update_normals", b_row="b_update_normals_f64",
                    neutral_row="b_flat_normals", parent_row="a_parent", compared="awn"),
}


def pct(ts):
    ts = np.asarray(ts) * 1e6
    return {"p50_us": round(float(np.percentile(ts, 50)), 2), "p99_us": round(float(np.percentile(ts, 99)), 2), "min_us": round(float(ts.min()), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=tuple(KINDS), required=True)
    ap.add_argument("--calls", type=int, default=10000)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--own", default=None)
    ap.add_argument("--last", choices=("parent", "this"), default="parent")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    k = dict(KINDS[a.kind])
    k["d_row"] = "d_mpc_update_" + k["flag"]                       # (d)'s row is named after MPC's flag
    wrench = a.kind == "wrench"
    import torch  # noqa: F401  (one HIP runtime for the process)
    import srbd_oracle as orc
    from g1_locomotion_amd import BatchMPC, MPC, _lib
    x0, xr, ft, ct = orc.synthetic_batch(1, N, seed=99, schedule="double")
    rng = np.random.default_rng(7)
    if not wrench:                                                  # (each kind's draws in the order its earlier runs made them)
        tilt, az = rng.uniform(0.0, 0.35, (N, 2)), rng.uniform(-np.pi, np.pi, (N, 2))
        nr = np.repeat(np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], -1), 2, axis=1).reshape(N, 12)   # (heel and toe of a foot share its normal)
    w = np.concatenate([rng.uniform(-4, 4, (1, 3)) + rng.uniform(-1, 1, (N, 3)), rng.uniform(-40, 40, (1, 3)) + rng.uniform(-10, 10, (N, 3))], axis=1)
    side = w if wrench else nr
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
    getattr(eng, k["stage"])()[0] = side
    fn_b, _, args_b = getattr(eng, k["bind"])()
    rows["a_update_f64"] = lambda: raw.srbdqp_update_f64(*args_a)
    rows[k["b_row"]] = lambda: fn_b(*args_b)
    eng0 = BatchMPC(horizon=N)                                      # (the neutral row: a handle of its own -- its staged side array stays zero / (0, 0, 1))
    s0, _ = staged(eng0)
    fn_0, _, args_0 = getattr(eng0, k["bind"])()
    rows[k["neutral_row"]] = lambda: fn_0(*args_0)

    # (c), (d): the Python object on its two routes
    mpcs = {"c_mpc_update_default_route": MPC(horizon=N), k["d_row"]: MPC(horizon=N, **{k["flag"]: True})}
    for m in mpcs.values():
        m.init_matrices()
        m.x_ref_hor[:] = xr[0]
    for name, m in mpcs.items():
        rows[name] = (lambda m: lambda: m.update(ctl, ftl, None, x_current=x0c, **{k["keyword"]: side}))(m)

    def second_build(path, tag, plain_row):
        """Another build of the library beside this tree's, a handle on it with the QP (and, where the kind's compared handles make those calls, a wrench and
        the normals) staged; its calls as rows plain_row, w_<tag>, n_<tag> -> (library, handle, its staging arrays)."""
        lib = C.CDLL(os.path.abspath(path))
        calls = {"w": ("srbdqp_stage_ext_wrench", "srbdqp_update_wrench_f64", w), "n": ("srbdqp_stage_contact_normals", "srbdqp_update_normals_f64", None if wrench else nr)}
        calls = {c: v for c, v in calls.items() if c in k["compared"] and hasattr(lib, v[1])}
        for name in ("srbdqp_create", "srbdqp_destroy", "srbdqp_stage_ptrs", "srbdqp_update_f64", "srbdqp_kernel_name") + tuple(n for v in calls.values() for n in v[:2]):
            getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        cfg = _lib.default_config()
        cfg.horizon = N
        hp = C.c_void_p()
        assert lib.srbdqp_create(C.byref(cfg), C.byref(hp)) == _lib.OK
        sp = _lib.Stage()
        assert lib.srbdqp_stage_ptrs(hp, C.byref(sp)) == _lib.OK
        vp = lambda p: C.c_void_p(p)
        ins = (hp, vp(sp.x0), vp(sp.x_ref), vp(sp.foot), vp(sp.contact), None)
        outs = (vp(sp.u), None, vp(sp.x), None, None)
        fill = [(sp.x0, x0[0]), (sp.x_ref, xr[0]), (sp.foot, ft[0])]
        rows[plain_row] = lambda: lib.srbdqp_update_f64(*ins, *outs)
        for c, (stage, update, v) in calls.items():
            at = C.c_void_p()
            assert getattr(lib, stage)(hp, C.byref(at)) == _lib.OK
            fill.append((at.value, v))
            rows[c + "_" + tag] = (lambda fn, at: lambda: fn(*ins, at, *outs))(getattr(lib, update), at)
        for addr, v in fill:
            C.memmove(addr, np.ascontiguousarray(v, np.float64).ctypes.data, v.size * 8)
        C.memmove(sp.contact, np.ascontiguousarray(ct[0] != 0, np.uint8).ctypes.data, 4 * N)
        return lib, hp, sp

    seconds = []

    def own_handle():
        if a.own:
            seconds.append(second_build(a.own, "own_handle", "a_own_handle"))
            return None
        e1 = BatchMPC(horizon=N)                                    # (the calls of k["compared"] only)
        s1, args_1 = staged(e1)
        rows["a_own_handle"] = lambda: raw.srbdqp_update_f64(*args_1)
        for c, stage, bind, v in (("w", "stage_ext_wrench", "bind_update_wrench", w), ("n", "stage_contact_normals", "bind_update_normals", None if wrench else nr)):
            if c in k["compared"]:
                getattr(e1, stage)()[0] = v
                fn, _, args = getattr(e1, bind)()
                rows[c + "_own_handle"] = (lambda fn, args: lambda: fn(*args))(fn, args)
        return e1

    # the two handles that are compared, made last and side by side
    parent = None
    if a.parent and a.last == "this":
        parent = second_build(a.parent, "parent", k["parent_row"])
    eng1 = own_handle()
    if a.parent and a.last == "parent":
        parent = second_build(a.parent, "parent", k["parent_row"])

    # warm-up, and the results before any timing
    for r in rows.values():
        for _ in range(200):
            r()
    assert rows["a_update_f64"]() == 0 and int(st["status"][0]) == 1
    info["a_kernel"], info["a_iters"], info["launch_path_of_a"] = eng.kernel_name(), int(st["iters"][0]), eng.batch1_launch_path()
    u_plain = st["u"][0].copy()
    if wrench:
        info["b_zero_equals_a_bitwise"], info["b_zero_iters"] = bool(np.array_equal(s0["u"][0], u_plain) and np.array_equal(s0["x"][0], st["x"][0])), int(s0["iters"][0])
    else:
        info["b_flat_iters"], info["max_du_b_flat_vs_a_N"] = int(s0["iters"][0]), float(np.abs(s0["u"][0] - u_plain).max())
    if parent:
        lib, hp, sp = parent
        assert rows[k["parent_row"]]() == 0
        up = np.ctypeslib.as_array((C.c_double * (12 * N)).from_address(sp.u)).reshape(N, 12)
        info["a_parent_kernel"] = lib.srbdqp_kernel_name(hp).decode()
        info["a_parent_equals_a_bitwise"] = bool(np.array_equal(up, u_plain))
        for c in "wn":
            if c + "_parent" in rows:
                assert rows[c + "_parent"]() == 0
                info[c + "_parent_kernel"] = lib.srbdqp_kernel_name(hp).decode()
                u_p = up.copy()
                if eng1 is not None:
                    assert rows[c + "_own_handle"]() == 0
                    info[f"{c}_parent_equals_{c}_own_bitwise"] = bool(np.array_equal(u_p, eng1.stage()["u"][0]))
    assert rows[k["b_row"]]() == 0 and int(st["status"][0]) == 1
    info["b_kernel"], info["b_iters"] = eng.kernel_name(), int(st["iters"][0])
    u_b = st["u"][0].copy()
    u_c = mpcs["c_mpc_update_default_route"].update(ctl, ftl, None, x_current=x0c, **{k["keyword"]: side})[0]
    u_d = mpcs[k["d_row"]].update(ctl, ftl, None, x_current=x0c, **{k["keyword"]: side})[0]
    info["c_kernel"], info["d_kernel"] = (mpcs[n]._engine.kernel_name() for n in mpcs)
    info["max_du_b_vs_c_N"] = float(np.abs(u_b[0] - u_c.reshape(-1)).max())
    info["max_du_d_vs_c_N"] = float(np.abs(u_d - u_c).max())
    info["wrench_moves_u0_by_N" if wrench else "normals_move_u0_by_N"] = moved = float(np.abs(u_b[0] - u_plain[0]).max())
    assert info["max_du_b_vs_c_N"] < 2e-3 and info["max_du_d_vs_c_N"] < 2e-3, info
    assert (moved > 1.0) if wrench else (info["max_du_b_flat_vs_a_N"] < 1e-6), info

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
    out = {"kind": a.kind, "qp": f"N = {N}, full double support, one QP", "handle_made_last": a.last if a.parent else "this", "own_handle_on": a.own or "this build",
           "calls_per_row": blocks * per, **info, "rows": {n: pct(v) for n, v in ts.items()}}
    p50 = {n: out["rows"][n]["p50_us"] for n in rows}
    out["b_over_a"] = round(p50[k["b_row"]] / p50["a_update_f64"], 4)
    out["b_over_c"] = round(p50[k["b_row"]] / p50["c_mpc_update_default_route"], 4)
    out["b_below_c"] = bool(p50[k["b_row"]] < p50["c_mpc_update_default_route"])
    if not wrench:
        out["b_flat_over_a"] = round(p50[k["neutral_row"]] / p50["a_update_f64"], 4)
    if parent:
        if wrench:
            out["a_minus_a_parent_us"] = round(p50["a_update_f64"] - p50[k["parent_row"]], 2)
        out["a_own_handle_minus_a_parent_us"] = round(p50["a_own_handle"] - p50[k["parent_row"]], 2)
        for c in "wn":
            if c + "_parent" in rows and c + "_own_handle" in rows:
                out[f"{c}_own_handle_minus_{c}_parent_us"] = round(p50[c + "_own_handle"] - p50[c + "_parent"], 2)
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
