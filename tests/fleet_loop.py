"""What the GPU tests of the fleet roll-outs share (test_gpu_fleet.py, test_gpu_terrain.py, test_gpu_observer.py, test_gpu_steer.py): the roll-out call against
the same steps driven through the public device calls, and two small helpers.  Not a test module."""
import numpy as np

import fleet_twin as ft
import observer_twin as ot

DT = 0.04


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _stamps(stamp0, steps):
    """stamp of every robot at every step, by the roll-out's own repeated rounded addition -> (steps + 1, B)."""
    out = [np.asarray(stamp0, np.float64).copy()]
    for _ in range(steps):
        out.append(out[-1] + DT)
    return np.array(out)


def _device_loop(eng, c, B, steps, mode="flat", defer=False, horizon=10, observer=None):
    """The roll-out call, and the same steps driven from here through the public device calls on the same engine -> two dicts of host arrays, and the
    engine's kernel_name() behind the call.  c: the crowd -- with c["command"] the steered calls, with c["v_ref"] the plain ones.
    mode: "flat", "defer" (= flat with defer), "terrain" (a map is set on the engine: the normals of the step set on it), "observer" (the wrench buffer set on
    the engine; observer: observer_settings()' keywords, c["w0"] the estimate to start from).  defer: the engine defers its tails, a flush behind every solve."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=dev)
    Nh = horizon
    defer = defer or mode == "defer"
    obs, steered = mode == "observer", "command" in c
    alive0 = np.ones(B, np.uint8)
    if B > 4:
        alive0[3] = 0
    w0 = c["w0"] if obs else np.zeros((B, 6))
    out = []
    for call in (True, False):
        x, feet, stamp, sd, pu, al, w = up(c["x"]), up(c["feet"]), up(c["stamp"]), up(c["standing"]), up(c["push"]), up(alive0), up(w0)
        v = up(c["command"] if steered else c["v_ref"])
        if call:
            xl, ul, fl, wl = f64(steps + 1, B, 13), f64(steps, B, 12), f64(steps + 1, B, 12), f64(steps, B, 6)
            sl, il = torch.zeros((steps, B), dtype=torch.int32, device=dev), torch.zeros((steps, B), dtype=torch.int32, device=dev)
            eng.rollout_device(B, steps, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), 0 if steered else v.data_ptr(), ft.COM, standing=sd.data_ptr(),
                               push=pu.data_ptr(), alive=al.data_ptr(), x_log=xl.data_ptr(), u0_log=ul.data_ptr(), feet_log=fl.data_ptr(),
                               status_log=sl.data_ptr(), iters_log=il.data_ptr(), **(dict(command=v.data_ptr(), command_steps=1) if steered else {}),
                               **(dict(observer=observer, w_est=w.data_ptr(), w_log=wl.data_ptr()) if obs else {}))
            eng.synchronize()
            name = eng.kernel_name()
            logs = dict(x_log=xl, u0_log=ul, feet_log=fl, status_log=sl, iters_log=il)
            if obs:
                logs["w_log"] = wl
        else:
            xr, fo, pc, lp, ly, cn = f64(B, Nh, 13), f64(B, Nh, 12), f64(B, Nh, 3), f64(B, 3), f64(B), f64(B, Nh, 12)
            ct = torch.zeros((B, Nh, 4), dtype=torch.uint8, device=dev)
            u, xo = f64(B, Nh, 12), f64(B, Nh + 1, 13)
            st, it = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            xs, fs, us, ss, its, ws = [x.clone()], [feet.clone()], [], [], [], []
            yaw = dict(landing_yaw=ly.data_ptr()) if steered else {}
            if obs:
                ew = up(ot.horizon(w0, Nh, observer["horizon_decay"]))
                eng.set_external_wrench(ew)                                 # (the device setter: read in place at every solve)
            try:
                for k in range(steps):
                    (eng.mpc_inputs_steered_device if steered else eng.mpc_inputs_device)(
                        B, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), v.data_ptr(), ft.COM, xr.data_ptr(), fo.data_ptr(), ct.data_ptr(), pc.data_ptr(),
                        landing=lp.data_ptr(), standing=sd.data_ptr(), **yaw)
                    if mode == "terrain":
                        eng.terrain_inputs_device(B, feet.data_ptr(), xr.data_ptr(), cn.data_ptr())
                        eng.set_contact_normals(cn)                                   # (a CUDA tensor: srbdqp_set_contact_normals_device)
                    eng.solve_device(B, x.data_ptr(), xr.data_ptr(), fo.data_ptr(), ct.data_ptr(), u.data_ptr(), x_out=xo.data_ptr(), status=st.data_ptr(),
                                     iters=it.data_ptr(), pcom=pc.data_ptr())
                    if mode == "terrain":
                        assert eng.kernel_name() == f"wrench_f64_n{Nh}_cn"
                    if obs:
                        assert eng.kernel_name() == f"wrench_f64_n{Nh}_ew"
                    if defer:
                        eng.flush()
                    xp, fp = x.clone(), feet.clone()
                    eng.fleet_advance_device(B, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), u.data_ptr(), lp.data_ptr(), u0_stride=12 * Nh,
                                             standing=sd.data_ptr(), push=pu[k].data_ptr(), alive=al.data_ptr(), **yaw)
                    if obs:
                        eng.wrench_observer_device(B, xp.data_ptr(), x.data_ptr(), fp.data_ptr(), u.data_ptr(), w.data_ptr(), ew=ew.data_ptr(), u0_stride=12 * Nh,
                                                   alive=al.data_ptr(), **observer)
                    eng.synchronize()
                    xs.append(x.clone()); fs.append(feet.clone()); us.append(u[:, 0].clone()); ss.append(st.clone()); its.append(it.clone()); ws.append(w.clone())
            finally:
                eng.synchronize()
                if mode == "terrain":
                    eng.set_contact_normals(None)
                if obs:
                    eng.set_external_wrench(None)
            logs = dict(x_log=torch.stack(xs), u0_log=torch.stack(us), feet_log=torch.stack(fs), status_log=torch.stack(ss), iters_log=torch.stack(its))
            if obs:
                logs["w_log"] = torch.stack(ws)
        logs.update(x=x, feet=feet, stamp=stamp, alive=al)
        if obs:
            logs["w_est"] = w
        out.append({k: a.cpu().numpy() for k, a in logs.items()})
    return out[0], out[1], name
