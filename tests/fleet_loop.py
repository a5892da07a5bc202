"""What the GPU tests of the fleet roll-outs share (test_gpu_fleet.py, test_gpu_terrain.py, test_gpu_observer.py, test_gpu_steer.py, test_gpu_track.py,
test_gpu_preview.py, test_gpu_tile_loops.py; _bits alone: test_gpu_plant_reference.py): their crowds, the engine opener, the device-form inputs call, the
roll-out call against the same steps driven through the public device calls, the host form against the device form, and the roll-out's C entry points called
directly.  Not a test module.

The stream rule.  The engine's device forms with stream=0 run on the handle's own stream, which is created non-blocking: nothing orders it against torch's
current stream.  So
  - after any torch operation that writes or reads a tensor (an upload, torch.full, zeros, clone, stack), torch.cuda.synchronize() stands before an engine
    call that reads or writes that tensor;
  - after an engine call, eng.synchronize() stands before torch touches what it wrote.
The tests are about the engine's own stream: none of them hands torch's stream to a call instead."""
import ctypes as C

import numpy as np

import fleet_twin as ft
import observer_twin as ot
import terrain_twin as tt
import track_twin as ttw

DT = 0.04
OBS = dict(gain=0.5, horizon_decay=0.9, torque_max=50.0, force_max=200.0)      # the observer of the steered, tracked and previewed suites


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _stamps(stamp0, steps):
    """stamp of every robot at every step, by the roll-out's own repeated rounded addition -> (steps + 1, B)."""
    out = [np.asarray(stamp0, np.float64).copy()]
    for _ in range(steps):
        out.append(out[-1] + DT)
    return np.array(out)


def crowd(flavour, B, seed, steps=0, push="now and then", pose=False, P=6, on=None):
    """B robots around the nominal stance, drawn from default_rng(seed) in the fixed order of the flavour -> a dict of host arrays.
    "v_ref": random velocity references, a fifth standing, stamps anywhere in the gait period (rng.integers), pushes of up to 30 N / 3 N m now and then -- or,
    push="sustained", one push held from step 2 on, and w0, the estimates an observer starts from.  on: a terrain_twin map the robots stand on, placed over
    x in [-0.4, 1.6], y in [-0.5, 0.5].
    "commanded": any heading, commands of up to (0.3, 0.1) m/s and 1 rad/s, some of them zero, some turning on the spot, a few robots standing, stamps
    staggered over every phase of the gait, pushes now and then; pose: a pose each inside the default bounds, the last draw.
    "preview": the commanded crowd with velocities, footholds off the nominal ones, every eleventh robot standing, stamps staggered over a period of 2 P
    steps and some of them negative, a pose each, no pushes."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 13)); x[:, 12] = -9.80665
    if on is None:
        x[:, 3:6] = ft.COM + rng.normal(size=(B, 3)) * 0.005
        feet = np.tile(ft.FEET.reshape(12), (B, 1))
    else:
        at = np.stack([rng.uniform(-0.4, 1.6, B), rng.uniform(-0.5, 0.5, B)], -1)
        feet = np.tile(ft.FEET, (B, 1, 1))
        feet[:, :, 0:2] += at[:, None, :]
        feet[:, :, 2] = tt.sample(on, feet.reshape(-1, 3)[:, 0:2])[0].reshape(B, 4)
        feet = feet.reshape(B, 12)
        x[:, 3:5] = ft.COM[0:2] + at + rng.normal(size=(B, 2)) * 0.005
        x[:, 5] = tt.sample(on, x[:, 3:5])[0] + ft.COM[2] + rng.normal(size=B) * 0.005
    x[:, 0:2] = rng.normal(size=(B, 2)) * 0.02
    now_and_then = lambda: np.where(rng.random((steps, B, 1)) < 0.1, rng.uniform(-1.0, 1.0, (steps, B, 6)) * np.array([3.0, 3.0, 0.3, 30.0, 30.0, 30.0]), 0.0)
    if flavour == "v_ref":
        stamp = DT * rng.integers(0, 24, B).astype(np.float64)
        v_ref = np.where(rng.random((B, 1)) < 0.3, 0.0, rng.uniform(-0.2, 0.3, (B, 2)) * np.array([1.0, 0.4]))
        c = dict(x=x, feet=feet, stamp=stamp, v_ref=v_ref, standing=(rng.random(B) < 0.2).astype(np.uint8))
        if push == "sustained":
            c["push"] = np.zeros((steps, B, 6))
            c["push"][2:] = rng.uniform(-1.0, 1.0, (1, B, 6)) * np.array([1.0, 1.0, 0.1, 20.0, 20.0, 5.0])
            c["w0"] = rng.uniform(-1.0, 1.0, (B, 6)) * np.array([0.5, 0.5, 0.05, 5.0, 5.0, 2.0])
        else:
            c["push"] = now_and_then()
        return c
    preview = flavour == "preview"
    x[:, 2] = rng.uniform(-3.0, 3.0, B)
    if preview:
        x[:, 9:11] = rng.normal(size=(B, 2)) * 0.1
        feet = feet + rng.normal(size=(B, 12)) * 0.01
        stamp = DT * ((np.arange(B) * 5) % (2 * P)).astype(np.float64) - np.where(np.arange(B) % 3 == 0, 2 * P * DT * 4, 0.0)
    else:
        stamp = DT * ((np.arange(B) * 5) % 12).astype(np.float64)
    cmd = rng.uniform(-1.0, 1.0, (B, 3)) * np.array([0.3, 0.1, 1.0])
    kind = np.arange(B) % 7
    cmd[kind == 0] = 0.0
    cmd[kind == 1, 0:2] = 0.0
    cmd[kind == 2, 2] = 0.0
    c = dict(x=x, feet=feet, stamp=stamp, command=cmd)
    if preview:
        c["standing"] = (np.arange(B) % 11 == 4).astype(np.uint8)
    else:
        c["standing"] = (rng.random(B) < 0.15).astype(np.uint8)
        c["push"] = now_and_then()
    if pose or preview:
        c["pose"] = ttw.start_pose(x) + rng.uniform(-1.0, 1.0, (B, 3)) * np.array([0.05, 0.05, 0.25])
    return c


def turned_feet(c):
    """The crowd's feet under its robots: the nominal stance turned to every robot's heading about its CoM (so that a roll-out starts from a stance it can hold)."""
    B = c["x"].shape[0]
    rel = (ft.FEET - np.array([ft.COM[0], ft.COM[1], 0.0]))[None, :, :]
    s, co_ = np.sin(c["x"][:, 2])[:, None], np.cos(c["x"][:, 2])[:, None]
    f = np.zeros((B, 4, 3))
    f[:, :, 0] = c["x"][:, None, 3] + co_ * rel[:, :, 0] - s * rel[:, :, 1]
    f[:, :, 1] = c["x"][:, None, 4] + s * rel[:, :, 0] + co_ * rel[:, :, 1]
    return f.reshape(B, 12)


def engine(horizon, flags=0):
    """A BatchMPC of that horizon: a horizon the general kernel has no instantiation for opens it with SRBDQP_FLAG_ANY_HORIZON."""
    from g1_locomotion_amd import BatchMPC, _lib
    flags |= 0 if horizon in (4, 8, 10, 12, 16, 20, 24) else _lib.FLAG_ANY_HORIZON
    return BatchMPC(horizon=horizon, **(dict(flags=flags) if flags else {}))


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _filled(value, dtype, *shape):
    import torch
    return torch.full(shape, value, dtype=getattr(torch, dtype), device=torch.device("cuda", 0))


def _f64(*shape):
    return _filled(-7.0, "float64", *shape)


def _p(a):
    return 0 if a is None else a.data_ptr()


def _mpc_inputs(e, flavour, B, x, feet, stamp, v, sd, pose, xr, fo, ct, pc, lp, ly, pv=None, **kw):
    """The device-form inputs call of a flavour -- "plain" (v: the velocity references), "steered" or "tracked" (v: the commands) -- on torch tensors; with pv,
    the previewed bytes, the previewed call, steered or tracked."""
    head, outs = (B, _p(x), _p(feet), _p(stamp), _p(v)), (ft.COM, _p(xr), _p(fo), _p(ct), _p(pc))
    kw = dict(landing=_p(lp), standing=_p(sd), **kw)
    if flavour == "plain":
        e.mpc_inputs_device(*head, *outs, **kw)
    elif pv is not None:
        e.mpc_inputs_previewed_device(*head, *outs, landing_yaw=_p(ly), pose=_p(pose) if flavour == "tracked" else 0, previewed=_p(pv), **kw)
    elif flavour == "tracked":
        e.mpc_inputs_tracked_device(*head, _p(pose), *outs, landing_yaw=_p(ly), **kw)
    else:
        e.mpc_inputs_steered_device(*head, *outs, landing_yaw=_p(ly), **kw)


def inputs_device(e, c, horizon, flavour, preview=False, **kw):
    """mpc_inputs_device ("plain"), mpc_inputs_steered_device ("steered") or mpc_inputs_tracked_device ("tracked") -- with preview, mpc_inputs_previewed_device
    in its steered or tracked form -- on device copies of the crowd, into outputs prefilled with -7.0 (doubles) and 9 (bytes) -> a dict of host arrays, with
    the pose behind the call when tracked and previewed when previewed.  kw: the call's gait and track settings.  The device forms take what the host forms
    refuse: poses and commands that are not finite."""
    import torch
    B = c["x"].shape[0]
    x, feet, stamp, sd, v = _up(c["x"]), _up(c["feet"]), _up(c["stamp"]), _up(c["standing"]), _up(c["v_ref" if flavour == "plain" else "command"])
    pose = _up(c["pose"]) if flavour == "tracked" else None
    out = dict(x_ref=_f64(B, horizon, 13), foot=_f64(B, horizon, 12), contact=_filled(9, "uint8", B, horizon, 4), pcom=_f64(B, horizon, 3), landing=_f64(B, 3))
    ly = None if flavour == "plain" else _f64(B)
    pv = _filled(9, "uint8", B, horizon, 4) if preview else None
    torch.cuda.synchronize()                                      # (the uploads and fills above run on torch's stream, the call on the engine's own)
    _mpc_inputs(e, flavour, B, x, feet, stamp, v, sd, pose, out["x_ref"], out["foot"], out["contact"], out["pcom"], out["landing"], ly, pv, **kw)
    e.synchronize()
    out.update({k: a for k, a in dict(landing_yaw=ly, previewed=pv, pose=pose).items() if a is not None})
    return {k: a.cpu().numpy() for k, a in out.items()}


def device_loop(eng, c, B, steps, mode="flat", defer=False, horizon=10, observer=None, track=None, preview=False, dead=True, call=True):
    """The roll-out call, and the same steps driven from here through the public device calls on the same engine -- the inputs call -> (the terrain inputs +
    the normals set on the engine) -> solve_device -> (flush) -> fleet_advance_device -> (wrench_observer_device) -- -> two dicts of host arrays under the same
    keys (x_log, u0_log, feet_log, status_log, iters_log[, w_log, pose_log] and the final x, feet, stamp, alive[, w_est, pose]), and the engine's kernel_name()
    behind the call.  c: the crowd -- with c["command"] the steered calls, with c["v_ref"] the plain ones; c["push"] where there are pushes.
    mode: "flat", "defer" (= flat with defer), "terrain" (a map is set on the engine: the normals of the step set on it), "observer" (the wrench buffer set on
    the engine; observer: observer_settings()' keywords, c["w0"] the estimate to start from).  defer: the engine defers its tails, a flush behind every solve.
    track: True or track_settings()' keywords -- the tracked calls, from c["pose"].  preview: the previewed calls, steered or tracked.  dead: robot 3 of a
    crowd of more than 4 is handed in dead.  call=False: the steps from here alone (None for the call's dict and for the name)."""
    import torch
    Nh = horizon
    defer = defer or mode == "defer"
    obs, terrain = mode == "observer", mode == "terrain"
    flavour = "tracked" if track is not None else "steered" if "command" in c else "plain"
    steered, tracked = flavour != "plain", flavour == "tracked"
    alive0 = np.ones(B, np.uint8)
    if dead and B > 4:
        alive0[3] = 0
    w0 = c["w0"] if obs else np.zeros((B, 6))
    out, name = {}, None
    for whole in ((True, False) if call else (False,)):
        x, feet, stamp, sd, al, w = _up(c["x"]), _up(c["feet"]), _up(c["stamp"]), _up(c["standing"]), _up(alive0), _up(w0)
        v, pu, pose = _up(c["command"] if steered else c["v_ref"]), _up(c["push"]) if "push" in c else None, _up(c["pose"]) if tracked else None
        if whole:
            xl, ul, fl, wl, pl = _f64(steps + 1, B, 13), _f64(steps, B, 12), _f64(steps + 1, B, 12), _f64(steps, B, 6), _f64(steps, B, 3)
            sl, il = _filled(0, "int32", steps, B), _filled(0, "int32", steps, B)
            torch.cuda.synchronize()
            eng.rollout_device(B, steps, _p(x), _p(feet), _p(stamp), 0 if steered else _p(v), ft.COM, standing=_p(sd), push=_p(pu), alive=_p(al), x_log=_p(xl),
                               u0_log=_p(ul), feet_log=_p(fl), status_log=_p(sl), iters_log=_p(il), **(dict(command=_p(v), command_steps=1) if steered else {}),
                               **(dict(track=track, pose=_p(pose), pose_log=_p(pl)) if tracked else {}), **(dict(preview=True) if preview else {}),
                               **(dict(observer=observer, w_est=_p(w), w_log=_p(wl)) if obs else {}))
            eng.synchronize()
            name = eng.kernel_name()
            logs = dict(x_log=xl, u0_log=ul, feet_log=fl, status_log=sl, iters_log=il)
            if obs:
                logs["w_log"] = wl
            if tracked:
                logs["pose_log"] = pl
        else:
            xr, fo, pc, lp, ly, cn = _f64(B, Nh, 13), _f64(B, Nh, 12), _f64(B, Nh, 3), _f64(B, 3), _f64(B), _f64(B, Nh, 12)
            ct, pv = _filled(0, "uint8", B, Nh, 4), _filled(0, "uint8", B, Nh, 4) if preview else None
            u, xo = _f64(B, Nh, 12), _f64(B, Nh + 1, 13)
            st, it = _filled(0, "int32", B), _filled(0, "int32", B)
            xs, fs, us, ss, its, ws, ps = [x.clone()], [feet.clone()], [], [], [], [], []
            yaw = dict(landing_yaw=_p(ly)) if steered else {}
            if obs:
                ew = _up(ot.horizon(w0, Nh, observer["horizon_decay"]))
                eng.set_external_wrench(ew)                                 # (the device setter: read in place at every solve)
            try:
                for k in range(steps):
                    torch.cuda.synchronize()                                # (the uploads, the fills and the clones behind the step before)
                    _mpc_inputs(eng, flavour, B, x, feet, stamp, v, sd, pose, xr, fo, ct, pc, lp, ly, pv, **({} if track in (None, True) else track))
                    if tracked and not preview:
                        assert eng.kernel_name() == "mpc_inputs_tracked_f64"
                    if terrain:
                        if preview:
                            eng.terrain_inputs_previewed_device(B, _p(fo), _p(pv), _p(xr), _p(cn))
                        else:
                            eng.terrain_inputs_device(B, _p(feet), _p(xr), _p(cn))
                        eng.set_contact_normals(cn)                                   # (a CUDA tensor: srbdqp_set_contact_normals_device)
                    eng.solve_device(B, _p(x), _p(xr), _p(fo), _p(ct), _p(u), x_out=_p(xo), status=_p(st), iters=_p(it), pcom=_p(pc))
                    if terrain:
                        assert eng.kernel_name() == f"wrench_f64_n{Nh}_cn"
                    if obs:
                        assert eng.kernel_name() == f"wrench_f64_n{Nh}_ew"
                    if defer:
                        eng.flush()
                    xp, fp = x.clone(), feet.clone()                        # (what no engine call above writes)
                    torch.cuda.synchronize()                                # (... and the step below does)
                    eng.fleet_advance_device(B, _p(x), _p(feet), _p(stamp), _p(u), _p(lp), u0_stride=12 * Nh, standing=_p(sd),
                                             push=_p(None if pu is None else pu[k]), alive=_p(al), **yaw)
                    if obs:
                        eng.wrench_observer_device(B, _p(xp), _p(x), _p(fp), _p(u), _p(w), ew=_p(ew), u0_stride=12 * Nh, alive=_p(al), **observer)
                    eng.synchronize()
                    xs.append(x.clone()); fs.append(feet.clone()); us.append(u[:, 0].clone()); ss.append(st.clone()); its.append(it.clone()); ws.append(w.clone())
                    if tracked:
                        ps.append(pose.clone())
            finally:
                eng.synchronize()
                if terrain:
                    eng.set_contact_normals(None)
                if obs:
                    eng.set_external_wrench(None)
            logs = dict(x_log=torch.stack(xs), u0_log=torch.stack(us), feet_log=torch.stack(fs), status_log=torch.stack(ss), iters_log=torch.stack(its))
            if obs:
                logs["w_log"] = torch.stack(ws)
            if tracked:
                logs["pose_log"] = torch.stack(ps)
        logs.update(x=x, feet=feet, stamp=stamp, alive=al)
        if obs:
            logs["w_est"] = w
        if tracked:
            logs["pose"] = pose
        out[whole] = {k: a.cpu().numpy() for k, a in logs.items()}
    return out.get(True), out[False], name


def rollout_device_against_host(e, c, T, v_ref=None, observer=None, w0=None, track=None):
    """rollout() on host arrays against rollout_device() on device copies of the same inputs, robot 3 handed in dead, into logs prefilled with 7: every log
    and every final array bit for bit -> the host form's result.  v_ref: the (B,2) references of the plain call; None: the steered call on c["command"].
    observer: observer_settings()' keywords, with w0 the estimates to start from.  track: track_settings()' keywords, from c["pose"]."""
    import torch
    B = c["x"].shape[0]
    steered, observed, tracked = v_ref is None, observer is not None, track is not None
    alive0 = np.ones(B, np.uint8)
    alive0[3] = 0
    host = e.rollout(c["x"], c["feet"], c["stamp"], v_ref, T, ft.COM, standing=c["standing"], push=c["push"], alive=alive0,
                     command=c["command"] if steered else None, **(dict(track=track, pose=c["pose"]) if tracked else {}),
                     **(dict(observer=observer, w_est=w0) if observed else {}))
    dev = {k: _up(a) for k, a in dict(x=c["x"], feet=c["feet"], stamp=c["stamp"], standing=c["standing"], push=c["push"], alive=alive0,
                                      vel=c["command"] if steered else v_ref, **(dict(w_est=w0) if observed else {}),
                                      **(dict(pose=c["pose"]) if tracked else {})).items()}
    logs = {k: _up(np.full_like(host[k], 7)) for k in ("x", "u0", "feet", "status", "iters") + (("w_log",) if observed else ()) + (("pose_log",) if tracked else ())}
    ptr = lambda k: logs[k].data_ptr()
    torch.cuda.synchronize()                                      # (the uploads run on torch's stream, the call on the engine's own)
    e.rollout_device(B, T, _p(dev["x"]), _p(dev["feet"]), _p(dev["stamp"]), 0 if steered else _p(dev["vel"]), ft.COM, standing=_p(dev["standing"]),
                     push=_p(dev["push"]), alive=_p(dev["alive"]), x_log=ptr("x"), u0_log=ptr("u0"), feet_log=ptr("feet"), status_log=ptr("status"),
                     iters_log=ptr("iters"), **(dict(command=_p(dev["vel"]), command_steps=1) if steered else {}),
                     **(dict(track=track, pose=_p(dev["pose"]), pose_log=ptr("pose_log")) if tracked else {}),
                     **(dict(observer=observer, w_est=_p(dev["w_est"]), w_log=ptr("w_log")) if observed else {}))
    e.synchronize()
    for k, a in logs.items():
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(host[k])), k
    finals = dict(x=host["x"][-1], feet=host["feet"][-1], stamp=host["stamp"], alive=host["alive"], **(dict(w_est=host["w_est"]) if observed else {}),
                  **(dict(pose=host["pose"]) if tracked else {}))
    for k, a in finals.items():
        assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(a)), k
    return host


def direct_rollout(e, entry, c, steps, vel):
    """The C roll-out `entry` -- "srbdqp_fleet_rollout_f64" (vel: the (B,2) references), "srbdqp_fleet_rollout_steered_f64" or "srbdqp_fleet_rollout_tracked_f64"
    (vel: the (B,3) commands, held over the call; tracked: from c["pose"] under the default track settings) -- called through ctypes on copies of the crowd's
    arrays, every robot alive, under fleet_settings(COM), with c["push"] where there is one -> its logs x, u0, feet, status, iters and the final alive, stamp."""
    B = c["x"].shape[0]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    x, feet, stamp, al = c["x"].copy(), c["feet"].copy(), c["stamp"].copy(), np.ones(B, np.uint8)
    xl, ul, fl = np.empty((steps + 1, B, 13)), np.empty((steps, B, 12)), np.empty((steps + 1, B, 12))
    sl, il = np.empty((steps, B), np.int32), np.empty((steps, B), np.int32)
    s = e.fleet_settings(ft.COM)
    commanded = entry != "srbdqp_fleet_rollout_f64"
    args = [e._h, B, steps, p(x), p(feet), p(stamp), p(vel)] + ([1] if commanded else []) + [p(c["standing"]), p(c.get("push")), C.byref(s), p(al), p(xl), p(ul),
                                                                                              p(fl), p(sl), p(il)] + ([None, None, None] if commanded else [])
    if entry == "srbdqp_fleet_rollout_tracked_f64":
        k, pose, pl = e.track_settings(), c["pose"].copy(), np.empty((steps, B, 3))
        args += [C.byref(k), p(pose), p(pl)]
    assert getattr(e._lib, entry)(*args) == 0
    return dict(x=xl, u0=ul, feet=fl, status=sl, iters=il, alive=al, stamp=stamp)
