"""GPU tests of the tracked fleet calls (include/srbdqp_cascade.h srbdqp_mpc_inputs_tracked_*, srbdqp_fleet_rollout_tracked_*) against
the NumPy twin of tests/track_twin.py (tests/test_track_cpu.py holds the twin itself).

Bounds: those of test_gpu_steer.py.  What passes through no sine or cosine is compared bit for bit -- the bounded pose, the heading references, the heading
behind the step among it.  What does: 1e-12 absolute -- the device's sin / cos against NumPy's at arguments below 10, on values of order 1, through at most 24
sums.  Free-running trajectories: 1e-4 at 50 steps, with every iteration count equal to the twin's."""
import ctypes as C
import time

import numpy as np
import pytest

import c_oracle  # noqa: F401
import srbd_oracle as orc
import fleet_twin as ft
from fleet_loop import _bits
import observer_twin as ot
import steer_twin as stw
import terrain_twin as tt
import track_twin as ttw

pytestmark = pytest.mark.gpu
N, DT, B77 = 10, 0.04, 77
EXACT_COLS = [0, 1, 2, 5, 6, 7, 8, 11, 12]
TRIG_COLS = [3, 4, 9, 10]
OBS = dict(gain=0.5, horizon_decay=0.9, torque_max=50.0, force_max=200.0)
# the robots of the 77-robot crowd that are not plainly inside the bounds
FAR, YAW_HI, YAW_LO, BOTH, NAN_X, NAN_YAW, NAN_POSE, NAN_TH, NAN_CMD, INF_CMD = (5, 37, 70), (11, 44), (12, 45), (20, 66), 9, 33, 40, 41, 50, 76
ODD = FAR + YAW_HI + YAW_LO + BOTH + (NAN_X, NAN_YAW, NAN_POSE, NAN_TH, NAN_CMD, INF_CMD)


def _crowd(B, seed, steps=0):
    """test_gpu_steer.py's crowd -- robots around the nominal stance at any heading, commands of up to (0.3, 0.1) m/s and 1 rad/s, some of them zero, some
    turning on the spot, a few standing, stamps over every phase of the gait, pushes now and then -- with a pose each, inside the default bounds."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 13)); x[:, 3:6] = ft.COM + rng.normal(size=(B, 3)) * 0.005; x[:, 0:2] = rng.normal(size=(B, 2)) * 0.02; x[:, 12] = -9.80665
    x[:, 2] = rng.uniform(-3.0, 3.0, B)
    feet = np.tile(ft.FEET.reshape(12), (B, 1))
    stamp = DT * ((np.arange(B) * 5) % 12).astype(np.float64)
    cmd = rng.uniform(-1.0, 1.0, (B, 3)) * np.array([0.3, 0.1, 1.0])
    kind = np.arange(B) % 7
    cmd[kind == 0] = 0.0
    cmd[kind == 1, 0:2] = 0.0
    cmd[kind == 2, 2] = 0.0
    standing = (rng.random(B) < 0.15).astype(np.uint8)
    push = np.where(rng.random((steps, B, 1)) < 0.1, rng.uniform(-1.0, 1.0, (steps, B, 6)) * np.array([3.0, 3.0, 0.3, 30.0, 30.0, 30.0]), 0.0)
    pose = ttw.start_pose(x) + rng.uniform(-1.0, 1.0, (B, 3)) * np.array([0.05, 0.05, 0.25])
    return dict(x=x, feet=feet, stamp=stamp, command=cmd, standing=standing, push=push, pose=pose)


def _odd(c):
    """The 77-robot crowd with its odd robots: beyond the position bound, beyond the yaw bound on either side, beyond both, a state, a pose and a command that
    are not finite.  (FAR[0] and BOTH[0] carry a zero command: their references show the clamped pose itself.)"""
    c = {k: v.copy() for k, v in c.items()}
    rng = np.random.default_rng(5)
    for b in FAR + BOTH:
        a = rng.uniform(-np.pi, np.pi)
        c["pose"][b, 0:2] = c["x"][b, 3:5] + rng.uniform(0.15, 2.0) * np.array([np.cos(a), np.sin(a)])
    for b, s in [(b, 1.0) for b in YAW_HI + BOTH[:1]] + [(b, -1.0) for b in YAW_LO + BOTH[1:]]:
        c["pose"][b, 2] = c["x"][b, 2] + s * rng.uniform(0.35, 4.0)
    c["command"][FAR[0]] = 0.0; c["command"][BOTH[0]] = 0.0
    c["x"][NAN_X, 4] = np.nan; c["x"][NAN_YAW, 2] = np.nan
    c["pose"][NAN_POSE, 0] = np.nan; c["pose"][NAN_TH, 2] = np.nan
    c["command"][NAN_CMD, 2] = np.nan; c["command"][INF_CMD, 0] = np.inf
    return c


def _turned_feet(c):
    """The crowd's feet under its robots: the nominal stance turned to every robot's heading about its CoM (so that a roll-out starts from a stance it can hold)."""
    B = c["x"].shape[0]
    rel = (ft.FEET - np.array([ft.COM[0], ft.COM[1], 0.0]))[None, :, :]
    s, co_ = np.sin(c["x"][:, 2])[:, None], np.cos(c["x"][:, 2])[:, None]
    f = np.zeros((B, 4, 3))
    f[:, :, 0] = c["x"][:, None, 3] + co_ * rel[:, :, 0] - s * rel[:, :, 1]
    f[:, :, 1] = c["x"][:, None, 4] + s * rel[:, :, 0] + co_ * rel[:, :, 1]
    return f.reshape(B, 12)


def _engine(horizon, flags=0):
    from g1_locomotion_amd import BatchMPC, _lib
    flags |= 0 if horizon in (4, 8, 10, 12, 16, 20, 24) else _lib.FLAG_ANY_HORIZON
    return BatchMPC(horizon=horizon, **(dict(flags=flags) if flags else {}))


def _inputs_device(e, c, horizon, steered=False, **track):
    """mpc_inputs_tracked_device (steered: mpc_inputs_steered_device) on device copies of the crowd -> a dict of host arrays.  The device forms take what the
    host forms refuse: poses and commands that are not finite."""
    import torch
    dev = torch.device("cuda", 0)
    B = c["x"].shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=dev)
    x, feet, stamp, cmd, sd, pose = up(c["x"]), up(c["feet"]), up(c["stamp"]), up(c["command"]), up(c["standing"]), up(c["pose"])
    xr, fo, pc, lp, ly = f64(B, horizon, 13), f64(B, horizon, 12), f64(B, horizon, 3), f64(B, 3), f64(B)
    ct = torch.full((B, horizon, 4), 9, dtype=torch.uint8, device=dev)
    out = dict(x_ref=xr, foot=fo, contact=ct, pcom=pc, landing=lp, landing_yaw=ly)
    if steered:
        e.mpc_inputs_steered_device(B, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), cmd.data_ptr(), ft.COM, xr.data_ptr(), fo.data_ptr(), ct.data_ptr(),
                                    pc.data_ptr(), landing=lp.data_ptr(), landing_yaw=ly.data_ptr(), standing=sd.data_ptr())
    else:
        e.mpc_inputs_tracked_device(B, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), cmd.data_ptr(), pose.data_ptr(), ft.COM, xr.data_ptr(), fo.data_ptr(),
                                    ct.data_ptr(), pc.data_ptr(), landing=lp.data_ptr(), landing_yaw=ly.data_ptr(), standing=sd.data_ptr(), **track)
        out["pose"] = pose
    e.synchronize()
    return {k: a.cpu().numpy() for k, a in out.items()}


def _close(got, want, what):
    """NaNs in the same places, everything else within 1e-12 -> the largest difference"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)
    d = d[np.isfinite(d)]
    # (an infinity on both sides is a NaN difference; on one side an infinite one, which fails below)
    assert np.array_equal(np.isinf(got), np.isinf(want)), what
    return float(d.max()) if d.size else 0.0


@pytest.mark.parametrize("horizon", [1, 10, 24, 15])
def test_tracked_inputs_against_the_twin(horizon):
    """77 robots (two tiles of 32 and a tail of 13) at N = 1, 10, 24 -- the bound of the kernel's tables -- and at the live horizon 15: robots inside the
    bounds, beyond each bound with both signs of yaw, a state, a pose and a command that are not finite."""
    plain = _crowd(B77, 300 + horizon)
    c = _odd(plain)
    with _engine(horizon) as e:
        got = _inputs_device(e, c, horizon)
        assert e.kernel_name() == "mpc_inputs_tracked_f64"
        calm = _inputs_device(e, plain, horizon)                  # the crowd without its odd robots
        steered = _inputs_device(e, c, horizon, steered=True)
        # the first identity: from the measured pose under moving commands, the device's own steered inputs
        m = {k: v.copy() for k, v in plain.items()}
        m["pose"] = ttw.start_pose(m["x"])
        m["command"][(m["command"][:, 0] == 0.0) & (m["command"][:, 1] == 0.0), 0] = 0.1
        ident, ident_st = _inputs_device(e, m, horizon), _inputs_device(e, m, horizon, steered=True)
    want = ttw.mpc_inputs(c["x"], c["feet"], c["stamp"], c["command"], c["pose"], ft.COM, horizon, DT, standing=c["standing"])
    # the crowd is what its names say
    assert want["engaged"][list(FAR + BOTH), 0].all() and want["engaged"][list(YAW_HI + YAW_LO + BOTH), 1].all()
    rest = np.setdiff1d(np.arange(B77), ODD)
    assert not want["engaged"][rest].any() and np.array_equal(_bits(want["bounded"][rest]), _bits(c["pose"][rest]))
    # what passes through no sine: bit for bit
    assert np.array_equal(got["contact"], want["contact"]) and np.array_equal(_bits(got["foot"]), _bits(want["foot"]))
    assert np.array_equal(_bits(got["x_ref"][:, :, EXACT_COLS]), _bits(want["x_ref"][:, :, EXACT_COLS]))
    assert np.array_equal(_bits(got["pcom"][:, :, 2]), _bits(want["pcom"][:, :, 2]))
    assert np.array_equal(_bits(got["landing_yaw"]), _bits(want["landing_yaw"]))
    assert np.array_equal(_bits(got["pose"][:, 2]), _bits(want["pose"][:, 2]))
    errs = dict(x_ref=_close(got["x_ref"][:, :, TRIG_COLS], want["x_ref"][:, :, TRIG_COLS], "x_ref"), pcom=_close(got["pcom"], want["pcom"], "pcom"),
                landing=_close(got["landing"], want["landing"], "landing"), pose=_close(got["pose"], want["pose"], "pose"))
    print("tracked inputs against the twin, N =", horizon, errs)
    with np.errstate(invalid="ignore"):
        assert np.nanmax(np.abs(np.where(np.isfinite(want["x_ref"][:, :, 2]), want["x_ref"][:, :, 2], 0.0))) < 10.0
    for k, v in errs.items():
        assert v <= 1e-12, (k, v)
    # section 1, robot by robot.  Beyond the position bound under a zero command: the references ARE the clamped pose, and it stays
    for b in (FAR[0], BOTH[0]):
        q = want["bounded"][b]
        assert np.hypot(*(q[0:2] - c["x"][b, 3:5])) < 0.1 + 1e-15 < np.hypot(*(c["pose"][b, 0:2] - c["x"][b, 3:5]))
        assert np.array_equal(_bits(got["x_ref"][b, :, 3:5]), _bits(np.tile(q[0:2], (horizon, 1)))) and np.array_equal(_bits(got["pose"][b]), _bits(q))
    # beyond the yaw bound: the heading references start at exactly psi0 +- yaw_lead_max
    for b, s in [(b, 1.0) for b in YAW_HI + BOTH[:1]] + [(b, -1.0) for b in YAW_LO + BOTH[1:]]:
        th = c["x"][b, 2] + s * 0.3
        assert np.array_equal(_bits(got["x_ref"][b, :, 2]), _bits(th + (c["command"][b, 2] * np.arange(1.0, horizon + 1)) * DT)), b
    # a state that is not finite clamps nothing, and the pose moves on
    for b in (NAN_X, NAN_YAW):
        assert np.isfinite(got["pose"][b]).all() and np.isfinite(got["x_ref"][b]).all()
        assert _bits(got["pose"][b, 2]) == _bits(c["pose"][b, 2] + (c["command"][b, 2] * 1.0) * DT)
    assert np.isnan(got["pcom"][NAN_X]).any() and np.isnan(got["landing"][NAN_YAW]).any()          # (what is measured there is not a number)
    # a pose or a command that is not finite: references that are not numbers, the pose as it stood after the bound
    for b in (NAN_POSE, NAN_TH, NAN_CMD, INF_CMD):
        assert not np.isfinite(got["x_ref"][b]).all() and np.array_equal(_bits(got["pose"][b]), _bits(want["bounded"][b])), b
    assert np.isfinite(want["bounded"][[NAN_CMD, INF_CMD]]).all()
    # what belongs to where the robot is: the device's own steered call, bit for bit, on every robot
    for k in ("foot", "contact", "pcom", "landing", "landing_yaw"):
        assert np.array_equal(_bits(got[k]), _bits(steered[k])), k
    # the neighbours of the odd robots are what they are without them
    for k in got:
        assert np.array_equal(_bits(got[k][rest]), _bits(calm[k][rest])), k
    # the first identity
    for k in ident_st:
        assert np.array_equal(_bits(ident[k]), _bits(ident_st[k])), k
    assert np.array_equal(_bits(ident["pose"][:, 0:2]), _bits(ident["x_ref"][:, 0, 3:5]))
    assert np.array_equal(_bits(ident["pose"][:, 2]), _bits(m["x"][:, 2] + (m["command"][:, 2] * 1.0) * DT))


def _tracked_loop(eng, c, B, steps, mode, horizon=N, track=True):
    """The tracked roll-out call, and the same steps driven from here through the public device calls on the same engine -- mpc_inputs_tracked_device ->
    (terrain_inputs_device + the normals set on the engine) -> solve_device -> (flush) -> fleet_advance_device(landing_yaw=) -> (wrench_observer_device) --
    -> two dicts of host arrays.  fleet_loop._device_loop's method, with the pose."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=dev)
    Nh, obs = horizon, mode == "observer"
    trk = {} if track is True else dict(track)
    alive0 = np.ones(B, np.uint8)
    if B > 4:
        alive0[3] = 0
    w0 = c["w0"] if obs else np.zeros((B, 6))
    out = []
    for call in (True, False):
        x, feet, stamp, sd, pu, al, w = up(c["x"]), up(c["feet"]), up(c["stamp"]), up(c["standing"]), up(c["push"]), up(alive0), up(w0)
        v, pose = up(c["command"]), up(c["pose"])
        if call:
            xl, ul, fl, wl, pl = f64(steps + 1, B, 13), f64(steps, B, 12), f64(steps + 1, B, 12), f64(steps, B, 6), f64(steps, B, 3)
            sl, il = torch.zeros((steps, B), dtype=torch.int32, device=dev), torch.zeros((steps, B), dtype=torch.int32, device=dev)
            eng.rollout_device(B, steps, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), 0, ft.COM, standing=sd.data_ptr(), push=pu.data_ptr(),
                               alive=al.data_ptr(), x_log=xl.data_ptr(), u0_log=ul.data_ptr(), feet_log=fl.data_ptr(), status_log=sl.data_ptr(),
                               iters_log=il.data_ptr(), command=v.data_ptr(), command_steps=1, track=track, pose=pose.data_ptr(), pose_log=pl.data_ptr(),
                               **(dict(observer=OBS, w_est=w.data_ptr(), w_log=wl.data_ptr()) if obs else {}))
            eng.synchronize()
            logs = dict(x_log=xl, u0_log=ul, feet_log=fl, status_log=sl, iters_log=il, pose_log=pl)
            if obs:
                logs["w_log"] = wl
        else:
            xr, fo, pc, lp, ly, cn = f64(B, Nh, 13), f64(B, Nh, 12), f64(B, Nh, 3), f64(B, 3), f64(B), f64(B, Nh, 12)
            ct = torch.zeros((B, Nh, 4), dtype=torch.uint8, device=dev)
            u, xo = f64(B, Nh, 12), f64(B, Nh + 1, 13)
            st, it = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            xs, fs, us, ss, its, ws, ps = [x.clone()], [feet.clone()], [], [], [], [], []
            if obs:
                ew = up(ot.horizon(w0, Nh, OBS["horizon_decay"]))
                eng.set_external_wrench(ew)
            try:
                for k in range(steps):
                    eng.mpc_inputs_tracked_device(B, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), v.data_ptr(), pose.data_ptr(), ft.COM, xr.data_ptr(),
                                                  fo.data_ptr(), ct.data_ptr(), pc.data_ptr(), landing=lp.data_ptr(), landing_yaw=ly.data_ptr(),
                                                  standing=sd.data_ptr(), **trk)
                    assert eng.kernel_name() == "mpc_inputs_tracked_f64"
                    if mode == "terrain":
                        eng.terrain_inputs_device(B, feet.data_ptr(), xr.data_ptr(), cn.data_ptr())
                        eng.set_contact_normals(cn)
                    eng.solve_device(B, x.data_ptr(), xr.data_ptr(), fo.data_ptr(), ct.data_ptr(), u.data_ptr(), x_out=xo.data_ptr(), status=st.data_ptr(),
                                     iters=it.data_ptr(), pcom=pc.data_ptr())
                    if mode == "defer":
                        eng.flush()
                    xp, fp = x.clone(), feet.clone()
                    eng.fleet_advance_device(B, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), u.data_ptr(), lp.data_ptr(), u0_stride=12 * Nh,
                                             standing=sd.data_ptr(), push=pu[k].data_ptr(), alive=al.data_ptr(), landing_yaw=ly.data_ptr())
                    if obs:
                        eng.wrench_observer_device(B, xp.data_ptr(), x.data_ptr(), fp.data_ptr(), u.data_ptr(), w.data_ptr(), ew=ew.data_ptr(), u0_stride=12 * Nh,
                                                   alive=al.data_ptr(), **OBS)
                    eng.synchronize()
                    xs.append(x.clone()); fs.append(feet.clone()); us.append(u[:, 0].clone()); ss.append(st.clone()); its.append(it.clone()); ws.append(w.clone())
                    ps.append(pose.clone())
            finally:
                eng.synchronize()
                if mode == "terrain":
                    eng.set_contact_normals(None)
                if obs:
                    eng.set_external_wrench(None)
            logs = dict(x_log=torch.stack(xs), u0_log=torch.stack(us), feet_log=torch.stack(fs), status_log=torch.stack(ss), iters_log=torch.stack(its),
                        pose_log=torch.stack(ps))
            if obs:
                logs["w_log"] = torch.stack(ws)
        logs.update(x=x, feet=feet, stamp=stamp, alive=al, pose=pose)
        if obs:
            logs["w_est"] = w
        out.append({k: a.cpu().numpy() for k, a in logs.items()})
    return out[0], out[1]


@pytest.mark.parametrize("mode", ["flat", "defer", "observer", "terrain"])
def test_the_tracked_loop_is_the_public_calls(mode):
    """rollout_device(command=, track=) over 20 steps of 6 robots against the public device calls driven step by step on the same engine: every log, pose_log
    and every final array bit for bit -- on flat ground, on a SRBDQP_FLAG_DEFER_TAIL engine, with the observer, and on an 8 x 8 map.  The bounds are tight
    enough to engage: the clamp is part of what is compared."""
    import torch  # noqa: F401
    from g1_locomotion_amd import _lib
    B, steps = 6, 20
    c = _crowd(B, 400, steps)
    c["feet"] = _turned_feet(c)
    c["w0"] = np.random.default_rng(B).uniform(-1.0, 1.0, (B, 6)) * np.array([0.5, 0.5, 0.1, 5.0, 5.0, 5.0])
    track = dict(lead_max=0.03, yaw_lead_max=0.1)
    with _engine(N, _lib.FLAG_DEFER_TAIL if mode == "defer" else 0) as e:
        if mode == "terrain":
            e.set_terrain(**tt.rough(8, 8, 5, cell=0.5, origin=(-1.5, -1.5), amp=0.1).args())
        call, loop = _tracked_loop(e, c, B, steps, mode, track=track)
    for k in call:
        assert np.array_equal(_bits(call[k]), _bits(loop[k])), k
    assert np.array_equal(_bits(call["pose_log"][-1]), _bits(call["pose"])) and np.array_equal(_bits(call["x_log"][-1]), _bits(call["x"]))
    assert (call["status_log"] == 1).mean() > 0.5 and np.any(call["feet_log"][-1] != call["feet_log"][0])
    assert np.array_equal(_bits(call["x_log"][:, 3]), _bits(np.tile(c["x"][3], (steps + 1, 1)))) and call["alive"][3] == 0     # the robot that came in dead held
    # ... while its pose kept being clamped to that held state
    lead = np.hypot(*(call["pose_log"][:, 3, 0:2] - c["x"][3, 3:5]).T)
    assert lead.max() <= 0.03 + np.linalg.norm(c["command"][3, 0:2]) * DT + 1e-12
    # the bounds engaged somewhere: the pose log is not the commands integrated freely
    free = ttw.ideal_path(np.concatenate([np.zeros((B, 2)), c["pose"][:, 2:3], c["pose"][:, 0:2], np.zeros((B, 8))], axis=1), c["command"], steps, DT)
    assert np.abs(call["pose_log"] - free[1:]).max() > 1e-3


@pytest.fixture(scope="module")
def eng():
    import torch  # noqa: F401
    from g1_locomotion_amd import BatchMPC
    e = BatchMPC(horizon=N)
    yield e
    e.close()


def test_host_and_device_forms_agree(eng):
    """rollout(track=) on host arrays against rollout_device(track=) on device copies, B = 6, T = 20, with the observer (every array the host form stages):
    every log and every final array bit for bit; and the host inputs call against the device one."""
    import torch
    B, T = 6, 20
    c = _crowd(B, 31, T)
    c["feet"] = _turned_feet(c)
    alive0 = np.ones(B, np.uint8)
    alive0[3] = 0
    w0 = np.random.default_rng(B).uniform(-1.0, 1.0, (B, 6)) * np.array([0.5, 0.5, 0.1, 5.0, 5.0, 5.0])
    track = dict(lead_max=0.03, yaw_lead_max=0.1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    host = eng.rollout(c["x"], c["feet"], c["stamp"], None, T, ft.COM, standing=c["standing"], push=c["push"], alive=alive0, command=c["command"], track=track,
                       pose=c["pose"], observer=OBS, w_est=w0)
    dev = {k: up(a) for k, a in dict(x=c["x"], feet=c["feet"], stamp=c["stamp"], standing=c["standing"], push=c["push"], alive=alive0, w_est=w0,
                                     vel=c["command"], pose=c["pose"]).items()}
    logs = {k: up(np.full_like(host[k], 7)) for k in ("x", "u0", "feet", "status", "iters", "w_log", "pose_log")}
    ptr = lambda k: logs[k].data_ptr()
    eng.rollout_device(B, T, dev["x"].data_ptr(), dev["feet"].data_ptr(), dev["stamp"].data_ptr(), 0, ft.COM, standing=dev["standing"].data_ptr(),
                       push=dev["push"].data_ptr(), alive=dev["alive"].data_ptr(), x_log=ptr("x"), u0_log=ptr("u0"), feet_log=ptr("feet"),
                       status_log=ptr("status"), iters_log=ptr("iters"), command=dev["vel"].data_ptr(), command_steps=1, track=track,
                       pose=dev["pose"].data_ptr(), pose_log=ptr("pose_log"), observer=OBS, w_est=dev["w_est"].data_ptr(), w_log=ptr("w_log"))
    eng.synchronize()
    for k, a in logs.items():
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(host[k])), k
    finals = dict(x=host["x"][-1], feet=host["feet"][-1], stamp=host["stamp"], alive=host["alive"], w_est=host["w_est"], pose=host["pose"])
    for k, a in finals.items():
        assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(a)), k
    assert np.array_equal(_bits(host["pose"]), _bits(host["pose_log"][-1])) and (host["status"] == 1).any() and np.any(host["x"][-1] != host["x"][0])
    assert np.array_equal(c["pose"], _crowd(B, 31, T)["pose"])                   # (the caller's pose is not modified)
    a = eng.mpc_inputs_tracked(c["x"], c["feet"], c["stamp"], c["command"], c["pose"], ft.COM, standing=c["standing"], **track)
    assert eng.kernel_name() == "mpc_inputs_tracked_f64"
    b = _inputs_device(eng, c, N, **track)
    for k in b:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_chunks_and_schedules_compose(eng):
    """T = 20 in one call = 12 + 8 with the pose carried, bit for bit; and a (20, B, 3) schedule that changes command at step 12 = the two constant-command
    chunks it is made of; a pose that is not carried gives another roll-out."""
    B, steps = 21, 20
    c = _crowd(B, 7, steps)
    c["feet"] = _turned_feet(c)
    c1 = c["command"].copy()
    c1[:, 2] = 0.3 - c1[:, 2]
    c1[:, 0] += 0.05
    kw = dict(standing=c["standing"], track=dict(lead_max=0.03, yaw_lead_max=0.1))
    run = lambda x, feet, stamp, cmd, n, push, **k: eng.rollout(x, feet, stamp, None, n, ft.COM, command=cmd, push=push, **kw, **k)
    for second in (c["command"], c1):
        a = run(c["x"], c["feet"], c["stamp"], c["command"], 12, c["push"][:12], pose=c["pose"])
        b = run(a["x"][-1], a["feet"][-1], a["stamp"], second, 8, c["push"][12:], alive=a["alive"], pose=a["pose"])
        whole = c["command"] if second is c["command"] else np.concatenate([np.tile(c["command"], (12, 1, 1)), np.tile(c1, (8, 1, 1))])
        w = run(c["x"], c["feet"], c["stamp"], whole, steps, c["push"], pose=c["pose"])
        for k in ("x", "feet"):
            assert np.array_equal(_bits(np.concatenate([a[k], b[k][1:]])), _bits(w[k])), k
        for k in ("u0", "status", "iters", "pose_log"):
            assert np.array_equal(_bits(np.concatenate([a[k], b[k]])), _bits(w[k])), k
        assert np.array_equal(b["alive"], w["alive"]) and np.array_equal(_bits(b["stamp"]), _bits(w["stamp"])) and np.array_equal(_bits(b["pose"]), _bits(w["pose"]))
    lost = run(a["x"][-1], a["feet"][-1], a["stamp"], c1, 8, c["push"][12:], alive=a["alive"])
    assert np.any(lost["pose_log"] != b["pose_log"]) and np.any(lost["x"][-1] != b["x"][-1])
    # pose=None starts on the measured state
    s0 = run(c["x"], c["feet"], c["stamp"], c["command"], 3, c["push"][:3])
    s1 = run(c["x"], c["feet"], c["stamp"], c["command"], 3, c["push"][:3], pose=ttw.start_pose(c["x"]))
    for k in ("x", "u0", "pose_log", "pose"):
        assert np.array_equal(_bits(s0[k]), _bits(s1[k])), k


def test_without_track_the_rollout_is_the_steered_one(eng):
    """rollout(command=, track=None) against srbdqp_fleet_rollout_steered_f64 in the same process: bit for bit, and no pose in the result; track= without
    command= and pose= without track= are ValueErrors."""
    steps, B = 9, 21
    c = _crowd(B, 17, steps)
    c["feet"] = _turned_feet(c)
    got = eng.rollout(c["x"], c["feet"], c["stamp"], None, steps, ft.COM, standing=c["standing"], push=c["push"], command=c["command"], track=None)
    x, feet, stamp, al = c["x"].copy(), c["feet"].copy(), c["stamp"].copy(), np.ones(B, np.uint8)
    xl, ul, fl = np.empty((steps + 1, B, 13)), np.empty((steps, B, 12)), np.empty((steps + 1, B, 12))
    sl, il = np.empty((steps, B), np.int32), np.empty((steps, B), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    s = eng.fleet_settings(ft.COM)
    rc = eng._lib.srbdqp_fleet_rollout_steered_f64(eng._h, B, steps, p(x), p(feet), p(stamp), p(c["command"]), 1, p(c["standing"]), p(c["push"]), C.byref(s), p(al),
                                                   p(xl), p(ul), p(fl), p(sl), p(il), None, None, None)
    assert rc == 0
    for k, v in dict(x=xl, u0=ul, feet=fl, status=sl, iters=il, alive=al, stamp=stamp).items():
        assert np.array_equal(_bits(got[k]), _bits(v)), k
    assert "pose" not in got and "pose_log" not in got
    tracked = eng.rollout(c["x"], c["feet"], c["stamp"], None, steps, ft.COM, standing=c["standing"], push=c["push"], command=c["command"], track=True)
    assert np.any(tracked["x"][-1] != got["x"][-1]) and tracked["pose_log"].shape == (steps, B, 3)
    with pytest.raises(ValueError, match="track="):
        eng.rollout(c["x"], c["feet"], c["stamp"], c["command"][:, 0:2], steps, ft.COM, track=True)
    with pytest.raises(ValueError, match="pose"):
        eng.rollout(c["x"], c["feet"], c["stamp"], None, steps, ft.COM, command=c["command"], pose=c["pose"])


def test_refusals_and_plain_solves_unchanged(eng):
    """The refusals for the handle's state are those of the roll-out the call becomes; nothing is launched on a refused call; and the engine's plain solves
    are what they were before a tracked roll-out ran on it."""
    import torch
    from g1_locomotion_amd import SrbdqpError
    steps, B = 3, 21
    c = _crowd(B, 23, steps)
    c["feet"] = _turned_feet(c)
    x0, xr, ft_, ct = orc.synthetic_batch(64, N, seed=3, schedule="single")
    before = eng.solve(x0, xr, ft_, ct)
    run = lambda **k: eng.rollout(c["x"], c["feet"], c["stamp"], None, steps, ft.COM, command=c["command"], **{**dict(track=True, pose=c["pose"]), **k})
    bad = c["pose"].copy(); bad[4, 2] = np.nan
    with pytest.raises(SrbdqpError, match="pose of robot 4.*not finite"):
        run(pose=bad)
    with pytest.raises(SrbdqpError, match="pose of robot 4.*not finite"):
        eng.mpc_inputs_tracked(c["x"], c["feet"], c["stamp"], c["command"], bad, ft.COM)
    badc = c["command"].copy(); badc[2, 1] = np.inf
    with pytest.raises(SrbdqpError, match="command of robot 2.*not finite"):
        eng.rollout(c["x"], c["feet"], c["stamp"], None, steps, ft.COM, command=badc, track=True)
    with pytest.raises(SrbdqpError, match="srbdqp_track_settings"):
        run(track=dict(lead_max=0.0))
    with pytest.raises(SrbdqpError, match="srbdqp_track_settings"):
        run(track=dict(yaw_lead_max=np.inf))
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x, feet, stamp, cm, po = up(c["x"]), up(c["feet"]), up(c["stamp"]), up(c["command"]), up(c["pose"])
    with pytest.raises(SrbdqpError, match="pose is NULL"):
        eng.rollout_device(B, steps, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), 0, ft.COM, command=cm.data_ptr(), track=True)
    # what the roll-out it becomes refuses: a wrench set on the engine, bad fleet settings, an observed roll-out on a map
    eng.set_external_wrench(np.full((B, N, 6), 0.5))
    try:
        with pytest.raises(SrbdqpError, match="srbdqp_set_external_wrench"):
            run()
    finally:
        eng.set_external_wrench(None)
    with pytest.raises(SrbdqpError, match="srbdqp_fleet_settings"):
        run(substeps=0)
    eng.set_terrain(np.zeros((4, 5)), origin=(-2.0, -2.0), cell=1.5)
    try:
        with pytest.raises(SrbdqpError, match="terrain"):
            run(observer=True)
        with pytest.raises(SrbdqpError, match="terrain"):
            eng.rollout_device(B, steps, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), 0, ft.COM, command=cm.data_ptr(), track=True, pose=po.data_ptr(),
                               observer=True, w_est=up(np.zeros((B, 6))).data_ptr())
    finally:
        eng.set_terrain(None)
    eng.synchronize()
    assert np.array_equal(po.cpu().numpy(), c["pose"]) and np.array_equal(x.cpu().numpy(), c["x"])                # nothing was launched on the refused calls
    r = run()
    assert r["status"].max() == 1
    after = eng.solve(x0, xr, ft_, ct)
    assert {"u", "status", "iters"} <= set(before)
    for k, v in before.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(_bits(v), _bits(after[k])), k


def test_free_running_against_the_twin(eng):
    """The six robots of steer_twin.fleet() over 50 steps from the measured pose, the engine and the twin each on its own trajectory: every robot alive on both,
    the iteration counts equal, states and poses within 1e-4 -- test_gpu_steer.py's bounds."""
    T = 50
    f = stw.fleet()
    want = ttw.rollout(orc.default_params(N), f["x"], f["feet"], f["stamp"], f["command"], T, ft.COM, standing=f["standing"], solver="c")
    got = eng.rollout(f["x"], f["feet"], f["stamp"], None, T, ft.COM, standing=f["standing"], command=f["command"], track=True)
    err = np.abs(got["x"] - want["x"]).max(axis=(0, 2))
    eyaw = np.abs(got["x"][T, :, 2] - want["x"][T, :, 2])
    epose = np.abs(got["pose_log"] - want["pose_log"]).max()
    ideal = ttw.ideal_path(f["x"], f["command"], T, DT)
    print("free-running tracked: max |x - twin| per robot", err.tolist(), "final yaw against the twin's", eyaw.tolist(), "pose log", epose,
          "distance from the path after 2 s", np.hypot(*(got["x"][T, :, 3:5] - ideal[T, :, 0:2]).T).tolist(),
          "steps with other iters", (got["iters"] != want["iters"]).sum(axis=0).tolist())
    assert got["alive"].tolist() == [1] * 6 and want["alive"].tolist() == [1] * 6
    assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["status"], want["status"])
    assert err.max() < 1e-4, err
    assert eyaw.max() < 1e-4, eyaw
    assert epose <= 1e-12, epose                                    # (the bounds never engage here: the pose is the commands integrated)


def test_the_tile_loop_takes_its_second_trip():
    """test_gpu_tile_loops.py's method on srbdqp_mpc_inputs_commanded_kernel's tracked instantiation, whose launcher caps the grid at 256 * 32 workgroups: the 77-robot crowd, odd robots
    and all, repeated to 262,189 robots = cap * 32 + 32 + 13 on an engine of horizon 4, robot b being robot b mod 77.  Every output and the pose behind the step
    equal the 77-robot call's gathered by the same index, bit for bit; so does the pose_log row of a one-step roll-out of the large fleet."""
    import torch
    t0 = time.perf_counter()
    cap, tile, Nh = 256 * 32, 32, 4
    B = cap * tile + tile + 13
    assert B == 262189 and B // tile > cap and -(-B // tile) == cap + 2 and B % tile == 13
    c = _odd(_crowd(B77, 900))
    idx = np.arange(B) % B77
    big = {k: (v if k == "push" else np.take(v, idx, axis=0)) for k, v in c.items()}
    with _engine(Nh) as e:
        small = _inputs_device(e, c, Nh)
        assert np.isnan(small["pcom"]).any() and np.isnan(small["x_ref"]).any() and small["contact"].min() == 0
        large = _inputs_device(e, big, Nh)
        assert e.kernel_name() == "mpc_inputs_tracked_f64"
        for k, v in small.items():
            want = np.take(v, idx, axis=0)
            assert large[k].shape == want.shape and np.array_equal(_bits(large[k]), _bits(want)), k
            del want
        del large
        # ... and the row of pose_log, which the same kernel writes in a roll-out
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        x, feet, stamp, cm, sd, po = up(big["x"]), up(big["feet"]), up(big["stamp"]), up(big["command"]), up(big["standing"]), up(big["pose"])
        pl = torch.full((1, B, 3), -7.0, dtype=torch.float64, device=dev)
        e.rollout_device(B, 1, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), 0, ft.COM, standing=sd.data_ptr(), command=cm.data_ptr(), command_steps=1,
                         track=True, pose=po.data_ptr(), pose_log=pl.data_ptr())
        e.synchronize()
        want = np.take(small["pose"], idx, axis=0)
        assert np.array_equal(_bits(pl.cpu().numpy()[0]), _bits(want)) and np.array_equal(_bits(po.cpu().numpy()), _bits(want))
    print(f"mpc_inputs_tracked, second trip: B = {B} robots = {-(-B // tile)} tiles of {tile} on {cap} workgroups, {time.perf_counter() - t0:.1f} s")
