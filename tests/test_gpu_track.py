"""GPU tests of the tracked fleet calls (include/srbdqp_cascade.h srbdqp_mpc_inputs_tracked_*, srbdqp_fleet_rollout_tracked_*) against
the NumPy twin of tests/track_twin.py (tests/test_track_cpu.py holds the twin itself).

Bounds: those of test_gpu_steer.py.  What passes through no sine or cosine is compared bit for bit -- the bounded pose, the heading references, the heading
behind the step among it.  What does: 1e-12 absolute -- the device's sin / cos against NumPy's at arguments below 10, on values of order 1, through at most 24
sums.  Free-running trajectories: 1e-4 at 50 steps, with every iteration count equal to the twin's."""
import numpy as np
import pytest

import c_oracle  # noqa: F401
import srbd_oracle as orc
import fleet_twin as ft
from fleet_loop import OBS, _bits, crowd, device_loop, direct_rollout, engine, inputs_device, rollout_device_against_host, turned_feet
import steer_twin as stw
import terrain_twin as tt
import track_twin as ttw

pytestmark = pytest.mark.gpu
N, DT, B77 = 10, 0.04, 77
EXACT_COLS = [0, 1, 2, 5, 6, 7, 8, 11, 12]
TRIG_COLS = [3, 4, 9, 10]
# the robots of the 77-robot crowd that are not plainly inside the bounds
FAR, YAW_HI, YAW_LO, BOTH, NAN_X, NAN_YAW, NAN_POSE, NAN_TH, NAN_CMD, INF_CMD = (5, 37, 70), (11, 44), (12, 45), (20, 66), 9, 33, 40, 41, 50, 76
ODD = FAR + YAW_HI + YAW_LO + BOTH + (NAN_X, NAN_YAW, NAN_POSE, NAN_TH, NAN_CMD, INF_CMD)


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
    plain = crowd("commanded", B77, 300 + horizon, pose=True)
    c = _odd(plain)
    with engine(horizon) as e:
        got = inputs_device(e, c, horizon, "tracked")
        assert e.kernel_name() == "mpc_inputs_tracked_f64"
        calm = inputs_device(e, plain, horizon, "tracked")                  # the crowd without its odd robots
        steered = inputs_device(e, c, horizon, "steered")
        # the first identity: from the measured pose under moving commands, the device's own steered inputs
        m = {k: v.copy() for k, v in plain.items()}
        m["pose"] = ttw.start_pose(m["x"])
        m["command"][(m["command"][:, 0] == 0.0) & (m["command"][:, 1] == 0.0), 0] = 0.1
        ident, ident_st = inputs_device(e, m, horizon, "tracked"), inputs_device(e, m, horizon, "steered")
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


@pytest.mark.parametrize("mode", ["flat", "defer", "observer", "terrain"])
def test_the_tracked_loop_is_the_public_calls(mode):
    """rollout_device(command=, track=) over 20 steps of 6 robots against the public device calls driven step by step on the same engine: every log, pose_log
    and every final array bit for bit -- on flat ground, on a SRBDQP_FLAG_DEFER_TAIL engine, with the observer, and on an 8 x 8 map.  The bounds are tight
    enough to engage: the clamp is part of what is compared."""
    import torch  # noqa: F401
    from g1_locomotion_amd import _lib
    B, steps = 6, 20
    c = crowd("commanded", B, 400, steps, pose=True)
    c["feet"] = turned_feet(c)
    c["w0"] = np.random.default_rng(B).uniform(-1.0, 1.0, (B, 6)) * np.array([0.5, 0.5, 0.1, 5.0, 5.0, 5.0])
    track = dict(lead_max=0.03, yaw_lead_max=0.1)
    with engine(N, _lib.FLAG_DEFER_TAIL if mode == "defer" else 0) as e:
        if mode == "terrain":
            e.set_terrain(**tt.rough(8, 8, 5, cell=0.5, origin=(-1.5, -1.5), amp=0.1).args())
        call, loop, _ = device_loop(e, c, B, steps, mode, observer=OBS, track=track)
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
    B, T = 6, 20
    c = crowd("commanded", B, 31, T, pose=True)
    c["feet"] = turned_feet(c)
    w0 = np.random.default_rng(B).uniform(-1.0, 1.0, (B, 6)) * np.array([0.5, 0.5, 0.1, 5.0, 5.0, 5.0])
    track = dict(lead_max=0.03, yaw_lead_max=0.1)
    host = rollout_device_against_host(eng, c, T, observer=OBS, w0=w0, track=track)
    assert np.array_equal(_bits(host["pose"]), _bits(host["pose_log"][-1])) and (host["status"] == 1).any() and np.any(host["x"][-1] != host["x"][0])
    assert np.array_equal(c["pose"], crowd("commanded", B, 31, T, pose=True)["pose"])                   # (the caller's pose is not modified)
    a = eng.mpc_inputs_tracked(c["x"], c["feet"], c["stamp"], c["command"], c["pose"], ft.COM, standing=c["standing"], **track)
    assert eng.kernel_name() == "mpc_inputs_tracked_f64"
    b = inputs_device(eng, c, N, "tracked", **track)
    for k in b:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_chunks_and_schedules_compose(eng):
    """T = 20 in one call = 12 + 8 with the pose carried, bit for bit; and a (20, B, 3) schedule that changes command at step 12 = the two constant-command
    chunks it is made of; a pose that is not carried gives another roll-out."""
    B, steps = 21, 20
    c = crowd("commanded", B, 7, steps, pose=True)
    c["feet"] = turned_feet(c)
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
    c = crowd("commanded", B, 17, steps, pose=True)
    c["feet"] = turned_feet(c)
    got = eng.rollout(c["x"], c["feet"], c["stamp"], None, steps, ft.COM, standing=c["standing"], push=c["push"], command=c["command"], track=None)
    want = direct_rollout(eng, "srbdqp_fleet_rollout_steered_f64", c, steps, c["command"])
    for k, v in want.items():
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
    c = crowd("commanded", B, 23, steps, pose=True)
    c["feet"] = turned_feet(c)
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
    x, feet, stamp, cm, po, we = up(c["x"]), up(c["feet"]), up(c["stamp"]), up(c["command"]), up(c["pose"]), up(np.zeros((B, 6)))
    torch.cuda.synchronize()                                      # (fleet_loop.py's stream rule)
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
                               observer=True, w_est=we.data_ptr())
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
