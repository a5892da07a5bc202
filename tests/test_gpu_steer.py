"""GPU tests of the steered fleet calls (include/srbdqp_cascade.h srbdqp_mpc_inputs_steered_*, srbdqp_fleet_advance_steered_*, srbdqp_fleet_rollout_steered_*;
DESIGN.md section 20) against the NumPy twin of tests/steer_twin.py (tests/test_steer_cpu.py holds the twin itself).

Bounds.  What passes through no sine or cosine is compared bit for bit.  What does: 1e-12 absolute -- the device's sin / cos against NumPy's at arguments below
10, on values of order 1, through at most 24 sums.  States behind a plant period: 1e-9, the bar of test_gpu_fleet.py.  Free-running trajectories: 1e-4,
test_gpu_fleet.py's bar for its fleet at the same 50 steps, with every iteration count equal to the twin's."""
import ctypes as C

import numpy as np
import pytest

import c_oracle  # noqa: F401
import srbd_oracle as orc
import fleet_twin as ft
from fleet_loop import OBS, _bits, crowd, device_loop, direct_rollout, engine, rollout_device_against_host, turned_feet
import steer_twin as stw
import terrain_twin as tt

pytestmark = pytest.mark.gpu
N, DT, B77 = 10, 0.04, 77
EXACT_COLS = [0, 1, 5, 6, 7, 8, 11, 12]
TRIG_COLS = [2, 3, 4, 9, 10]


@pytest.fixture(scope="module")
def eng():
    import torch  # noqa: F401
    from g1_locomotion_amd import BatchMPC
    e = BatchMPC(horizon=N)
    yield e
    e.close()


@pytest.mark.parametrize("horizon", [10, 7, 24])
def test_steered_inputs_against_the_twin(horizon):
    """77 robots (two tiles of 32 and a tail of 13), at N = 10, at the live horizon 7 and at N = 24, the bound of the kernel's table."""
    c = crowd("commanded", B77, 100 + horizon)
    with engine(horizon) as e:
        got = e.mpc_inputs_steered(c["x"], c["feet"], c["stamp"], c["command"], ft.COM, standing=c["standing"])
        assert e.kernel_name() == "mpc_inputs_steered_f64"
        # a zero command at yaw 0: the device's own mpc_inputs
        z = {k: v.copy() for k, v in c.items()}
        z["x"][:, 2] = 0.0
        a = e.mpc_inputs_steered(z["x"], z["feet"], z["stamp"], np.zeros((B77, 3)), ft.COM, standing=z["standing"])
        b = e.mpc_inputs(z["x"], z["feet"], z["stamp"], np.zeros((B77, 2)), ft.COM, standing=z["standing"])
    want = stw.mpc_inputs(c["x"], c["feet"], c["stamp"], c["command"], ft.COM, horizon, DT, standing=c["standing"])
    assert np.array_equal(got["contact"], want["contact"]) and np.array_equal(_bits(got["foot"]), _bits(want["foot"]))
    assert np.array_equal(_bits(got["x_ref"][:, :, EXACT_COLS]), _bits(want["x_ref"][:, :, EXACT_COLS]))
    assert np.array_equal(_bits(got["pcom"][:, :, 2]), _bits(want["pcom"][:, :, 2]))
    errs = dict(x_ref=np.abs(got["x_ref"][:, :, TRIG_COLS] - want["x_ref"][:, :, TRIG_COLS]).max(), pcom=np.abs(got["pcom"] - want["pcom"]).max(),
                landing=np.abs(got["landing"] - want["landing"]).max(), landing_yaw=np.abs(got["landing_yaw"] - want["landing_yaw"]).max())
    print("steered inputs against the twin, N =", horizon, errs)
    assert np.abs(want["x_ref"][:, :, 2]).max() < 10.0
    for k, v in errs.items():
        assert v <= 1e-12, (k, v)
    assert np.all(got["landing"][:, 2] == 0.0)
    for k in ("x_ref", "foot", "contact", "pcom", "landing"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["landing_yaw"], np.zeros(B77))


def _period(seed):
    """One period's inputs for 77 robots: the crowd, the forces of a robot held up on its four contacts and a little more, the twin's landing points and
    headings, some robots dead, random pushes."""
    c = crowd("commanded", B77, seed)
    rng = np.random.default_rng(seed + 1)
    p = orc.default_params(N)
    c["feet"] = turned_feet(c)
    inp = stw.mpc_inputs(c["x"], c["feet"], c["stamp"], c["command"], ft.COM, N, DT, standing=c["standing"])
    u0 = np.tile([0.0, 0.0, p.mass * 9.80665 / 4.0], (B77, 4)) + rng.normal(size=(B77, 12)) * 5.0
    x = c["x"].copy()
    x[:, 6:12] += rng.normal(size=(B77, 6)) * 0.05
    push = rng.uniform(-1.0, 1.0, (B77, 6)) * np.array([3.0, 3.0, 0.3, 30.0, 30.0, 30.0])
    alive = (rng.random(B77) > 0.15).astype(np.uint8)
    return p, x, c["feet"], c["stamp"], u0, inp["landing"], inp["landing_yaw"], c["standing"], push, alive


def _moved(got_feet, feet):
    return np.where(np.any(got_feet[:, 0:6] != feet[:, 0:6], axis=1), 1, np.where(np.any(got_feet[:, 6:12] != feet[:, 6:12], axis=1), 2, 0))


def test_one_steered_period_against_the_twin(eng):
    """One period of 77 robots (a tile of 64 and a tail of 13), left touchdowns, right touchdowns and none among them: stamps, alive flags and which foot moved bit
    for bit, footholds within 1e-12, states within 1e-9; with landing_yaw = 0 it is fleet_advance bit for bit; and once more on an 8 x 8 map, where heel and toe
    stand at the map's height under the turned points."""
    p, x, feet, stamp, u0, landing, yaw, standing, push, alive = _period(31)
    kw = dict(standing=standing, push=push, alive=alive)
    want = stw.advance(p, x, feet, stamp, u0, landing, yaw, **kw)
    got = eng.fleet_advance(x, feet, stamp, u0, landing, landing_yaw=yaw, **kw)
    assert eng.kernel_name() == "fleet_advance_steered_f64"
    assert {1, 2} <= set(want["moved"].tolist()) and (want["moved"] == 0).sum() > 20 and 0 < (alive == 0).sum() < B77 // 2
    assert np.array_equal(_moved(got["feet"], feet), want["moved"])
    assert np.array_equal(_bits(got["stamp"]), _bits(want["stamp"])) and np.array_equal(got["alive"], want["alive"])
    ef, ex = np.abs(got["feet"] - want["feet"]).max(), np.abs(got["x"] - want["x"]).max()
    print("steered period against the twin: footholds", ef, "states", ex)
    assert ef <= 1e-12 and ex < 1e-9, (ef, ex)
    stay = want["moved"] == 0
    assert np.array_equal(_bits(got["feet"][stay]), _bits(feet[stay]))
    # the feet that landed lie along their heading
    land = want["moved"] != 0
    c0 = np.where(want["moved"][land] == 1, 0, 6)
    rows = got["feet"][land]
    d = np.array([rows[i, c + 3:c + 5] - rows[i, c:c + 2] for i, c in enumerate(c0)])
    assert np.abs(d - 0.17 * np.stack([np.cos(yaw[land]), np.sin(yaw[land])], axis=1)).max() < 1e-12 and np.abs(np.sin(yaw[land])).max() > 0.5
    # landing_yaw = 0: the unsteered step
    a = eng.fleet_advance(x, feet, stamp, u0, landing, landing_yaw=np.zeros(B77), **kw)
    b = eng.fleet_advance(x, feet, stamp, u0, landing, **kw)
    assert eng.kernel_name() == "fleet_advance_f64"
    for k in ("x", "feet", "stamp", "alive"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    # ... and on a small map
    m = tt.rough(8, 8, 5, cell=0.5, origin=(-1.5, -1.5), amp=0.3)
    want = stw.advance(p, x, feet, stamp, u0, landing, yaw, terrain=m, **kw)
    eng.set_terrain(**m.args())
    try:
        got = eng.fleet_advance(x, feet, stamp, u0, landing, landing_yaw=yaw, **kw)
        assert eng.kernel_name() == "fleet_advance_terrain_steered_f64"
    finally:
        eng.set_terrain(None)
    assert np.array_equal(_moved(got["feet"], feet), want["moved"]) and np.array_equal(got["alive"], want["alive"])
    ef, ex = np.abs(got["feet"] - want["feet"]).max(), np.abs(got["x"] - want["x"]).max()
    print("steered period on the map against the twin: footholds", ef, "states", ex)
    assert ef <= 1e-12 and ex < 1e-9, (ef, ex)
    rows = got["feet"][land]
    zs = np.array([[rows[i, c + 2], rows[i, c + 5]] for i, c in enumerate(c0)])
    pts = np.array([[rows[i, c:c + 2], rows[i, c + 3:c + 5]] for i, c in enumerate(c0)]).reshape(-1, 2)
    assert np.abs(zs.reshape(-1) - tt.sample(m, pts)[0]).max() <= 1e-12 and np.ptp(zs) > 1e-3                                       # (the map is not flat where they landed)


@pytest.mark.parametrize("B,mode,horizon", [(B77, "flat", 10), (B77, "flat", 7), (6, "defer", 10), (6, "terrain", 10), (6, "observer", 10)])
def test_the_steered_loop_is_the_public_calls(B, mode, horizon):
    """rollout_device(command=) over 12 steps against mpc_inputs_steered_device -> (terrain_inputs_device + the normals set on the engine) -> solve_device ->
    (flush) -> fleet_advance_device(landing_yaw=) -> (wrench_observer_device) driven step by step on the same engine: every log and every final array bit for
    bit -- on flat ground at N = 10 and at the live horizon 7, on a SRBDQP_FLAG_DEFER_TAIL engine, on a map, and with the observer."""
    import torch  # noqa: F401
    from g1_locomotion_amd import _lib
    steps = 12
    c = crowd("commanded", B, 200 + B + horizon, steps)
    c["feet"] = turned_feet(c)
    c["w0"] = np.random.default_rng(B).uniform(-1.0, 1.0, (B, 6)) * np.array([0.5, 0.5, 0.1, 5.0, 5.0, 5.0])
    with engine(horizon, _lib.FLAG_DEFER_TAIL if mode == "defer" else 0) as e:
        if mode == "terrain":
            e.set_terrain(**tt.rough(8, 8, 5, cell=0.5, origin=(-1.5, -1.5), amp=0.1).args())
        call, loop, _ = device_loop(e, c, B, steps, mode, horizon=horizon, observer=OBS)
    for k in call:
        assert np.array_equal(_bits(call[k]), _bits(loop[k])), k
    assert np.array_equal(_bits(call["x_log"][-1]), _bits(call["x"])) and np.array_equal(_bits(call["x_log"][0]), _bits(c["x"]))
    assert (call["status_log"] == 1).mean() > 0.5 and np.any(call["feet_log"][-1] != call["feet_log"][0])
    assert np.array_equal(_bits(call["x_log"][:, 3]), _bits(np.tile(c["x"][3], (steps + 1, 1)))) and call["alive"][3] == 0     # the robot that came in dead held


@pytest.mark.parametrize("flavour", ["flat", "terrain", "observed", "steered_observed"])
def test_host_and_device_buffers_agree(flavour):
    """rollout() on host arrays against rollout_device() on device copies of the same inputs, B = 6, T = 3, N = 10 -- flat, on a map, observed (all three
    from v_ref) and steered with the observer: every log and every final array bit for bit.  The host form stages what the flavour has and runs the same loop.
    (That an observed rollout_device() without logs, through the two-slot ring, ends in the x, feet and w_est of the call with logs: test_gpu_observer.py's
    test_chunks_compose.)"""
    import torch  # noqa: F401
    from g1_locomotion_amd import BatchMPC
    B, T = 6, 3
    steered, observed = flavour.startswith("steered"), flavour.endswith("observed")
    c = crowd("commanded", B, 31, T)
    if steered:
        c["feet"] = turned_feet(c)
    else:
        c["x"][:, 2] = 0.0                                                      # (v_ref is a world-frame velocity: the nominal stance, unturned)
    v_ref = None if steered else c["command"][:, 0:2].copy()
    w0 = np.random.default_rng(B).uniform(-1.0, 1.0, (B, 6)) * np.array([0.5, 0.5, 0.1, 5.0, 5.0, 5.0])
    with BatchMPC(horizon=N) as e:
        if flavour == "terrain":
            e.set_terrain(**tt.rough(8, 8, 5, cell=0.5, origin=(-1.5, -1.5), amp=0.1).args())
        host = rollout_device_against_host(e, c, T, v_ref=v_ref, **(dict(observer=OBS, w0=w0) if observed else {}))
    assert (host["status"] == 1).any() and host["alive"][3] == 0 and np.any(host["x"][-1] != host["x"][0])       # (solves that solved, robots that moved)
    assert ("w_est" in host) == observed and ("w_log" in host) == observed


def test_chunks_and_schedules_compose(eng):
    """T = 12 in one call = 5 + 7, bit for bit; and a (12, B, 3) schedule that changes command at step 5 = the two constant-command chunks it is made of."""
    B, steps = 21, 12
    c = crowd("commanded", B, 7, steps)
    c["feet"] = turned_feet(c)
    c1 = c["command"].copy()
    c1[:, 2] = 0.3 - c1[:, 2]
    c1[:, 0] += 0.05
    kw = dict(standing=c["standing"])
    run = lambda x, feet, stamp, cmd, n, push, **k: eng.rollout(x, feet, stamp, None, n, ft.COM, command=cmd, push=push, **kw, **k)
    for second in (c["command"], c1):
        a = run(c["x"], c["feet"], c["stamp"], c["command"], 5, c["push"][:5])
        b = run(a["x"][-1], a["feet"][-1], a["stamp"], second, 7, c["push"][5:], alive=a["alive"])
        whole = c["command"] if second is c["command"] else np.concatenate([np.tile(c["command"], (5, 1, 1)), np.tile(c1, (7, 1, 1))])
        w = run(c["x"], c["feet"], c["stamp"], whole, steps, c["push"])
        for k in ("x", "feet"):
            assert np.array_equal(_bits(np.concatenate([a[k], b[k][1:]])), _bits(w[k])), k
        for k in ("u0", "status", "iters"):
            assert np.array_equal(_bits(np.concatenate([a[k], b[k]])), _bits(w[k])), k
        assert np.array_equal(b["alive"], w["alive"]) and np.array_equal(_bits(b["stamp"]), _bits(w["stamp"]))
    held = run(c["x"], c["feet"], c["stamp"], c["command"], steps, c["push"])
    assert np.any(held["x"][-1] != w["x"][-1]) and np.array_equal(_bits(held["x"][:6]), _bits(w["x"][:6]))


def test_free_running_against_the_twin(eng):
    """The six robots of steer_twin.fleet() over 50 steps, the engine and the twin each on its own trajectory: every robot alive on both, the iteration counts
    equal, states -- the final yaws among them -- within 1e-4."""
    T = 50
    f = stw.fleet()
    want = stw.rollout(orc.default_params(N), f["x"], f["feet"], f["stamp"], f["command"], T, ft.COM, standing=f["standing"], solver="c")
    got = eng.rollout(f["x"], f["feet"], f["stamp"], None, T, ft.COM, standing=f["standing"], command=f["command"])
    err = np.abs(got["x"] - want["x"]).max(axis=(0, 2))
    eyaw = np.abs(got["x"][T, :, 2] - want["x"][T, :, 2])
    print("free-running steered: max |x - twin| per robot", err.tolist(), "final yaw", got["x"][T, :, 2].tolist(), "against the twin's", eyaw.tolist(),
          "steps with other iters", (got["iters"] != want["iters"]).sum(axis=0).tolist())
    assert got["alive"].tolist() == [1] * 6 and want["alive"].tolist() == [1] * 6
    assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["status"], want["status"])
    assert err.max() < 1e-4, err
    assert eyaw.max() < 1e-4, eyaw


def test_without_a_command_the_rollout_is_what_it_was(eng):
    """rollout(v_ref) with command=None against the unsteered C calls in the same process: bit for bit; and command= beside v_ref is a ValueError."""
    steps, B = 9, 21
    c = crowd("commanded", B, 17, steps)
    v_ref = c["command"][:, 0:2].copy()
    c["x"][:, 2] = 0.0
    got = eng.rollout(c["x"], c["feet"], c["stamp"], v_ref, steps, ft.COM, standing=c["standing"], push=c["push"], command=None)
    want = direct_rollout(eng, "srbdqp_fleet_rollout_f64", c, steps, v_ref)
    for k, v in want.items():
        assert np.array_equal(_bits(got[k]), _bits(v)), k
    with pytest.raises(ValueError, match="command"):
        eng.rollout(c["x"], c["feet"], c["stamp"], v_ref, steps, ft.COM, command=c["command"])


def test_refusals_and_a_command_that_is_not_finite(eng):
    import torch
    from g1_locomotion_amd import SrbdqpError
    steps = 3
    c = crowd("commanded", B77, 23, steps)
    c["feet"] = turned_feet(c)
    c["standing"][:] = 0
    run = lambda cmd, **k: eng.rollout(c["x"], c["feet"], c["stamp"], None, steps, ft.COM, command=cmd, **k)
    # the host forms refuse a command that is not finite, by robot
    bad = c["command"].copy()
    bad[3, 2] = np.nan
    with pytest.raises(SrbdqpError, match="robot 3.*not finite"):
        run(bad)
    with pytest.raises(SrbdqpError, match="robot 3.*not finite"):
        eng.mpc_inputs_steered(c["x"], c["feet"], c["stamp"], bad, ft.COM)
    # command_steps outside {1, T}, a NULL command
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x, feet, stamp, cm = up(c["x"]), up(c["feet"]), up(c["stamp"]), up(c["command"])
    torch.cuda.synchronize()                                      # (fleet_loop.py's stream rule)
    for cs in (0, 2, steps + 1):
        with pytest.raises(SrbdqpError, match="command_steps"):
            eng.rollout_device(B77, steps, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), 0, ft.COM, command=cm.data_ptr(), command_steps=cs)
    v = lambda q: C.c_void_p(int(q))
    s = eng.fleet_settings(ft.COM)
    assert eng._lib.srbdqp_fleet_rollout_steered_device_f64(eng._h, B77, steps, v(x.data_ptr()), v(feet.data_ptr()), v(stamp.data_ptr()), None, 1, None, None, C.byref(s),
                                                            *([None] * 10)) == -1
    assert "command is NULL" in eng._lib.srbdqp_last_error(eng._h).decode()
    # ... and what the roll-out it becomes refuses: a wrench set on the engine, bad settings, an observed roll-out on a map
    eng.set_external_wrench(np.full((B77, N, 6), 0.5))
    try:
        with pytest.raises(SrbdqpError, match="srbdqp_set_external_wrench"):
            run(c["command"])
    finally:
        eng.set_external_wrench(None)
    with pytest.raises(SrbdqpError, match="srbdqp_fleet_settings"):
        run(c["command"], substeps=0)
    eng.set_terrain(np.zeros((4, 5)), origin=(-2.0, -2.0), cell=1.5)
    try:
        with pytest.raises(SrbdqpError, match="terrain"):
            run(c["command"], observer=True)
    finally:
        eng.set_terrain(None)
    eng.synchronize()
    assert np.array_equal(x.cpu().numpy(), c["x"]) and np.array_equal(stamp.cpu().numpy(), c["stamp"])          # nothing was launched on the refused calls
    # the device form: a NaN yaw rate for robot 3 of 77 -- it ends with status -1 and zero forces at every step, the other 76 as in a run without it
    al = up(np.ones(B77, np.uint8))
    bm = up(bad)
    ul = torch.full((steps, B77, 12), -7.0, dtype=torch.float64, device=dev)
    xl = torch.full((steps + 1, B77, 13), -7.0, dtype=torch.float64, device=dev)
    sl = torch.zeros((steps, B77), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()                                      # (fleet_loop.py's stream rule)
    eng.rollout_device(B77, steps, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), 0, ft.COM, alive=al.data_ptr(), x_log=xl.data_ptr(), u0_log=ul.data_ptr(),
                       status_log=sl.data_ptr(), command=bm.data_ptr(), command_steps=1)
    eng.synchronize()
    good = run(c["command"])
    ul, xl, sl = ul.cpu().numpy(), xl.cpu().numpy(), sl.cpu().numpy()
    assert np.all(sl[:, 3] == -1) and np.all(ul[:, 3] == 0.0)
    rest = np.arange(B77) != 3
    assert np.array_equal(_bits(ul[:, rest]), _bits(good["u0"][:, rest])) and np.array_equal(_bits(xl[:, rest]), _bits(good["x"][:, rest]))
    assert np.array_equal(sl[:, rest], good["status"][:, rest])
