"""GPU tests of the fleet roll-out (include/srbdqp_cascade.h srbdqp_fleet_advance_* / srbdqp_fleet_rollout_*), N = 10, against the NumPy
twin of tests/fleet_twin.py (tests/test_fleet_cpu.py holds the twin itself).

Bounds: the plant in float64 against the SAME scheme in long double differs by 2.2e-13 over a period on such inputs -- that is its rounding error, not its
accuracy: against the rigid body itself ten RK4 substeps are 1e-4 to 1e-6 away (tests/test_plant_reference_cpu.py, tests/test_gpu_plant_reference.py;
DESIGN.md section 17 has the table).  1e-9 absolute on states, kernel against twin, is the project's bound for wbid_reference.  Forces: 2e-3 N, the solver tolerance of the parity suites.  Free-running trajectories: 1e-4, the bound of
test_closed_loop_gpu_engine_stands_and_steps at its length (50 steps)."""
import numpy as np
import pytest

import c_oracle  # noqa: F401
import cascade_oracle as co
import srbd_oracle as orc
import fleet_twin as ft
from fleet_loop import _bits, _stamps, crowd, device_loop

pytestmark = pytest.mark.gpu
N, DT, T = 10, 0.04, 50


@pytest.fixture(scope="module")
def eng():
    import torch  # noqa: F401
    from g1_locomotion_amd import BatchMPC
    e = BatchMPC(horizon=N)
    yield e
    e.close()


@pytest.fixture(scope="module")
def twin():
    """The 6-robot fleet on the C oracle, T steps: computed once, read by every test that needs it."""
    f = ft.fleet()
    r = ft.rollout(orc.default_params(N), f["x"], f["feet"], f["stamp"], f["v_ref"], T, ft.COM, standing=f["standing"], push=ft.fleet_push(T, 6), solver="c")
    for v in r.values():
        v.setflags(write=False)
    return f, r


@pytest.fixture(scope="module")
def gpu(eng):
    """... and on the engine, through host buffers."""
    f = ft.fleet()
    return eng.rollout(f["x"], f["feet"], f["stamp"], f["v_ref"], T, ft.COM, standing=f["standing"], push=ft.fleet_push(T, 6))


def test_fleet_advance_against_the_twin(eng, twin):
    """One period of 77 robots (a tile of 64 and a remainder of 13) on states, footholds, forces and landing points of the twin's roll-out, tilted by up to
    0.3 rad more, some of them at a touchdown, some dead, under random pushes: stamps, footholds, alive flags bit for bit, states within 1e-9 -- with the
    config's robot, with robot records, and with thresholds under which some of them fall."""
    from g1_locomotion_amd.mpc import robots_array
    f, r = twin
    rng = np.random.default_rng(3)
    B = 77
    t, b = rng.integers(0, T, B), rng.integers(0, 6, B)
    stamps = _stamps(f["stamp"], T)
    x, feet, u0, landing, stamp = r["x"][t, b].copy(), r["feet"][t, b].copy(), r["u0"][t, b].copy(), r["landing"][t, b].copy(), stamps[t, b].copy()
    x[:, 0:2] += rng.uniform(-0.3, 0.3, (B, 2))
    x[:, 6:12] += rng.normal(size=(B, 6)) * 0.05
    assert np.abs(x[:, 0:2]).max() < 0.5
    standing = f["standing"][b]
    push = rng.uniform(-1.0, 1.0, (B, 6)) * np.array([3.0, 3.0, 3.0, 30.0, 30.0, 30.0])
    alive = (rng.random(B) > 0.15).astype(np.uint8)
    p = orc.default_params(N)
    rec = robots_array(B, mass=rng.uniform(25.0, 45.0, B), inertia=np.array(p.inertia) * rng.uniform(0.7, 1.5, (B, 3)))
    for robots, settings in ((None, {}), (rec, {}), (None, dict(tilt_max=0.2, z_min=0.59, substeps=7, foot_half_length=0.06))):
        want = ft.advance(p, x, feet, stamp, u0, landing, standing=standing, push=push, alive=alive, robots=robots, **settings)
        eng.set_robots(robots)
        try:
            got = eng.fleet_advance(x, feet, stamp, u0, landing, standing=standing, push=push, alive=alive, **settings)
        finally:
            eng.set_robots(None)
        assert eng.kernel_name() == "fleet_advance_f64"
        if not settings:
            assert {1, 2} <= set(want["moved"].tolist()) and (want["moved"] == 0).sum() > 20 and 0 < (alive == 0).sum() < B // 2
        else:
            assert 0 < (want["alive"][alive == 1] == 0).sum() < (alive == 1).sum()          # some fall in this period, some do not
        moved = np.where(np.any(got["feet"][:, 0:6] != feet[:, 0:6], axis=1), 1, np.where(np.any(got["feet"][:, 6:12] != feet[:, 6:12], axis=1), 2, 0))
        assert np.array_equal(moved, want["moved"])
        assert np.array_equal(_bits(got["stamp"]), _bits(want["stamp"])) and np.array_equal(_bits(got["feet"]), _bits(want["feet"]))
        assert np.array_equal(got["alive"], want["alive"])
        err = np.abs(got["x"] - want["x"]).max()
        print("fleet_advance against the twin, robots" if robots is not None else "fleet_advance against the twin", settings, err)
        assert err < 1e-9, err
        dead = alive == 0
        assert np.array_equal(_bits(got["x"][dead]), _bits(x[dead])) and np.array_equal(_bits(got["feet"][dead]), _bits(feet[dead]))


@pytest.mark.parametrize("B,defer", [(33, False), (1, False), (33, True)])
def test_the_loop_is_the_public_calls(B, defer):
    """rollout_device() over 14 steps against mpc_inputs_device -> solve_device(pcom=) -> fleet_advance_device driven step by step on the same engine: every log
    and every final array bit for bit; once on a SRBDQP_FLAG_DEFER_TAIL engine, where a flush follows every solve."""
    import torch  # noqa: F401
    from g1_locomotion_amd import BatchMPC, _lib
    steps = 14
    c = crowd("v_ref", B, 40 + B, steps)
    with BatchMPC(horizon=N, **(dict(flags=_lib.FLAG_DEFER_TAIL) if defer else {})) as e:
        call, loop, _ = device_loop(e, c, B, steps, defer=defer)
    for k in call:
        assert np.array_equal(_bits(call[k]), _bits(loop[k])), k
    assert np.array_equal(_bits(call["x_log"][-1]), _bits(call["x"])) and np.array_equal(_bits(call["x_log"][0]), _bits(c["x"]))
    assert (call["status_log"] == 1).mean() > 0.9 and np.any(call["feet_log"][-1] != call["feet_log"][0]) == (not c["standing"].all())
    if B > 4:                                                            # the robot that came in dead held, and its clock ran
        assert np.array_equal(_bits(call["x_log"][:, 3]), _bits(np.tile(c["x"][3], (steps + 1, 1)))) and call["alive"][3] == 0
        assert call["stamp"][3] == _stamps(c["stamp"], steps)[-1, 3]


def test_chunks_compose(eng):
    """rollout(9) and rollout(16) from where it ended = rollout(25), bit for bit."""
    c = crowd("v_ref", 21, 7, 25)
    a = eng.rollout(c["x"], c["feet"], c["stamp"], c["v_ref"], 9, ft.COM, standing=c["standing"], push=c["push"][:9])
    b = eng.rollout(a["x"][-1], a["feet"][-1], a["stamp"], c["v_ref"], 16, ft.COM, standing=c["standing"], push=c["push"][9:], alive=a["alive"])
    w = eng.rollout(c["x"], c["feet"], c["stamp"], c["v_ref"], 25, ft.COM, standing=c["standing"], push=c["push"])
    for k in ("x", "feet"):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k][1:]])), _bits(w[k])), k
    for k in ("u0", "status", "iters"):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k]])), _bits(w[k])), k
    assert np.array_equal(b["alive"], w["alive"]) and np.array_equal(_bits(b["stamp"]), _bits(w["stamp"]))


def test_teacher_forced_parity_over_a_whole_rollout(gpu, twin):
    """Every step of the engine's 50-step roll-out of the 6-robot fleet, taken on its own: from the engine's x_log[t], feet_log[t] and u0_log[t] the twin's
    advance gives x_log[t + 1] within 1e-9 and feet_log[t + 1] bit for bit, and the twin's solve on x_log[t] ends with the engine's status and within 2e-3 N of
    u0_log[t]."""
    f, _ = twin
    p = orc.default_params(N)
    B = 6
    flat = lambda a: a.reshape((T * B,) + a.shape[2:])
    x, feet = flat(gpu["x"][:-1]), flat(gpu["feet"][:-1])
    stamp = flat(_stamps(f["stamp"], T)[:-1])
    rep = lambda a: np.tile(a, (T,) + (1,) * (a.ndim - 1))
    standing, v_ref = rep(f["standing"]), rep(f["v_ref"])
    inp = co.mpc_inputs(x, feet, stamp, v_ref, ft.COM, N, DT, standing=standing)
    sol = ft.solve(p, x, inp, "c")
    assert np.array_equal(sol["status"], flat(gpu["status"])) and np.all(sol["status"] == 1)
    du = np.abs(sol["u0"] - flat(gpu["u0"])).max()
    nxt = ft.advance(p, x, feet, stamp, flat(gpu["u0"]), inp["landing"], standing=standing, push=flat(ft.fleet_push(T, B)))
    dx = np.abs(nxt["x"] - flat(gpu["x"][1:])).max()
    print("teacher-forced: forces", du, "N, states", dx)
    assert du < 2e-3, du
    assert dx < 1e-9, dx
    assert np.array_equal(_bits(nxt["feet"]), _bits(flat(gpu["feet"][1:])))
    assert np.array_equal(_bits(gpu["stamp"]), _bits(_stamps(f["stamp"], T)[-1])) and gpu["alive"].tolist() == [1] * B


def test_free_running_parity(gpu, twin):
    """The engine's roll-out beside the twin's, each on its own trajectory: a robot whose solves ended with the twin's status and iteration count at every step
    stays within 1e-4 of the twin's trajectory; at least 5 of the 6 do (the two CPU oracles qualify all 6 against each other); none falls."""
    _, r = twin
    same = np.all(gpu["status"] == r["status"], axis=0) & np.all(gpu["iters"] == r["iters"], axis=0)
    err = np.abs(gpu["x"] - r["x"]).max(axis=(0, 2))
    print("free-running: qualified", same.tolist(), "max |x - twin| per robot", err.tolist(), "steps with other iters", (gpu["iters"] != r["iters"]).sum(axis=0).tolist())
    assert gpu["alive"].tolist() == [1] * 6 and gpu["x"][:, :, 5].min() > 0.45 and np.abs(gpu["x"][:, :, 0:2]).max() < 0.5
    assert same.sum() >= 5, same
    assert err[same].max() < 1e-4, err


def test_fallen_non_finite_and_refusals(eng):
    import torch
    from g1_locomotion_amd import SrbdqpError
    f = ft.fleet()
    steps = 8
    args = lambda d: (d["x"], d["feet"], d["stamp"], d["v_ref"], steps, ft.COM)
    # a solve before anything else, to be repeated at the end
    x0, xr, fo, ct = orc.synthetic_batch(16, N, seed=21, schedule="single")
    before = eng.solve(x0, xr, fo, ct)
    base = eng.rollout(*args(f), standing=f["standing"])
    # a robot handed over on its side (roll 1.2 > tilt_max = 1.0) has fallen: it gets its first period -- in which this MPC turns it back to 0.905 rad, measured
    # on every robot of this fleet -- and holds from then on (include/srbdqp_cascade.h, step 5: the envelope is tested on the state a period starts from too)
    g = {k: v.copy() for k, v in f.items()}
    g["x"][2, 0] = 1.2
    r = eng.rollout(*args(g), standing=g["standing"])
    assert r["alive"].tolist() == [1, 1, 0, 1, 1, 1]
    assert np.any(r["x"][1, 2] != r["x"][0, 2])
    assert np.array_equal(_bits(r["x"][1:, 2]), _bits(np.tile(r["x"][1, 2], (steps, 1)))) and np.array_equal(_bits(r["feet"][1:, 2]), _bits(np.tile(r["feet"][1, 2], (steps, 1))))
    others = [0, 1, 3, 4, 5]
    assert np.array_equal(_bits(r["x"][:, others]), _bits(base["x"][:, others]))
    # a NaN in x0: dead at once, arrays untouched, the neighbours as in a run without that robot
    g = {k: v.copy() for k, v in f.items()}
    g["x"][4, 7] = np.nan
    r = eng.rollout(*args(g), standing=g["standing"])
    assert r["alive"].tolist() == [1, 1, 1, 1, 0, 1]
    assert np.array_equal(_bits(r["x"][:, 4]), _bits(np.tile(g["x"][4], (steps + 1, 1)))) and np.array_equal(_bits(r["feet"][:, 4]), _bits(np.tile(g["feet"][4], (steps + 1, 1))))
    keep = [0, 1, 2, 3, 5]
    h = {k: v[keep] for k, v in f.items()}
    w = eng.rollout(*args(h), standing=h["standing"])
    for k in ("x", "feet", "u0", "status", "iters"):
        assert np.array_equal(_bits(r[k][:, keep]), _bits(w[k])), k
    # a handle whose QPs know a wrench or a slope the plant does not: refused by the setter's name, nothing written
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for setter, value in (("set_external_wrench", np.full((6, N, 6), 0.5)), ("set_contact_normals", np.tile([0.0, 0.0, 1.0], (6, N, 4)))):
        getattr(eng, setter)(value)
        try:
            x, feet, stamp, v = up(f["x"]), up(f["feet"]), up(f["stamp"]), up(f["v_ref"])
            xl = torch.full((steps + 1, 6, 13), -7.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()                                 # (fleet_loop.py's stream rule)
            with pytest.raises(SrbdqpError, match="srbdqp_" + setter):
                eng.rollout_device(6, steps, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), v.data_ptr(), ft.COM, x_log=xl.data_ptr())
            eng.synchronize()
            assert torch.all(xl == -7.0) and np.array_equal(x.cpu().numpy(), f["x"]) and np.array_equal(stamp.cpu().numpy(), f["stamp"])
            with pytest.raises(SrbdqpError, match="srbdqp_" + setter):
                eng.rollout(*args(f))
        finally:
            getattr(eng, setter)(None)
    # bad arguments: no launch
    for bad in (dict(substeps=0), dict(z_min=float("nan")), dict(tilt_max=-1.0), dict(foot_half_length=0.0), dict(period_steps=0)):
        with pytest.raises(SrbdqpError, match="srbdqp_fleet_settings"):
            eng.rollout(*args(f), **bad)
    with pytest.raises(SrbdqpError):
        eng.rollout(f["x"], f["feet"], f["stamp"], f["v_ref"], 0, ft.COM)
    # the handle is what it was: the same solve, the same answer
    after = eng.solve(x0, xr, fo, ct)
    for k in ("u", "x", "status", "iters"):
        assert np.array_equal(_bits(after[k]), _bits(before[k])), k
