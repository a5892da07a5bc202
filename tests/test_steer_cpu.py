"""CPU side of the steered fleet calls (include/srbdqp_cascade.h srbdqp_mpc_inputs_steered_*, srbdqp_fleet_advance_steered_*, srbdqp_fleet_rollout_steered_*;
DESIGN.md section 20): the library exports the calls and the binding lists them, the refusals that need no device, the twin of tests/steer_twin.py against what
exists where the command does not turn, its geometry, its behaviour over 150 steps on the C oracle, command schedules, and a stand-alone host build of
csrc/srbdqp_steer.hpp against the twin.

The behaviour's bars are the issue's: every robot alive, every QP SOLVED, |roll| and |pitch| at most 0.1, the yaw reached within 20 % of the commanded wz T dt
where wz is not 0, and below 0.02 rad for the straight walker."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import cascade_oracle as co
import fleet_twin as ft
import srbd_oracle as orc
import steer_twin as stw

CALLS = ("srbdqp_mpc_inputs_steered_f64", "srbdqp_mpc_inputs_steered_device_f64", "srbdqp_fleet_advance_steered_f64", "srbdqp_fleet_advance_steered_device_f64",
         "srbdqp_fleet_rollout_steered_device_f64", "srbdqp_fleet_rollout_steered_f64")
N, DT, T = 10, 0.04, 150
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_the_library_exports_the_steered_calls_and_the_binding_lists_them(built_lib):
    from g1_locomotion_amd import _lib, BatchMPC
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in CALLS:
        assert f" T {name}\n" in syms, name
        assert name in _lib.SIGNATURES and getattr(built_lib, name).restype is C.c_int
    for method in ("mpc_inputs_steered", "mpc_inputs_steered_device"):
        assert callable(getattr(BatchMPC, method))
    assert "landing_yaw" in inspect.signature(BatchMPC.fleet_advance).parameters and "landing_yaw" in inspect.signature(BatchMPC.fleet_advance_device).parameters
    assert "command" in inspect.signature(BatchMPC.rollout).parameters
    assert {"command", "command_steps"} <= set(inspect.signature(BatchMPC.rollout_device).parameters)


def test_refusals_that_need_no_device(built_lib):
    """A NULL handle is refused, not dereferenced; command_steps outside {1, T}, a NULL command and -- in the host forms -- a command that is not finite are
    refused before the handle is looked at, by name (srbdqp_last_error(NULL))."""
    from g1_locomotion_amd import _lib
    lib = built_lib
    why = lambda: lib.srbdqp_last_error(None).decode()
    B, steps = 4, 5
    good = np.tile([0.2, 0.0, 0.3], (steps, B, 1))
    assert lib.srbdqp_mpc_inputs_steered_f64(None, B, *([None] * 3), _p(good), *([None] * 8)) == _lib.E_INVALID
    assert lib.srbdqp_mpc_inputs_steered_device_f64(None, B, *([None] * 13)) == _lib.E_INVALID
    assert lib.srbdqp_fleet_advance_steered_f64(None, B, *([None] * 4), 12, *([None] * 6)) == _lib.E_INVALID
    assert lib.srbdqp_fleet_advance_steered_device_f64(None, B, *([None] * 4), 12, *([None] * 7)) == _lib.E_INVALID
    roll = lambda fn, cmd, cs, *tail: fn(None, B, steps, None, None, None, cmd, cs, *([None] * 12), *tail)
    for fn, tail in ((lib.srbdqp_fleet_rollout_steered_f64, ()), (lib.srbdqp_fleet_rollout_steered_device_f64, (None,))):
        assert roll(fn, _p(good), 1, *tail) == _lib.E_INVALID and roll(fn, _p(good), steps, *tail) == _lib.E_INVALID
        for cs in (0, 2, steps + 1, -1):
            assert roll(fn, _p(good), cs, *tail) == _lib.E_INVALID and "command_steps" in why(), cs
        assert roll(fn, None, 1, *tail) == _lib.E_INVALID and "command is NULL" in why()
    for bad in (np.nan, np.inf, -np.inf):
        for cs in (1, steps):
            cmd = good.copy()
            cmd[cs - 1, 2, 2] = bad
            assert roll(lib.srbdqp_fleet_rollout_steered_f64, _p(cmd), cs) == _lib.E_INVALID and "not finite" in why() and "robot 2" in why(), (bad, cs)
        cmd = good[0].copy()
        cmd[3, 0] = bad
        assert lib.srbdqp_mpc_inputs_steered_f64(None, B, *([None] * 3), _p(cmd), *([None] * 8)) == _lib.E_INVALID and "not finite" in why() and "robot 3" in why()


def _draw(B, seed, psi0=None):
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 13)); x[:, 3:6] = ft.COM + rng.normal(size=(B, 3)) * 0.01; x[:, 0:2] = rng.normal(size=(B, 2)) * 0.02; x[:, 12] = -9.80665
    x[:, 2] = rng.uniform(-3.0, 3.0, B) if psi0 is None else psi0
    x[:, 6:12] = rng.normal(size=(B, 6)) * 0.05
    feet = np.tile(ft.FEET.reshape(12), (B, 1)) + rng.normal(size=(B, 12)) * 0.01
    stamp = DT * (np.arange(B) % 12).astype(np.float64)          # every phase of the gait's 12 steps, so that both feet touch down somewhere
    standing = (rng.random(B) < 0.2).astype(np.uint8)
    return x, feet, stamp, standing


def test_without_a_turn_the_twin_is_what_exists():
    """wz = 0 at yaw 0: under a zero velocity every output equals cascade_oracle.mpc_inputs'; under a velocity the contacts are equal and x_ref, pcom and landing
    agree to 1e-14 (the positions are a serial sum here and a product there); the touchdown at heading 0 is fleet_twin.advance's."""
    B = 24
    x, feet, stamp, standing = _draw(B, 1, psi0=0.0)
    zero = np.zeros((B, 3))
    a, b = stw.mpc_inputs(x, feet, stamp, zero, ft.COM, N, DT, standing=standing), co.mpc_inputs(x, feet, stamp, zero[:, :2], ft.COM, N, DT, standing=standing)
    for k in ("x_ref", "foot", "contact", "pcom", "landing"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["landing_yaw"], np.zeros(B))
    cmd = np.zeros((B, 3)); cmd[:, 0:2] = np.random.default_rng(2).uniform(-0.3, 0.3, (B, 2))
    a, b = stw.mpc_inputs(x, feet, stamp, cmd, ft.COM, N, DT, standing=standing), co.mpc_inputs(x, feet, stamp, cmd[:, :2], ft.COM, N, DT, standing=standing)
    assert np.array_equal(a["contact"], b["contact"]) and np.array_equal(a["foot"], b["foot"])
    for k in ("x_ref", "pcom", "landing"):
        err = np.abs(a[k] - b[k]).max()
        assert err <= 1e-14, (k, err)
    p = orc.default_params(N)
    u0 = np.tile([0.0, 0.0, p.mass * 9.80665 / 4.0], (B, 4))
    r0 = ft.advance(p, x, feet, stamp, u0, b["landing"], standing=standing)
    r1 = stw.advance(p, x, feet, stamp, u0, b["landing"], np.zeros(B), standing=standing)
    assert {1, 2} <= set(r0["moved"].tolist())
    for k in ("x", "feet", "stamp", "alive", "moved"):
        assert np.array_equal(_bits(r0[k]), _bits(r1[k])), k


def test_geometry():
    # the arc: under (v, wz) the reference walks a circle of radius |v| / |wz|; over the angle wz N dt its chord is 2 r sin(|wz| N dt / 2).  The sum is the
    # midpoint rule on the integral of v_w(psi0 + wz t) over [0, N dt] with steps of dt, whose error is at most (N dt) dt^2 / 24 max |v_w''| = (N dt) dt^2 / 24 |v| wz^2
    # in norm (|v_w''| = |v| wz^2 at every t); 4e-15 on top for the roundings of N sums of values below 1
    psi0, wz, v = 0.7, 0.9, np.array([0.3, -0.1])
    x = np.zeros((1, 13)); x[0, 2] = psi0; x[0, 3:6] = ft.COM
    inp = stw.mpc_inputs(x, np.tile(ft.FEET.reshape(12), (1, 1)), np.zeros(1), np.array([[v[0], v[1], wz]]), ft.COM, N, DT)
    speed = np.hypot(*v)
    chord = 2.0 * (speed / abs(wz)) * np.sin(abs(wz) * N * DT / 2.0)
    got = np.hypot(*(inp["x_ref"][0, N - 1, 3:5] - inp["pcom"][0, 0, 0:2]))
    bound = (N * DT) * DT ** 2 / 24.0 * speed * wz ** 2 + 4e-15
    print("chord of the arc", chord, "the reference's", got, "difference", abs(got - chord), "bound", bound)
    assert abs(got - chord) <= bound and abs(got - chord) > 0.0
    assert np.array_equal(inp["pcom"][0, 0, 0:2], x[0, 3:5]) and np.array_equal(inp["pcom"][0, 1:, 0:2], inp["x_ref"][0, :-1, 3:5])
    # heel -> toe: length 2 foot_half_length, direction psi_L; the hip offset: perpendicular to the heading at mid-swing, on the swing foot's side
    B = 16
    xs, feet, stamp, _ = _draw(B, 5)
    cmd = np.random.default_rng(6).uniform(-1.0, 1.0, (B, 3)) * np.array([0.3, 0.1, 1.0])
    inp = stw.mpc_inputs(xs, feet, stamp, cmd, ft.COM, N, DT)
    half = 0.085
    heel, toe = stw.touchdown(inp["landing"], inp["landing_yaw"], half)
    d = toe - heel
    head = np.stack([np.cos(inp["landing_yaw"]), np.sin(inp["landing_yaw"])], axis=1)
    # (bars: a dozen roundings, 2.2e-16 each, of values below 2)
    assert np.abs(np.hypot(d[:, 0], d[:, 1]) - 2.0 * half).max() < 5e-15 and np.all(d[:, 2] == 0.0)
    assert np.abs(d[:, 0:2] / (2.0 * half) - head).max() < 5e-15
    assert np.array_equal(inp["landing_yaw"], xs[:, 2] + cmd[:, 2] * (0.5 * (6 * DT)))
    vw0 = np.stack(stw.rotate(xs[:, 2], cmd[:, 0], cmd[:, 1]), axis=1)
    off = inp["landing"][:, 0:2] - xs[:, 3:5] - 0.5 * (6 * DT) * xs[:, 9:11] - 0.03 * (xs[:, 9:11] - vw0)
    side = np.where(inp["contact"][:, 0, 0] == 0, 1.0, -1.0)
    assert np.abs((off * head).sum(1)).max() < 5e-15                                  # no component along the heading
    assert np.abs((head[:, 0] * off[:, 1] - head[:, 1] * off[:, 0]) - side * 0.0645).max() < 5e-15    # ... and side hip_offset_y to its left


@pytest.fixture(scope="module")
def walk():
    f = stw.fleet()
    return f, stw.rollout(orc.default_params(N), f["x"], f["feet"], f["stamp"], f["command"], T, ft.COM, standing=f["standing"], solver="c")


def test_six_robots_steer_on_the_twin(walk):
    f, r = walk
    wz = f["command"][:, 2]
    yaw, want = r["x"][T, :, 2], wz * (T * DT)
    tilt = np.abs(r["x"][:, :, 0:2]).max()
    print("yaw reached", yaw.tolist(), "commanded", want.tolist(), "relative", (np.abs(yaw - want)[wz != 0] / np.abs(want[wz != 0])).tolist(), "largest tilt", tilt,
          "iterations", int(r["iters"].min()), int(r["iters"].max()))
    assert r["alive"].tolist() == [1] * 6
    assert np.all(r["status"] == orc.STATUS_SOLVED)
    assert tilt <= 0.1, tilt
    turn = wz != 0.0
    assert np.all(np.abs(yaw - want)[turn] <= 0.2 * np.abs(want[turn])), (yaw, want)
    assert np.all(np.abs(yaw[~turn]) <= 0.02), yaw
    # the feet followed: the last foothold of every turning robot lies along its heading when it landed
    d = r["feet"][T, :, 3:5] - r["feet"][T, :, 0:2]
    assert np.abs(np.hypot(d[:, 0], d[:, 1]) - 0.17).max() < 1e-12 and np.ptp(np.arctan2(d[:, 1], d[:, 0])) > 1.0


def test_a_schedule_is_its_constant_chunks():
    """A (T, B, 3) schedule that switches wz at step 40 = a call of 40 steps under the first command and one of 20 under the second, bit for bit."""
    f = stw.fleet()
    p = orc.default_params(N)
    c0, c1 = f["command"].copy(), f["command"].copy()
    c1[:, 2] = -c0[:, 2] + 0.2
    steps = 60
    sched = np.concatenate([np.tile(c0, (40, 1, 1)), np.tile(c1, (steps - 40, 1, 1))])
    w = stw.rollout(p, f["x"], f["feet"], f["stamp"], sched, steps, ft.COM)
    a = stw.rollout(p, f["x"], f["feet"], f["stamp"], c0, 40, ft.COM)
    b = stw.rollout(p, a["x"][-1], a["feet"][-1], a["stamp"], c1, steps - 40, ft.COM, alive=a["alive"])
    for k in ("x", "feet"):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k][1:]])), _bits(w[k])), k
    for k in ("u0", "status", "iters", "landing_yaw"):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k]])), _bits(w[k])), k
    assert np.array_equal(b["alive"], w["alive"]) and np.array_equal(_bits(b["stamp"]), _bits(w["stamp"]))
    assert np.any(w["x"][-1, :, 2] != stw.rollout(p, f["x"], f["feet"], f["stamp"], c0, steps, ft.COM)["x"][-1, :, 2])


def _host_program(tmp_path):
    """The stand-alone program of tests/steer_host_main.cpp, built with the host compiler: with the address and undefined-behaviour sanitizers where the
    compiler has their runtimes, plainly where it has not."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++, c++, clang++) to build the steering's host program with")
    exe = str(tmp_path / "steer_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "g1_locomotion_amd", "csrc"), "-o", exe,
            os.path.join(ROOT, "tests", "steer_host_main.cpp")]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("horizon", [10, 24, 1])
def test_stand_alone_host_build_against_the_twin(tmp_path, horizon):
    """steer_table, steer_landing and steer_touchdown -- what the kernels call -- on eight robots at headings of up to 3 rad: 1e-12 against the twin (the C
    library's sines against NumPy's, on values of order 1)."""
    B = 8
    x, feet, stamp, _ = _draw(B, 9)
    cmd = np.random.default_rng(10).uniform(-1.0, 1.0, (B, 3)) * np.array([0.3, 0.1, 1.0])
    cmd[0] = 0.0
    inp = stw.mpc_inputs(x, feet, stamp, cmd, ft.COM, horizon, DT)
    p, v = stw.table(x[:, 2], x[:, 3:5], cmd[:, 0], cmd[:, 1], cmd[:, 2], DT, horizon)
    side = np.where(inp["contact"][:, 0, 0] == 0, 1.0, -1.0)
    half_T, half = 0.5 * (6 * DT), 0.085
    rows = [[DT, horizon, 0.0645, half_T, half, B]] + [np.concatenate([x[b], cmd[b], [side[b]]]).tolist() for b in range(B)]
    text = "\n".join(" ".join(repr(float(q)) for q in row) for row in rows) + "\n"
    out = subprocess.run([_host_program(tmp_path)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = [[float(q) for q in line.split()] for line in out.stdout.strip().splitlines()]
    assert len(lines) == B * (horizon + 2)
    heel, toe = stw.touchdown(inp["landing"], inp["landing_yaw"], half)
    worst = 0.0
    for b in range(B):
        blk = lines[b * (horizon + 2):(b + 1) * (horizon + 2)]
        tab = np.array(blk[:-1])
        worst = max(worst, np.abs(tab[:, 0:2] - p[b]).max(), np.abs(tab[:, 2:4] - v[b]).max())
        last = np.array(blk[-1])
        want = np.concatenate([inp["landing"][b, 0:2], [inp["landing_yaw"][b]], heel[b, 0:2], toe[b, 0:2]])
        worst = max(worst, np.abs(last - want).max())
    print("host build against the twin", worst)
    assert worst < 1e-12, worst
