"""CPU side of the tracked fleet calls (include/srbdqp_cascade.h srbdqp_mpc_inputs_tracked_*, srbdqp_fleet_rollout_tracked_*): the
library exports the calls and the binding lists them, the refusals that need no device, the identities of the twin of tests/track_twin.py, its behaviour over
150 steps on the C oracle -- walking, walking then stopping, pushed --, composition, and a stand-alone host build of csrc/srbdqp_steer.hpp's track_bound and
track_advance against the twin.

The behaviour's bars are the issue's: every robot alive, every QP SOLVED, |roll| and |pitch| at most 0.1, at most 0.1 m from the path the commands lead along
and 0.15 rad off its heading, the bounds never engaged; after walk-then-stop within 0.05 m and 0.01 rad of the path's end; pushed with 25 N for 20 steps, all
alive and no negative status under the default bounds.

Measured on the twin (six robots of steer_twin.fleet(), N = 10, T = 150):
  walking      tracked 0.022 0.026 0.043 0.006 0.032 0.017 m, yaw 0.089 0.076 0.013 0.003 -0.056 0.011 rad, largest lead 0.069 m and 0.170 rad, tilt 0.070
               steered 0.297 0.410 0.266 0.016 0.318 0.090 m, yaw 0.004 -0.132 -0.207 0.120 0.288 -0.202 rad
  walk, stop   tracked 0.004 0.005 0.006 0.006 0.006 0.021 m, yaw at most 4e-4 rad; steered: four of the six fall
  pushed       tracked 0.238 0.157 0.045 0.066 0.181 0.033 m, yaw at most 0.091 rad, the bounds engaged 85 times; with bounds of 1e9 robot 4 falls with a yaw
               lead beyond 3 rad; steered 0.14 - 0.90 m, yaw up to 0.79 rad"""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import fleet_twin as ft
import srbd_oracle as orc
import steer_twin as stw
import track_twin as ttw

CALLS = ("srbdqp_track_default_settings", "srbdqp_mpc_inputs_tracked_f64", "srbdqp_mpc_inputs_tracked_device_f64", "srbdqp_fleet_rollout_tracked_device_f64",
         "srbdqp_fleet_rollout_tracked_f64")
N, DT, T = 10, 0.04, 150
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _draw(B, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 13)); x[:, 3:6] = ft.COM + rng.normal(size=(B, 3)) * 0.01; x[:, 0:2] = rng.normal(size=(B, 2)) * 0.02; x[:, 12] = -9.80665
    x[:, 2] = rng.uniform(-3.0, 3.0, B)
    x[:, 6:12] = rng.normal(size=(B, 6)) * 0.05
    feet = np.tile(ft.FEET.reshape(12), (B, 1)) + rng.normal(size=(B, 12)) * 0.01
    stamp = DT * (np.arange(B) % 12).astype(np.float64)
    standing = (rng.random(B) < 0.2).astype(np.uint8)
    cmd = rng.uniform(-1.0, 1.0, (B, 3)) * np.array([0.3, 0.1, 1.0])
    return x, feet, stamp, standing, cmd


def test_the_library_exports_the_tracked_calls_and_the_binding_lists_them(built_lib):
    from g1_locomotion_amd import _lib, BatchMPC
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in CALLS:
        assert f" T {name}\n" in syms, name
        assert name in _lib.SIGNATURES and name in _lib.EXPORTS and getattr(built_lib, name).restype is C.c_int
    for method in ("mpc_inputs_tracked", "mpc_inputs_tracked_device", "track_settings"):
        assert callable(getattr(BatchMPC, method))
    assert {"track", "pose"} <= set(inspect.signature(BatchMPC.rollout).parameters)
    assert {"track", "pose", "pose_log"} <= set(inspect.signature(BatchMPC.rollout_device).parameters)
    s = _lib.TrackSettings()
    assert C.sizeof(s) == 24
    assert built_lib.srbdqp_track_default_settings(C.byref(s)) == _lib.E_INVALID          # struct_size 0: nothing written
    assert (s.lead_max, s.yaw_lead_max) == (0.0, 0.0)
    s.struct_size = C.sizeof(s)
    assert built_lib.srbdqp_track_default_settings(C.byref(s)) == _lib.OK and (s.lead_max, s.yaw_lead_max) == (0.1, 0.3)
    assert built_lib.srbdqp_track_default_settings(None) == _lib.E_INVALID


def test_refusals_that_need_no_device(built_lib):
    """A NULL handle is refused, not dereferenced; a NULL pose, a wrong struct_size, a bound that is not finite or not positive and -- in the host forms -- a
    pose or a command that is not finite are refused before the handle is looked at, by name and by robot (srbdqp_last_error(NULL))."""
    from g1_locomotion_amd import _lib
    lib = built_lib
    why = lambda: lib.srbdqp_last_error(None).decode()
    B, steps = 4, 5
    cmd = np.tile([0.2, 0.0, 0.3], (steps, B, 1))
    pose = np.zeros((B, 3))
    trk = _lib.TrackSettings(C.sizeof(_lib.TrackSettings), 0, 0.1, 0.3)
    inputs = lambda fn, c, k, po, *tail: fn(None, B, *([None] * 3), c, *([None] * 8), k, po, *tail)
    roll = lambda fn, c, cs, k, po, *tail: fn(None, B, steps, None, None, None, c, cs, *([None] * 12), k, po, None, *tail)
    forms = ((lib.srbdqp_mpc_inputs_tracked_f64, lib.srbdqp_fleet_rollout_tracked_f64, ()),
             (lib.srbdqp_mpc_inputs_tracked_device_f64, lib.srbdqp_fleet_rollout_tracked_device_f64, (None,)))
    for fin, fro, tail in forms:
        # a NULL handle with everything else in order
        assert inputs(fin, _p(cmd[0]), C.byref(trk), _p(pose), *tail) == _lib.E_INVALID
        assert roll(fro, _p(cmd), 1, C.byref(trk), _p(pose), *tail) == _lib.E_INVALID and roll(fro, _p(cmd), steps, C.byref(trk), _p(pose), *tail) == _lib.E_INVALID
        # a NULL pose
        assert inputs(fin, _p(cmd[0]), C.byref(trk), None, *tail) == _lib.E_INVALID and "pose is NULL" in why() and "srbdqp_mpc_inputs_tracked" in why()
        assert roll(fro, _p(cmd), 1, C.byref(trk), None, *tail) == _lib.E_INVALID and "pose is NULL" in why() and "srbdqp_fleet_rollout_tracked" in why()
        # the settings
        assert inputs(fin, _p(cmd[0]), None, _p(pose), *tail) == _lib.E_INVALID and "struct_size" in why()
        for size in (0, 16, 32):
            bad = _lib.TrackSettings(size, 0, 0.1, 0.3)
            assert inputs(fin, _p(cmd[0]), C.byref(bad), _p(pose), *tail) == _lib.E_INVALID and "struct_size" in why(), size
            assert roll(fro, _p(cmd), 1, C.byref(bad), _p(pose), *tail) == _lib.E_INVALID and "struct_size" in why(), size
        for v in (0.0, -0.1, np.nan, np.inf, -np.inf):
            for bad in (_lib.TrackSettings(24, 0, v, 0.3), _lib.TrackSettings(24, 0, 0.1, v)):
                assert inputs(fin, _p(cmd[0]), C.byref(bad), _p(pose), *tail) == _lib.E_INVALID and "finite and positive" in why(), v
                assert roll(fro, _p(cmd), steps, C.byref(bad), _p(pose), *tail) == _lib.E_INVALID and "finite and positive" in why(), v
        # the steered roll-out's own rules, in the tracked call's name
        assert roll(fro, None, 1, C.byref(trk), _p(pose), *tail) == _lib.E_INVALID and "command is NULL" in why() and "tracked" in why()
        for cs in (0, 2, steps + 1, -1):
            assert roll(fro, _p(cmd), cs, C.byref(trk), _p(pose), *tail) == _lib.E_INVALID and "command_steps" in why(), cs
    # the host forms: a pose or a command that is not finite, by robot
    for bad in (np.nan, np.inf, -np.inf):
        po = pose.copy(); po[2, 1] = bad
        assert inputs(lib.srbdqp_mpc_inputs_tracked_f64, _p(cmd[0]), C.byref(trk), _p(po)) == _lib.E_INVALID
        assert "pose of robot 2" in why() and "not finite" in why()
        assert roll(lib.srbdqp_fleet_rollout_tracked_f64, _p(cmd), steps, C.byref(trk), _p(po)) == _lib.E_INVALID
        assert "pose of robot 2" in why() and "not finite" in why()
        c1 = cmd[0].copy(); c1[3, 0] = bad
        assert inputs(lib.srbdqp_mpc_inputs_tracked_f64, _p(c1), C.byref(trk), _p(pose)) == _lib.E_INVALID
        assert "command of robot 3" in why() and "not finite" in why()
        for cs in (1, steps):
            c2 = cmd.copy(); c2[cs - 1, 1, 2] = bad
            assert roll(lib.srbdqp_fleet_rollout_tracked_f64, _p(c2), cs, C.byref(trk), _p(pose)) == _lib.E_INVALID
            assert "command of robot 1" in why() and "not finite" in why(), (bad, cs)


def test_track_without_a_command_is_a_value_error(built_lib):
    """rollout(track=) without command= has no path to follow: refused in Python, before any engine is needed."""
    from g1_locomotion_amd import BatchMPC
    eng = BatchMPC.__new__(BatchMPC)          # (the checks under test come before the first use of the handle)
    x = np.zeros((2, 13))
    with pytest.raises(ValueError, match="track="):
        BatchMPC.rollout(eng, x, np.zeros((2, 12)), np.zeros(2), np.zeros((2, 2)), 3, ft.COM, track=True)
    with pytest.raises(ValueError, match="track="):
        BatchMPC.rollout_device(eng, 2, 3, 1, 1, 1, 1, ft.COM, track=True, pose=1)


# ---- identities of the twin ----
def test_from_the_measured_pose_the_tracked_inputs_are_the_steered_ones():
    B = 24
    x, feet, stamp, standing, cmd = _draw(B, 1)
    assert np.all((cmd[:, 0] != 0.0) | (cmd[:, 1] != 0.0))
    a = ttw.mpc_inputs(x, feet, stamp, cmd, ttw.start_pose(x), ft.COM, N, DT, standing=standing)
    b = stw.mpc_inputs(x, feet, stamp, cmd, ft.COM, N, DT, standing=standing)
    for k in b:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    p, _ = stw.table(x[:, 2], x[:, 3:5], cmd[:, 0], cmd[:, 1], cmd[:, 2], DT, N)
    assert np.array_equal(_bits(a["pose"][:, 0:2]), _bits(p[:, 1]))
    assert np.array_equal(_bits(a["pose"][:, 2]), _bits(x[:, 2] + (cmd[:, 2] * 1.0) * DT))
    assert not a["engaged"].any()


def test_a_zero_command_holds_the_pose():
    B = 24
    x, feet, stamp, standing, _ = _draw(B, 2)
    rng = np.random.default_rng(3)
    pose = ttw.start_pose(x) + rng.uniform(-0.05, 0.05, (B, 3))
    a = ttw.mpc_inputs(x, feet, stamp, np.zeros((B, 3)), pose, ft.COM, N, DT, standing=standing)
    assert not a["engaged"].any()
    for k in range(N):
        assert np.array_equal(_bits(a["x_ref"][:, k, 3:5]), _bits(pose[:, 0:2])), k       # not com_target, which lies wherever the caller put it
        assert np.array_equal(_bits(a["x_ref"][:, k, 2]), _bits(pose[:, 2])), k
    assert np.array_equal(_bits(a["pose"]), _bits(pose))
    # ... and what belongs to where the robot is does not read the pose
    b = stw.mpc_inputs(x, feet, stamp, np.zeros((B, 3)), ft.COM, N, DT, standing=standing)
    for k in ("foot", "contact", "pcom", "landing", "landing_yaw"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_the_bound():
    B = 64
    x, _, _, _, _ = _draw(B, 4)
    rng = np.random.default_rng(5)
    lead, ylead = 0.1, 0.3
    ang, inside = rng.uniform(-np.pi, np.pi, B), ttw.start_pose(x)
    inside[:, 0] += 0.09 * np.cos(ang); inside[:, 1] += 0.09 * np.sin(ang); inside[:, 2] += rng.uniform(-0.29, 0.29, B)
    q, engaged = ttw.bound(inside, x, lead, ylead)
    assert not engaged.any() and np.array_equal(_bits(q), _bits(inside))                 # inside: untouched, bit for bit
    r = rng.uniform(0.11, 3.0, B)
    outside = ttw.start_pose(x)
    outside[:, 0] += r * np.cos(ang); outside[:, 1] += r * np.sin(ang); outside[:, 2] += np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * rng.uniform(0.31, 4.0, B)
    q, engaged = ttw.bound(outside, x, lead, ylead)
    assert engaged.all()
    d, d0 = q[:, 0:2] - x[:, 3:5], outside[:, 0:2] - x[:, 3:5]
    n = np.hypot(d[:, 0], d[:, 1])
    # at distance lead_max within 4 ulp -- of lead_max, or of the clamped coordinate where that is the larger number (its rounding is the last one taken):
    # n, s and dx s carry 1.5, 2 and 2.5 ulp of their own, the sum cx + dx s half an ulp of the coordinate, the difference and the hypot here 1.5 more
    ulp = np.spacing(np.maximum(lead, np.abs(q[:, 0:2]).max(axis=1)))
    print("clamped distance off lead_max, in ulp", (np.abs(n - lead) / ulp).max())
    assert np.all(np.abs(n - lead) <= 4 * ulp), (np.abs(n - lead) / ulp).max()
    cross = (d[:, 0] * d0[:, 1] - d[:, 1] * d0[:, 0]) / (n * np.hypot(d0[:, 0], d0[:, 1]))
    assert np.abs(cross).max() <= 1e-14 and np.all((d * d0).sum(1) > 0.0)                # along the same direction
    sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
    assert np.array_equal(_bits(q[:, 2]), _bits(np.where(sign > 0, x[:, 2] + ylead, x[:, 2] - ylead)))       # exactly psi0 +- yaw_lead_max
    # a NaN clamps nothing: in the state, in the pose
    xn = x.copy(); xn[0, 3] = np.nan; xn[1, 2] = np.nan
    q, engaged = ttw.bound(outside, xn, lead, ylead)
    assert np.array_equal(_bits(q[0, 0:2]), _bits(outside[0, 0:2])) and not engaged[0, 0] and engaged[0, 1]
    assert _bits(q[1, 2]) == _bits(outside[1, 2]) and engaged[1, 0] and not engaged[1, 1]
    pn = outside.copy(); pn[2, 1] = np.nan; pn[3, 2] = np.nan
    q, engaged = ttw.bound(pn, x, lead, ylead)
    assert np.array_equal(_bits(q[2:4]), _bits(np.stack([np.array([pn[2, 0], np.nan, q[2, 2]]), np.array([q[3, 0], q[3, 1], np.nan])])))
    assert not engaged[2, 0] and engaged[2, 1] and engaged[3, 0] and not engaged[3, 1]


def test_a_command_that_is_not_finite_costs_one_step():
    B = 6
    x, feet, stamp, standing, cmd = _draw(B, 6)
    pose = ttw.start_pose(x)
    pose[:, 0] += 0.5                                             # beyond the bound: the pose written back is the bounded one
    cmd[1, 0], cmd[2, 2], cmd[3, 1] = np.nan, np.inf, -np.inf
    a = ttw.mpc_inputs(x, feet, stamp, cmd, pose, ft.COM, N, DT, standing=standing)
    for b in (1, 2, 3):
        assert np.array_equal(_bits(a["pose"][b]), _bits(a["bounded"][b])) and not np.isfinite(a["x_ref"][b]).all()
    for b in (0, 4, 5):
        assert np.isfinite(a["pose"][b]).all() and not np.array_equal(a["pose"][b], a["bounded"][b]) and np.isfinite(a["x_ref"][b]).all()
    good = ttw.mpc_inputs(x, feet, stamp, np.where(np.isfinite(cmd), cmd, 0.0), pose, ft.COM, N, DT, standing=standing)
    for k in ("x_ref", "pose", "pcom", "landing"):
        assert np.array_equal(_bits(a[k][[0, 4, 5]]), _bits(good[k][[0, 4, 5]])), k


# ---- behaviour on the C oracle ----
@pytest.fixture(scope="module")
def fleet():
    return stw.fleet(), orc.default_params(N)


def _figures(r, ideal):
    dist = np.hypot(r["x"][-1, :, 3] - ideal[-1, :, 0], r["x"][-1, :, 4] - ideal[-1, :, 1])
    return dist, r["x"][-1, :, 2] - ideal[-1, :, 2]


def test_six_robots_follow_their_paths_on_the_twin(fleet):
    f, p = fleet
    r = ttw.rollout(p, f["x"], f["feet"], f["stamp"], f["command"], T, ft.COM, standing=f["standing"])
    s = stw.rollout(p, f["x"], f["feet"], f["stamp"], f["command"], T, ft.COM, standing=f["standing"])
    ideal = ttw.ideal_path(f["x"], f["command"], T, DT)
    dist, yaw = _figures(r, ideal)
    sdist, syaw = _figures(s, ideal)
    tilt = np.abs(r["x"][:, :, 0:2]).max()
    lead = np.hypot(r["pose_log"][:-1, :, 0] - r["x"][1:-1, :, 3], r["pose_log"][:-1, :, 1] - r["x"][1:-1, :, 4]).max()
    ylead = np.abs(r["pose_log"][:-1, :, 2] - r["x"][1:-1, :, 2]).max()
    print("tracked: distance from the path", dist.tolist(), "yaw error", yaw.tolist(), "largest tilt", tilt, "largest lead", lead, ylead,
          "bounds engaged", int(r["engaged"].sum()))
    print("steered: distance from the path", sdist.tolist(), "yaw error", syaw.tolist())
    assert r["alive"].tolist() == [1] * 6
    assert np.all(r["status"] == orc.STATUS_SOLVED)
    assert tilt <= 0.1, tilt
    assert dist.max() <= 0.1, dist
    assert np.abs(yaw).max() <= 0.15, yaw
    assert not r["engaged"].any()
    # (unbounded, the pose IS the ideal path: the same midpoint rule from the same start)
    assert np.array_equal(_bits(r["pose_log"]), _bits(ideal[1:]))


def test_walk_then_stop(fleet):
    f, p = fleet
    sched = np.concatenate([np.tile(f["command"], (100, 1, 1)), np.zeros((50, 6, 3))])
    r = ttw.rollout(p, f["x"], f["feet"], f["stamp"], sched, T, ft.COM, standing=f["standing"])
    ideal = ttw.ideal_path(f["x"], sched, T, DT)
    dist, yaw = _figures(r, ideal)
    print("walk, then stop: distance from the path's end", dist.tolist(), "yaw error", yaw.tolist())
    assert r["alive"].tolist() == [1] * 6 and np.all(r["status"] == orc.STATUS_SOLVED)
    assert dist.max() <= 0.05, dist
    assert np.abs(yaw).max() <= 0.01, yaw
    assert np.array_equal(_bits(ideal[100]), _bits(ideal[-1]))    # the path ends where the commands end


def test_pushed(fleet):
    f, p = fleet
    push = np.zeros((T, 6, 6)); push[40:60, :, 4] = 25.0
    r = ttw.rollout(p, f["x"], f["feet"], f["stamp"], f["command"], T, ft.COM, standing=f["standing"], push=push)
    ideal = ttw.ideal_path(f["x"], f["command"], T, DT)
    dist, yaw = _figures(r, ideal)
    print("pushed, default bounds: distance", dist.tolist(), "yaw error", yaw.tolist(), "bounds engaged", int(r["engaged"].sum()))
    assert r["alive"].tolist() == [1] * 6 and r["status"].min() >= 0
    # recorded, not asserted: without the bound the lead winds up
    with np.errstate(all="ignore"):
        u = ttw.rollout(p, f["x"], f["feet"], f["stamp"], f["command"], T, ft.COM, standing=f["standing"], push=push, lead_max=1e9, yaw_lead_max=1e9)
        ylead = np.nanmax(np.abs(u["pose_log"][:-1, :, 2] - u["x"][1:-1, :, 2]), axis=0)
    print("pushed, bounds of 1e9: alive", u["alive"].tolist(), "lowest status", int(u["status"].min()), "largest yaw lead per robot", ylead.tolist())


def test_a_schedule_is_its_chunks_with_the_pose_carried(fleet):
    f, p = fleet
    c0, c1 = f["command"].copy(), f["command"].copy()
    c1[:, 2] = -c0[:, 2] + 0.2
    steps = 40
    sched = np.concatenate([np.tile(c0, (25, 1, 1)), np.tile(c1, (steps - 25, 1, 1))])
    kw = dict(lead_max=0.02, yaw_lead_max=0.05)                    # tight: the bounds engage, so that the carried pose matters after a clamp too
    w = ttw.rollout(p, f["x"], f["feet"], f["stamp"], sched, steps, ft.COM, **kw)
    a = ttw.rollout(p, f["x"], f["feet"], f["stamp"], c0, 25, ft.COM, **kw)
    b = ttw.rollout(p, a["x"][-1], a["feet"][-1], a["stamp"], c1, steps - 25, ft.COM, alive=a["alive"], pose=a["pose"], **kw)
    assert w["engaged"].any()
    for k in ("x", "feet"):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k][1:]])), _bits(w[k])), k
    for k in ("u0", "status", "iters", "landing_yaw", "pose_log"):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k]])), _bits(w[k])), k
    assert np.array_equal(_bits(b["pose"]), _bits(w["pose"])) and np.array_equal(_bits(w["pose"]), _bits(w["pose_log"][-1]))
    # ... and a pose that is NOT carried gives another roll-out
    lost = ttw.rollout(p, a["x"][-1], a["feet"][-1], a["stamp"], c1, steps - 25, ft.COM, alive=a["alive"], **kw)
    assert not np.array_equal(lost["x"][-1], b["x"][-1])


# ---- the stand-alone host build ----
def _host_program(tmp_path):
    """The stand-alone program of tests/track_host_main.cpp, built with the host compiler: with the address and undefined-behaviour sanitizers where the
    compiler has their runtimes, plainly where it has not."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++, c++, clang++) to build the tracking's host program with")
    exe = str(tmp_path / "track_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "g1_locomotion_amd", "csrc"), "-o", exe,
            os.path.join(ROOT, "tests", "track_host_main.cpp")]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("horizon", [10, 24, 1])
def test_stand_alone_host_build_against_the_twin(tmp_path, horizon):
    """track_bound, steer_table from the bounded pose and track_advance -- what the kernel calls -- on sixteen robots: inside the bounds, beyond each with both
    signs of yaw, a state, a pose and a command that are not finite, a zero command.  What passes through no sine -- the bounded pose, the advanced heading, a
    zero command's positions -- to the last bit; the rest within 1e-12 (the C library's sines against NumPy's, on values of order 1)."""
    B = 16
    x, _, _, _, cmd = _draw(B, 9)
    rng = np.random.default_rng(10)
    pose = ttw.start_pose(x) + rng.uniform(-0.05, 0.05, (B, 3))
    pose[4:8, 0:2] += rng.uniform(0.2, 1.0, (4, 2)) * np.array([[1, 1], [-1, 1], [1, -1], [-1, -1]])
    pose[6:10, 2] += np.array([0.5, -0.5, 2.0, -2.0])
    cmd[0] = 0.0
    x[10, 3], x[11, 2] = np.nan, np.nan
    pose[12, 0], pose[13, 2] = np.nan, np.inf
    cmd[14, 2], cmd[15, 0] = np.nan, np.inf
    lead, ylead = 0.1, 0.3
    q, engaged = ttw.bound(pose, x, lead, ylead)
    assert engaged[4:8, 0].all() and engaged[6:10, 1].all() and not engaged[:4].any()
    with np.errstate(invalid="ignore", over="ignore"):
        p, v = stw.table(q[:, 2], q[:, 0:2], cmd[:, 0], cmd[:, 1], cmd[:, 2], DT, horizon)
        nxt = np.stack([p[:, 1, 0], p[:, 1, 1], stw.yaw(q[:, 2], cmd[:, 2], 1.0, DT)], axis=1)
    nxt = np.where(np.isfinite(nxt).all(axis=1)[:, None], nxt, q)
    rows = [[DT, horizon, lead, ylead, B]] + [np.concatenate([x[b], cmd[b], pose[b]]).tolist() for b in range(B)]
    text = "\n".join(" ".join(repr(float(w)) for w in row) for row in rows) + "\n"
    out = subprocess.run([_host_program(tmp_path)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = [[float(w) for w in line.split()] for line in out.stdout.strip().splitlines()]
    assert len(lines) == B * (horizon + 3)
    worst = 0.0
    for b in range(B):
        blk = lines[b * (horizon + 3):(b + 1) * (horizon + 3)]
        assert np.array_equal(_bits(np.array(blk[0])), _bits(q[b])), (b, blk[0], q[b])                     # the bounded pose
        tab, last = np.array(blk[1:-1]), np.array(blk[-1])
        assert np.array_equal(np.isnan(tab), np.isnan(np.concatenate([p[b], v[b]], axis=1))), b
        assert np.array_equal(np.isnan(last), np.isnan(nxt[b])), b
        assert _bits(last[2:3]) == _bits(nxt[b, 2:3]) or (np.isnan(last[2]) and np.isnan(nxt[b, 2])), b    # the heading behind the step
        if b == 0:
            assert np.array_equal(_bits(tab[:, 0:2]), _bits(p[b])) and np.array_equal(_bits(last), _bits(nxt[b]))
        with np.errstate(invalid="ignore"):
            err = np.concatenate([(tab[:, 0:2] - p[b]).ravel(), (tab[:, 2:4] - v[b]).ravel(), last - nxt[b]])
        err = err[np.isfinite(err)]
        worst = max(worst, np.abs(err).max() if err.size else 0.0)
    for b in (14, 15):                                            # a bad command: the pose stays where the bound left it
        assert np.array_equal(_bits(np.array(lines[(b + 1) * (horizon + 3) - 1])), _bits(q[b]))
    print("host build against the twin", worst)
    assert worst < 1e-12, worst
