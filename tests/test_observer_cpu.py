"""CPU side of the momentum observer and the observed roll-out (include/srbdqp_cascade.h srbdqp_wrench_observer_*, srbdqp_fleet_rollout_observed_*; DESIGN.md
section 19): the library exports the calls and the binding lists them, the settings struct and the refusals that need no device, the measurement of
tests/observer_twin.py against fleet_twin's plant, the filter's rules, the benefit on the twin roll-out, and a stand-alone host build of
csrc/srbdqp_observer.hpp against the twin.

The measurement's draw: 32 robots around the nominal stance at yaw 0.3, tilts of a few hundredths, body rates uniform in +-0.3 rad/s, CoM velocities in +-0.1 m/s,
forces from the CPU solve of their own QPs (so that they balance the robot, as the forces of a control loop do), pushes uniform in +-(3, 3, 0.3) N m and +-40 N.
About the vertical the draw is 0.3 N m, the scale of test_gpu_fleet's own pushes: the torso's I_z is 0.0032 kg m^2, a 3 N m yaw torque would spin it to 37 rad/s
within one period, which ten RK4 substeps do not resolve (the error of the plant, not of the observer: 1e-4 N m).  The bars: 1e-5 N m and 1e-11 N under pushes
at 10 substeps, 1e-5 without a push -- 10 x the 1.1e-6 N m and 9.1e-7, 100 x the 1.4e-13 N that the twin gave on such a draw when the observer was designed
(this draw: 6.6e-7 N m, 6.0e-14 N, 2.4e-7).

The benefit scenario: fleet_twin.fleet(), N = 10, T = 30, 10 N along x and -25 N along y from step 5 on, gain 0.5, decay 1."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cascade_oracle as co
import fleet_twin as ft
import observer_twin as ot
import side_inputs as si
import srbd_oracle as orc

CALLS = ("srbdqp_observer_default_settings", "srbdqp_wrench_observer_f64", "srbdqp_wrench_observer_device_f64", "srbdqp_fleet_rollout_observed_device_f64",
         "srbdqp_fleet_rollout_observed_f64")
N, T = 10, 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def test_the_library_exports_the_observer_calls_and_the_binding_lists_them(built_lib):
    from g1_locomotion_amd import _lib, BatchMPC
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in CALLS:
        assert f" T {name}\n" in syms, name
        assert name in _lib.SIGNATURES and getattr(built_lib, name).restype is C.c_int
    for method in ("observer_settings", "wrench_observer", "wrench_observer_device", "rollout", "rollout_device"):
        assert callable(getattr(BatchMPC, method))
    import inspect
    assert {"observer", "w_est"} <= set(inspect.signature(BatchMPC.rollout).parameters)
    assert {"observer", "w_est", "w_log"} <= set(inspect.signature(BatchMPC.rollout_device).parameters)


def test_settings_struct_defaults_and_null_handles(built_lib):
    from g1_locomotion_amd import _lib
    assert C.sizeof(_lib.ObserverSettings) == 40
    s = _lib.ObserverSettings()
    s.struct_size = C.sizeof(_lib.ObserverSettings)
    assert built_lib.srbdqp_observer_default_settings(C.byref(s)) == _lib.OK
    assert (s.struct_size, s.reserved0, s.gain, s.horizon_decay, s.torque_max, s.force_max) == (40, 0, 0.5, 1.0, 50.0, 200.0)
    # a struct of another size is refused before anything is written
    for size in (0, 32, 48):
        t = _lib.ObserverSettings()
        t.struct_size, t.gain = size, -3.0
        assert built_lib.srbdqp_observer_default_settings(C.byref(t)) == _lib.E_INVALID
        assert (t.struct_size, t.gain, t.force_max) == (size, -3.0, 0.0)
    assert built_lib.srbdqp_observer_default_settings(None) == _lib.E_INVALID
    # a null handle is refused, not dereferenced
    assert built_lib.srbdqp_wrench_observer_f64(None, 1, None, None, None, None, 12, None, C.byref(s), None, None) == _lib.E_INVALID
    assert built_lib.srbdqp_wrench_observer_device_f64(None, 1, None, None, None, None, 12, None, C.byref(s), None, None, None) == _lib.E_INVALID
    assert built_lib.srbdqp_fleet_rollout_observed_f64(None, 1, 1, *([None] * 14), C.byref(s), None, None) == _lib.E_INVALID
    assert built_lib.srbdqp_fleet_rollout_observed_device_f64(None, 1, 1, *([None] * 14), C.byref(s), None, None, None) == _lib.E_INVALID


def _draw(B, seed, push_scale):
    """The measurement's draw (module docstring) -> x, feet, stamp, u0, landing, push."""
    p = orc.default_params(N)
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 13)); x[:, 3:6] = ft.COM + rng.normal(size=(B, 3)) * 0.005; x[:, 0:2] = rng.normal(size=(B, 2)) * 0.02; x[:, 2] = 0.3
    x[:, 6:9] = rng.uniform(-0.3, 0.3, (B, 3)); x[:, 9:12] = rng.uniform(-0.1, 0.1, (B, 3)); x[:, 12] = -9.80665
    feet = np.tile(ft.FEET.reshape(12), (B, 1))
    stamp = 0.04 * rng.integers(0, 24, B).astype(np.float64)
    v_ref = rng.uniform(-0.2, 0.3, (B, 2))
    inp = co.mpc_inputs(x, feet, stamp, v_ref, ft.COM, N, p.dt)
    sol = ft.solve(p, x, inp, "c")
    assert np.all(sol["status"] == 1)
    push = rng.uniform(-1.0, 1.0, (B, 6)) * np.asarray(push_scale, np.float64)
    return p, x, feet, stamp, sol["u0"], inp["landing"], push


@pytest.mark.parametrize("pushed", [True, False])
def test_measure_recovers_the_push_of_the_twin_plant(pushed):
    B = 32
    p, x, feet, stamp, u0, landing, push = _draw(B, 11, [3.0, 3.0, 0.3, 40.0, 40.0, 40.0] if pushed else [0.0] * 6)
    r = ft.advance(p, x, feet, stamp, u0, landing, push=push, substeps=10)
    assert r["alive"].all() and np.any(r["moved"] != 0)              # (some feet touch down in this period: the measurement takes the feet before it)
    wm = np.array([ot.measure(p.mass, p.inertia, p.dt, x[b], r["x"][b], feet[b], u0[b]) for b in range(B)])
    et, ef = np.abs(wm - push)[:, 0:3].max(), np.abs(wm - push)[:, 3:6].max()
    print("measure against the applied push" if pushed else "measure without a push", et, "N m", ef, "N")
    assert et < 1e-5, et
    assert ef < (1e-11 if pushed else 1e-5), ef


def test_filter_rules():
    B = 8
    p, x, feet, stamp, u0, landing, push = _draw(B, 12, [3.0, 3.0, 0.3, 40.0, 40.0, 40.0])
    x1 = ft.advance(p, x, feet, stamp, u0, landing, push=push)["x"]
    rng = np.random.default_rng(2)
    w0 = rng.uniform(-1.0, 1.0, (B, 6)) * 5.0
    wm = np.array([ot.measure(p.mass, p.inertia, p.dt, x[b], x1[b], feet[b], u0[b]) for b in range(B)])
    # gain 1: the measurement itself, up to the two roundings of w0 + 1 (wm - w0) at magnitudes below 64 (2 x 2^-47); w_meas of observe() is measure()
    o = ot.observe(p, x, x1, feet, u0, w0, N, gain=1.0)
    wm1 = w0 + 1.0 * (wm - w0)
    assert np.abs(o["w_est"] - wm).max() < 1e-13 and np.array_equal(_bits(o["w_est"]), _bits(wm1)) and np.array_equal(_bits(o["w_meas"]), _bits(wm))
    # gain 0.5: half way, in this order of operations
    o = ot.observe(p, x, x1, feet, u0, w0, N)
    assert np.array_equal(_bits(o["w_est"]), _bits(w0 + 0.5 * (wm - w0)))
    # both clamps, each on its own components
    o = ot.observe(p, x, x1, feet, u0, w0, N, gain=1.0, torque_max=0.5, force_max=1e6)
    assert np.array_equal(_bits(o["w_est"][:, 0:3]), _bits(np.clip(wm1[:, 0:3], -0.5, 0.5))) and np.array_equal(_bits(o["w_est"][:, 3:6]), _bits(wm1[:, 3:6]))
    assert np.abs(wm[:, 0:3]).max() > 0.5
    o = ot.observe(p, x, x1, feet, u0, w0, N, gain=1.0, torque_max=1e6, force_max=7.0)
    assert np.array_equal(_bits(o["w_est"][:, 3:6]), _bits(np.clip(wm1[:, 3:6], -7.0, 7.0))) and np.array_equal(_bits(o["w_est"][:, 0:3]), _bits(wm1[:, 0:3]))
    assert np.abs(wm[:, 3:6]).max() > 7.0
    # a dead robot and robots with a NaN in either state keep their estimate; the others do not notice
    alive = np.ones(B, np.uint8); alive[1] = 0
    xa, xb = x.copy(), x1.copy()
    xa[3, 7] = np.nan; xb[5, 0] = np.inf
    o = ot.observe(p, xa, xb, feet, u0, w0, N, alive=alive, horizon_decay=0.8)
    kept = [1, 3, 5]
    rest = [b for b in range(B) if b not in kept]
    assert np.array_equal(_bits(o["w_est"][kept]), _bits(w0[kept])) and np.all(np.isnan(o["w_meas"][kept]))
    assert np.array_equal(_bits(o["w_est"][rest]), _bits((w0 + 0.5 * (wm - w0))[rest]))
    # ew[k] = w decay^k by repeated multiplication, bit for bit -- from the kept values too
    s = o["w_est"].copy()
    for k in range(N):
        assert np.array_equal(_bits(o["ew"][:, k]), _bits(s)), k
        s = s * 0.8
    assert np.array_equal(_bits(ot.observe(p, x, x1, feet, u0, w0, N)["ew"]), _bits(np.repeat((w0 + 0.5 * (wm - w0))[:, None], N, axis=1)))   # (decay 1)
    # robot records: robot b's own mass and inertia
    rec = np.zeros((B, 8)); rec[:, 0] = p.mass * rng.uniform(0.7, 1.5, B); rec[:, 1:4] = np.asarray(p.inertia) * rng.uniform(0.6, 1.6, (B, 3))
    o = ot.observe(p, x, x1, feet, u0, w0, N, robots=rec, gain=1.0)
    for b in range(B):
        assert np.array_equal(_bits(o["w_meas"][b]), _bits(ot.measure(rec[b, 0], rec[b, 1:4], p.dt, x[b], x1[b], feet[b], u0[b])))
    assert np.abs(o["w_meas"] - wm).max() > 1.0


@pytest.fixture(scope="module")
def scenario():
    """The benefit scenario on the twin: the unpushed, the blind and the observed run, each once."""
    f = ft.fleet()
    p = si.params(N)
    push = ot.sustained_push(T, 6)
    args = (p, f["x"], f["feet"], f["stamp"], f["v_ref"], T, ft.COM)
    free = ot.rollout(*args, standing=f["standing"])
    blind = ot.rollout(*args, standing=f["standing"], push=push)
    seen = ot.rollout(*args, standing=f["standing"], push=push, observer={})
    return free, blind, seen


def test_the_observed_rollout_is_pushed_less_far(scenario):
    """Every robot alive and every QP solved in both runs; on every robot the observed run is below the blind one in lateral deviation from the unpushed run at
    step T and in the largest roll."""
    free, blind, seen = scenario
    for r in (blind, seen):
        assert r["alive"].tolist() == [1] * 6 and np.all(r["status"] == 1)
    dev = lambda r: np.abs(r["x"][T, :, 4] - free["x"][T, :, 4])
    roll = lambda r: np.abs(r["x"][:, :, 0]).max(axis=0)
    print("lateral deviation at T: blind", dev(blind).tolist(), "observed", dev(seen).tolist())
    print("largest roll: blind", roll(blind).tolist(), "observed", roll(seen).tolist())
    print("mean iterations: blind", blind["iters"].mean(), "observed", seen["iters"].mean())
    print("ratios", (dev(seen) / dev(blind)).tolist(), (roll(seen) / roll(blind)).tolist())
    assert np.all(dev(seen) < dev(blind)), (dev(seen), dev(blind))
    assert np.all(roll(seen) < roll(blind)), (roll(seen), roll(blind))
    # the estimate has found the push: the force within 1 N of (10, -25, 0) at the end, w_log's last entry is w_est, and before the push it was nothing
    assert np.abs(seen["w_log"][-1][:, 3:6] - np.array([10.0, -25.0, 0.0])).max() < 1.0
    assert np.array_equal(_bits(seen["w_log"][-1]), _bits(seen["w_est"])) and np.abs(seen["w_log"][:5]).max() < 1e-4


def test_twin_rollout_without_a_push_matches_the_blind_one_closely(scenario):
    """With no push the estimate stays at the plant's integration error, and the observed roll-out's first solve -- under a zero wrench -- is the blind one's."""
    free, _, _ = scenario
    f = ft.fleet()
    seen = ot.rollout(si.params(N), f["x"], f["feet"], f["stamp"], f["v_ref"], 3, ft.COM, standing=f["standing"], observer={})
    assert np.array_equal(_bits(seen["u0"][0]), _bits(free["u0"][0]))
    assert np.abs(seen["w_log"]).max() < 1e-4 and np.abs(seen["x"] - free["x"][:4]).max() < 1e-6


def _host_program(tmp_path):
    """The stand-alone program of tests/observer_host_main.cpp, built with the host compiler: with the address and undefined-behaviour sanitizers where the
    compiler has their runtimes, plainly where it has not."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++, c++, clang++) to build the observer's host program with")
    exe = str(tmp_path / "observer_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "g1_locomotion_amd", "csrc"), "-o", exe,
            os.path.join(ROOT, "tests", "observer_host_main.cpp")]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)
    return exe


def test_stand_alone_host_build_against_the_twin(tmp_path):
    B = 6
    p, x, feet, stamp, u0, landing, push = _draw(B, 13, [3.0, 3.0, 0.3, 40.0, 40.0, 40.0])
    x1 = ft.advance(p, x, feet, stamp, u0, landing, push=push)["x"]
    w0 = np.random.default_rng(4).uniform(-1.0, 1.0, (B, 6)) * 5.0
    gain, tmax, fmax = 0.7, 1.5, 30.0
    rows = [[p.mass, *p.inertia, p.dt, gain, tmax, fmax, B]] + [np.concatenate([x[b], x1[b], feet[b], u0[b], w0[b]]).tolist() for b in range(B)]
    text = "\n".join(" ".join(repr(float(v)) for v in row) for row in rows) + "\n"
    out = subprocess.run([_host_program(tmp_path)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = np.array([[float(v) for v in line.split()] for line in out.stdout.strip().splitlines()]).reshape(B, 2, 6)
    want = ot.observe(p, x, x1, feet, u0, w0, N, gain=gain, torque_max=tmax, force_max=fmax)
    em, ee = np.abs(got[:, 0] - want["w_meas"]).max(), np.abs(got[:, 1] - want["w_est"]).max()
    print("host build against the twin: w_meas", em, "w_est", ee)
    assert em < 1e-12 and ee < 1e-12, (em, ee)
    assert np.abs(want["w_est"][:, 0:3]).max() == tmax and np.abs(want["w_est"][:, 3:6]).max() <= fmax      # (a clamp was at work)
