"""GPU tests of the fleet's plant step and momentum observer against the rigid body itself (DESIGN.md sections 17 and 19): tests/plant_reference.py, the equations
of motion on SO(3) in long double, where tests/test_gpu_fleet.py and tests/test_gpu_observer.py hold the kernels against twins that restate them
(tests/test_plant_reference_cpu.py holds the twins against the same reference).  B = 77 (a tile of 64 and a remainder of 13), N = 10.

Bounds.  Order: the device's error against the reference falls by a factor in [12, 20] per halving of the substep (a fourth-order method: 16).  Size: the device's
error is at most 1.05 times the twin's against the same reference, plus 1e-9, the project's bar between kernel and twin -- the twin is the specification, the
reference sets the bar.  Free flight: linear momentum and v_z within 1e-12 (the kernel adds h times a constant 4 substeps times; m |v| is about 30).  Observer on
the reference trajectory: 1e-9 N and N m, the project's absolute bar on these quantities, 200 times what the float64 formula reaches on this data on the CPU
(5.6e-12).  Kept estimates and the horizon's products: bit for bit."""
import numpy as np
import pytest

import c_oracle  # noqa: F401
import fleet_twin as ft
from fleet_loop import _bits
import observer_twin as ot
import plant_reference as pr
import srbd_oracle as orc

pytestmark = pytest.mark.gpu
N, SEED = 10, 3
SUBSTEPS = (5, 10, 20, 40)
FORCED = pr.KINDS[:4]


@pytest.fixture(scope="module")
def eng():
    import torch  # noqa: F401
    from g1_locomotion_amd import BatchMPC
    e = BatchMPC(horizon=N)
    yield e
    e.close()


@pytest.fixture(scope="module")
def refs():
    """(kind, records?) -> dict(d: the draw, ref: its reference, mass, inertia, robots: the records or None): the five draws with the config's robot, the four with
    forces again with robot records.  Computed once on the CPU, read-only."""
    from g1_locomotion_amd.mpc import robots_array
    p = orc.default_params(N)
    mass, inertia = pr.records(SEED + 1, p)
    out = {}
    for kind in pr.KINDS:
        d = pr.draws(SEED, kind)
        out[kind, False] = dict(d=d, ref=pr.reference(d["x"], d["feet"], d["u0"], d["push"], p.mass, p.inertia, p.dt), mass=p.mass, inertia=np.array(p.inertia), robots=None)
        if kind in FORCED:
            out[kind, True] = dict(d=d, ref=pr.reference(d["x"], d["feet"], d["u0"], d["push"], mass, inertia, p.dt), mass=mass, inertia=inertia,
                                   robots=robots_array(pr.B_DRAW, mass=mass, inertia=inertia))
    return out


@pytest.fixture(scope="module")
def twin_errors(refs):
    """e_s of fleet_twin.advance against the reference, s in SUBSTEPS, for the six cases of the order test: the specification's own distance from the model."""
    p = orc.default_params(N)
    out = {}
    for key in [(k, False) for k in pr.KINDS] + [("test", True)]:
        c = refs[key]
        d = c["d"]
        out[key] = []
        for s in SUBSTEPS:
            tw = ft.advance(p, d["x"], d["feet"], d["stamp"], d["u0"], d["landing"], standing=d["standing"], push=d["push"], robots=c["robots"], substeps=s, **d["settings"])
            assert tw["alive"].all()
            out[key].append(float(pr.state_error(tw["x"], c["ref"]["x1"]).max()))
    return out


def _advance(eng, c, s, **extra):
    d = c["d"]
    eng.set_robots(c["robots"])
    try:
        got = eng.fleet_advance(d["x"], d["feet"], d["stamp"], d["u0"], d["landing"], standing=d["standing"], push=d["push"], substeps=s, **extra, **d["settings"])
    finally:
        eng.set_robots(None)
    assert got["alive"].all() and np.array_equal(_bits(got["feet"]), _bits(d["feet"]))          # everybody stands: the plant alone acted
    return got


def test_the_plants_order_on_the_device(eng, refs, twin_errors):
    """eng.fleet_advance at 5, 10, 20 and 40 substeps against the reference, maximum over robots and the twelve states as the device returns them (yaw modulo
    2 pi): on all five draws, once with robot records (mass 25 to 45 kg, inertia x 0.7 to 1.5; the reference takes the same), once on
    fleet_advance_terrain_steered_f64 over an all-zero map under a landing_yaw.  Every halving gains a factor in [12, 20], and e_s is at most 1.05 times the
    twin's e_s against the same reference plus 1e-9.  A wrong RK4 weight, a wrong h, a missing gyroscopic term or a wrong sy entry of R fails the first by
    orders of magnitude, and the twin cannot vouch for it: the bar is the reference's.  Measured on the MI355X: the device's e_s equal the twin's to four digits
    (1.317e-3, 9.105e-5, 5.943e-6, 3.788e-7 on the first draw), factors 12.63 to 16.28 (DESIGN.md section 17 has every row)."""
    rng = np.random.default_rng(SEED + 2)
    runs = [(key, "fleet_advance_f64", {}) for key in twin_errors] + [(("yaw", False), "fleet_advance_terrain_steered_f64", dict(landing_yaw=rng.uniform(-np.pi, np.pi, pr.B_DRAW)))]
    print("fleet_advance against the reference: case, e_5 e_10 e_20 e_40 on the device, factors, the twin's e_s")
    for key, kernel, extra in runs:
        c = refs[key]
        if extra:
            eng.set_terrain(np.zeros((4, 4)), origin=(-3.0, -3.0), cell=2.0)
        try:
            errs = []
            for s in SUBSTEPS:
                got = _advance(eng, c, s, **extra)
                assert eng.kernel_name() == kernel
                errs.append(float(pr.state_error(got["x"], c["ref"]["x1"]).max()))
        finally:
            if extra:
                eng.set_terrain(None)
        ratios = [errs[i] / errs[i + 1] for i in range(len(errs) - 1)]
        what = key[0] + (", records" if key[1] else "") + (", terrain + steered" if extra else "")
        print(f"  {what:26s}", " ".join(f"{e:.3e}" for e in errs), " ", " ".join(f"{r:.2f}" for r in ratios), "  twin", " ".join(f"{e:.3e}" for e in twin_errors[key]))
        assert all(12.0 <= r <= 20.0 for r in ratios), (what, errs, ratios)
        for e, te in zip(errs, twin_errors[key]):
            assert e <= 1.05 * te + 1e-9, (what, errs, twin_errors[key])


def test_free_flight_on_the_device(eng, refs):
    """No forces, no push, rates of up to 2 rad/s at any yaw: the linear momentum in the plane is what it was (m |v1 - v0| within 1e-12 kg m/s) and v_z gained g dt within 1e-12 m/s,
    at every substep count; |L(x1) - L(x0)|, the drift of the angular momentum the scheme does not conserve, falls by a factor in [12, 20] per halving."""
    c = refs["flight", False]
    d = c["d"]
    p = orc.default_params(N)
    L0 = np.array([ot.momentum(p.inertia, d["x"][b]) for b in range(pr.B_DRAW)])
    drift = []
    for s in SUBSTEPS:
        got = _advance(eng, c, s)
        dv = got["x"][:, 9:12] - d["x"][:, 9:12]
        dv[:, 2] -= d["x"][:, 12] * p.dt
        assert p.mass * np.abs(dv[:, 0:2]).max() < 1e-12 and np.abs(dv[:, 2]).max() < 1e-12, np.abs(dv).max(axis=0)
        drift.append(np.abs(np.array([ot.momentum(p.inertia, got["x"][b]) for b in range(pr.B_DRAW)]) - L0).max())
    ratios = [drift[i] / drift[i + 1] for i in range(len(drift) - 1)]
    print("free flight on the device: |L1 - L0|", " ".join(f"{e:.3e}" for e in drift), "factors", " ".join(f"{r:.2f}" for r in ratios))
    assert all(12.0 <= r <= 20.0 for r in ratios), (drift, ratios)


def test_the_observer_on_the_reference_trajectory(eng, refs):
    """eng.wrench_observer(x, x1 of the reference rounded to float64, feet, u0, w_est = 0, gain = 1) under the default clamps, on the four draws with forces, with
    the config's robot and with robot records: w_est is the push within 1e-9 N and N m (the identity the observer is derived from, on a trajectory that is the
    rigid body's, not the plant's); a quarter of the robots are down and keep their estimate bit for bit; ew[b, k] = w_est[b] 0.9^k as observer_twin.horizon
    multiplies it, bit for bit.  Measured on the MI355X: worst |w_est - push| 5.64e-12 (the draw with large rates), 6e-14 without a push."""
    rng = np.random.default_rng(SEED + 3)
    B = pr.B_DRAW
    alive = (rng.random(B) >= 0.25).astype(np.uint8)
    dead = alive == 0
    assert B // 8 < dead.sum() < B // 2
    w0 = np.zeros((B, 6))
    w0[dead] = rng.uniform(-1.0, 1.0, (int(dead.sum()), 6))                         # what the robots that are down hold: theirs to keep
    worst = 0.0
    for key in [(k, r) for k in FORCED for r in (False, True)]:
        c = refs[key]
        d = c["d"]
        push = np.zeros((B, 6)) if d["push"] is None else d["push"]
        assert np.abs(push[:, 0:3]).max() < 50.0 and np.abs(push[:, 3:6]).max() < 200.0
        eng.set_robots(c["robots"])
        try:
            got = eng.wrench_observer(d["x"], c["ref"]["x1"].astype(np.float64), d["feet"], d["u0"], w0, alive=alive, gain=1.0, horizon_decay=0.9)
        finally:
            eng.set_robots(None)
        assert eng.kernel_name() == "wrench_observer_f64"
        err = np.abs(got["w_est"][~dead] - push[~dead]).max()
        worst = max(worst, err)
        print(f"wrench_observer on the reference trajectory, {key[0]}{', records' if key[1] else ''}: |w_est - push| {err:.2e}")
        assert err < 1e-9, (key, err)
        assert np.array_equal(_bits(got["w_est"][dead]), _bits(w0[dead]))
        assert np.array_equal(_bits(got["ew"]), _bits(ot.horizon(got["w_est"], N, 0.9)))
    print(f"wrench_observer on the reference trajectory: worst |w_est - push| {worst:.2e}")
