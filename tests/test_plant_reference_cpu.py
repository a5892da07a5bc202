"""The fleet's plant and its observer against the rigid body itself (DESIGN.md sections 17 and 19): tests/plant_reference.py integrates the equations of motion on
SO(3) in long double at 320 and 640 substeps, and the twins -- which restate the kernels operation for operation, and against which the kernels are tested --
are held against it here.  A twin test catches a kernel that departs from its specification; these catch a specification that departs from the model.

Bounds.  The reference against itself: 1e-10 (plant_reference.SELF_TOL), a condition of use.  The order of fleet_twin.advance: the error against the reference
falls by a factor in [12, 20] per halving of the substep -- a fourth-order method gives 16, [12, 20] is an order between 3.6 and 4.3; a wrong RK4 weight or
a missing term leaves an error that does not fall at all.  The observer's identity on the reference trajectory: 1e-10 N and N m -- the largest term is
m |v| / dt of about 900 with v rounded to float64 (1e-13), L / dt adds I |omega| / dt 2e-16 of about 1e-14, the reference's own 1e-10 / 40 divided by dt
bounds the rest.  Conservation inside the reference: 1e-12 relative on what RK4 only approximates, 1e-15 relative on what it sums exactly (2560 long-double
additions of 1.1e-19 each)."""
import numpy as np
import pytest

import c_oracle  # noqa: F401
import fleet_twin as ft
import observer_twin as ot
import plant_reference as pr
import srbd_oracle as orc

N, SEED = 10, 3
FORCED = pr.KINDS[:4]
SUBSTEPS = (5, 10, 20, 40)


@pytest.fixture(scope="module")
def refs():
    """The five draws and their references with the config's robot, and the four forced ones again with per-robot records: computed once, read-only."""
    p = orc.default_params(N)
    out = {}
    for kind in pr.KINDS:
        d = pr.draws(SEED, kind)
        out[kind, False] = (d, pr.reference(d["x"], d["feet"], d["u0"], d["push"], p.mass, p.inertia, p.dt), p.mass, np.array(p.inertia))
    mass, inertia = pr.records(SEED + 1, p)
    for kind in FORCED:
        d = pr.draws(SEED, kind)
        out[kind, True] = (d, pr.reference(d["x"], d["feet"], d["u0"], d["push"], mass, inertia, p.dt), mass, inertia)
    return out


def _twin_errors(p, d, ref):
    errs = []
    for s in SUBSTEPS:
        tw = ft.advance(p, d["x"], d["feet"], d["stamp"], d["u0"], d["landing"], standing=d["standing"], push=d["push"], substeps=s, **d["settings"])
        assert tw["alive"].all()
        errs.append(float(pr.state_error(tw["x"], ref["x1"]).max()))
    return errs


def test_closed_forms():
    """What has a closed form: a body spinning about its vertical principal axis under a constant torque about it, thrown sideways under a constant force --
    yaw = yaw0 + w dt + tau dt^2 / (2 I_z), w = w0 + tau dt / I_z, c = c0 + v0 dt + a dt^2 / 2 -- at 640 substeps."""
    dt, m, I = 0.04, 30.0, np.array([0.08, 0.07, 0.003])
    x = np.zeros((2, 13)); x[:, 12] = -9.80665
    x[:, 2] = [0.3, -2.9]; x[:, 8] = [5.0, -11.0]; x[:, 3:6] = [0.1, -0.2, 0.6]; x[:, 9:12] = [[0.3, -0.1, 0.2], [-1.0, 0.5, 0.0]]
    push = np.array([[0.0, 0.0, 0.02, 12.0, -7.0, 3.0], [0.0, 0.0, -0.05, 0.0, 20.0, -4.0]])
    x1, ortho = pr.integrate(x, np.zeros((2, 12)), np.zeros((2, 12)), push, m, I, dt, 640)
    LD = np.longdouble
    yaw = LD(1) * x[:, 2] + LD(dt) * x[:, 8] + LD(dt) ** 2 * push[:, 2] / (2 * LD(I[2]))
    want = np.zeros((2, 12), LD)
    want[:, 2], want[:, 8] = yaw, x[:, 8] + LD(dt) * push[:, 2] / LD(I[2])
    acc = push[:, 3:6] / LD(m) + np.array([0, 0, x[0, 12]], LD)
    want[:, 3:6], want[:, 9:12] = x[:, 3:6] + LD(dt) * x[:, 9:12] + LD(dt) ** 2 / 2 * acc, x[:, 9:12] + LD(dt) * acc
    err = pr.state_error(x1, want)
    # the rotation is RK4's (the reference's own bar); position and velocity are polynomials of degree <= 2 in t, which RK4 sums exactly
    assert ortho < pr.SELF_TOL and err[:, [0, 1, 2, 6, 7, 8]].max() < pr.SELF_TOL
    assert err[:, [3, 4, 5, 9, 10, 11]].max() < 1e-15


def test_the_reference_holds_itself(refs):
    """Self-convergence and orthogonality on every draw (reference() asserts 1e-10; measured under 4e-11 and 1e-11); in free flight L and the rotational
    kinetic energy L . omega / 2 stay within 1e-12 relative and v changes by g dt within 1e-15 relative; under forces m v changes by the impulse of forces,
    push and gravity within 1e-15 of the terms' size."""
    LD = np.longdouble
    for (kind, rec), (d, ref, mass, inertia) in refs.items():
        print(f"reference, {kind}{', records' if rec else ''}: 320 against 640 substeps {ref['self_diff']:.1e}, |R R' - I| {ref['ortho']:.1e}")
        assert ref["self_diff"] < pr.SELF_TOL and ref["ortho"] < pr.SELF_TOL
        body, x = ref["body"], d["x"]
        m = np.broadcast_to(np.asarray(mass, LD).reshape(-1, 1), (x.shape[0], 1))
        f = d["u0"].reshape(-1, 4, 3).astype(LD).sum(1) + (0 if d["push"] is None else d["push"][:, 3:6].astype(LD))
        impulse = (f + m * np.array([0, 0, 1], LD) * x[:, 12:13]) * LD(0.04)
        dp = m * (body["v1"] - x[:, 9:12].astype(LD))
        scale = np.abs(m * body["v1"]).max() + np.abs(impulse).max()
        assert np.abs(dp - impulse).max() < 1e-15 * scale
        if kind == "flight":
            I = np.broadcast_to(np.asarray(inertia, LD), (x.shape[0], 3))
            assert np.abs(body["L1"] - body["L0"]).max() <= 1e-12 * np.abs(body["L0"]).max()
            ke = [0.5 * (L * pr.omega_of(R, L, I)).sum(1) for R, L in ((body["R0"], body["L0"]), (body["R1"], body["L1"]))]
            assert np.abs(ke[1] - ke[0]).max() < 1e-12 * ke[0].max()
            dv = body["v1"] - x[:, 9:12].astype(LD)
            g_dt = LD(x[0, 12]) * LD(0.04)
            assert np.abs(dv[:, 0:2]).max() == 0 and np.abs(dv[:, 2] - g_dt).max() < 1e-15 * abs(g_dt)


def test_the_order_of_the_twins_plant(refs):
    """fleet_twin.advance at 5, 10, 20 and 40 substeps against the reference, maximum over robots and the twelve states, yaw modulo 2 pi: every halving gains
    a factor in [12, 20], on every draw with forces.  Measured (this table stands in DESIGN.md section 17):

        draw                          substeps 5      10       20       40    factors
        the test's own (3 N m yaw)       1.3e-03  9.1e-05  5.9e-06  3.8e-07   14.5 15.3 15.7
        yaw +-pi, yaw torque 0.3 N m     6.6e-05  4.0e-06  2.5e-07  1.6e-08   16.3 16.2 16.1
        rates +-0.5                      3.6e-03  2.9e-04  2.1e-05  1.4e-06   12.6 13.5 14.8
        no push                          4.2e-05  2.6e-06  1.6e-07  1.0e-08   16.1 16.0 16.0
        (free flight                     2.5e-09  1.6e-10  9.9e-12  6.2e-13   16.0 16.0 16.0)

    At the default 10 substeps the plant is 1e-4 to 1e-6 away from the model; 2.2e-13, the figure tests/test_gpu_fleet.py quotes, is the rounding error of the
    same scheme in float64 against long double, not its accuracy."""
    p = orc.default_params(N)
    print("fleet_twin.advance against the reference: draw, e_5 e_10 e_20 e_40, factors")
    for (kind, rec), (d, ref, mass, inertia) in refs.items():
        if rec:                                                                    # (records: tests/test_gpu_plant_reference.py, beside the device)
            continue
        errs = _twin_errors(p, d, ref)
        ratios = [errs[i] / errs[i + 1] for i in range(len(errs) - 1)]
        print(f"  {kind:8s}", " ".join(f"{e:.1e}" for e in errs), " ", " ".join(f"{r:.1f}" for r in ratios))
        assert errs[-1] > 100 * ref["self_diff"]                                   # the reference is the finer of the two by far
        if kind != "flight":
            assert all(12.0 <= r <= 20.0 for r in ratios), (kind, rec, errs, ratios)


def test_the_observer_returns_the_push_on_the_reference_trajectory(refs):
    """Under constant forces and a constant push, f_meas and tau_meas of observer_measure ARE the push: on the reference's x1, rounded to float64,
    observer_twin.measure returns it within 1e-10 N and N m (measured 5.6e-12), with the config's robot and with robot records; on the twin's own RK4
    trajectory at 10 substeps it is off by the plant's error over dt."""
    p = orc.default_params(N)
    worst = 0.0
    for (kind, rec), (d, ref, mass, inertia) in refs.items():
        if kind == "flight":
            continue
        B = d["x"].shape[0]
        m, I = np.broadcast_to(mass, (B,)), np.broadcast_to(inertia, (B, 3))
        x1 = ref["x1"].astype(np.float64)
        push = np.zeros((B, 6)) if d["push"] is None else d["push"]
        wm = np.array([ot.measure(float(m[b]), tuple(I[b]), p.dt, d["x"][b], x1[b], d["feet"][b], d["u0"][b]) for b in range(B)])
        err = np.abs(wm - push).max()
        worst = max(worst, err)
        assert err < 1e-10, (kind, rec, err)
        if not rec:
            tw = ft.advance(p, d["x"], d["feet"], d["stamp"], d["u0"], d["landing"], standing=d["standing"], push=d["push"], **d["settings"])
            wt = np.array([ot.measure(p.mass, p.inertia, p.dt, d["x"][b], tw["x"][b], d["feet"][b], d["u0"][b]) for b in range(B)])
            print(f"observer on the twin's own trajectory, {kind}: off the push by {np.abs(wt - push).max():.1e}")
            assert np.abs(wt - push).max() > 100 * err
    print(f"observer_twin.measure on the reference trajectory: worst |w_meas - push| {worst:.1e}")
