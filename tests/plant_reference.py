"""Test helper: a continuous-time reference of the fleet's plant, independent of tests/srbd_plant.py, tests/fleet_twin.py and
csrc/srbdqp_fleet.hpp in everything but the model.  Not a test module.

The rigid body is carried as (R in SO(3), c, L, v) -- attitude matrix, centre of mass, angular momentum about it in the world frame, velocity:

    R' = [omega]x R,   omega = R I_b^-1 R^T L
    c' = v
    L' = sum_i (p_i - c) x f_i + tau_push
    v' = (sum_i f_i + f_push) / m + g e_z

integrated in np.longdouble, vectorised over the robots, by classical RK4 at hundreds of substeps.  There are no Euler angles, no Euler rates and no equation
for omega' in it: roll, pitch and yaw are turned into R once at the start and read out of R once at the end.  reference() runs two resolutions and requires
them to agree, so that what is compared against it is compared against the differential equation, not against another discretisation of it.

draws() holds the inputs of tests/test_plant_reference_cpu.py and tests/test_gpu_plant_reference.py; it alone needs the twin (for QP forces: forces that are
no QP's, with net torques of tens of N m on I_z = 0.0032 kg m^2, take the body past 100 rad/s, which no integrator here resolves)."""
import functools

import numpy as np

LD = np.longdouble
KINDS = ("test", "yaw", "rates", "nopush", "flight")
B_DRAW = 77                      # a tile of 64 and a remainder of 13
SETTINGS = dict(tilt_max=1.5, z_min=0.1)   # nobody falls: tilt stays under 0.6 rad, the CoM above 0.5 m
SELF_TOL = 1e-10                 # reference(): 320 against 640 substeps


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _axis_rotation(axis, angle):
    """(B,3,3): the rotation by angle (B,) about coordinate axis 0, 1 or 2."""
    c, s = np.cos(angle), np.sin(angle)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    R = np.zeros(angle.shape + (3, 3), LD)
    R[..., axis, axis] = 1
    R[..., i, i] = c; R[..., j, j] = c
    R[..., j, i] = s; R[..., i, j] = -s
    return R


def attitude(rpy):
    """R = Rz(yaw) Ry(pitch) Rx(roll) (B,3,3) as a product of the three elementary rotations."""
    rpy = np.asarray(rpy, LD)
    return _axis_rotation(2, rpy[:, 2]) @ _axis_rotation(1, rpy[:, 1]) @ _axis_rotation(0, rpy[:, 0])


def angles(R):
    """(roll, pitch, yaw) (B,3) of R = Rz Ry Rx, |pitch| < pi / 2; yaw in (-pi, pi]."""
    return np.stack([np.arctan2(R[:, 2, 1], R[:, 2, 2]), np.arctan2(-R[:, 2, 0], np.hypot(R[:, 0, 0], R[:, 1, 0])), np.arctan2(R[:, 1, 0], R[:, 0, 0])], -1)


def omega_of(R, L, inertia):
    """omega = R I_b^-1 R^T L, (B,3)."""
    Lb = np.einsum("bji,bj->bi", R, L)
    return np.einsum("bij,bj->bi", R, Lb / inertia)


def momentum_of(R, omega, inertia):
    """L = R I_b R^T omega, (B,3)."""
    wb = np.einsum("bji,bj->bi", R, omega)
    return np.einsum("bij,bj->bi", R, wb * inertia)


def _per_robot(v, B, n):
    a = np.asarray(v, LD)
    return np.broadcast_to(a.reshape((-1, n)) if n > 1 else a.reshape(-1, 1), (B, n)).astype(LD)


def integrate(x, feet, u0, push, mass, inertia, dt, substeps, want_body=False):
    """One control period of B bodies.  x (B,13) = [rpy, c, omega (world), v, g], feet (B,12) world points, u0 (B,12) the forces held at them, push (B,6) =
    [torque about the CoM, force] or None, mass (B,) or a scalar, inertia (B,3) or (3,): the principal body inertias.
    Returns x1 (B,13) longdouble (yaw in (-pi, pi]) and max |R R^T - I| at the end; with want_body also dict(R0, L0, R1, L1, c1, v1)."""
    x = np.asarray(x, np.float64).astype(LD).reshape(-1, 13)
    B = x.shape[0]
    p = np.asarray(feet, np.float64).astype(LD).reshape(B, 4, 3)
    f = np.asarray(u0, np.float64).astype(LD).reshape(B, 4, 3)
    w = np.zeros((B, 6), LD) if push is None else np.asarray(push, np.float64).astype(LD).reshape(B, 6)
    m, I = _per_robot(mass, B, 1), _per_robot(inertia, B, 3)
    g = x[:, 12]
    fsum = f.sum(1)
    acc = (fsum + w[:, 3:6]) / m
    acc[:, 2] = acc[:, 2] + g
    # sum (p_i - c) x f_i = sum p_i x f_i - c x sum f_i
    tau_p = _cross(p, f).sum(1) + w[:, 0:3]

    def deriv(R, c, L, v):
        om = omega_of(R, L, I)
        dR = np.stack([_cross(om, R[:, :, j]) for j in range(3)], -1)
        return dR, v, tau_p - _cross(c, fsum), acc

    R, c, v = attitude(x[:, 0:3]), x[:, 3:6].copy(), x[:, 9:12].copy()
    L = momentum_of(R, x[:, 6:9], I)
    R0, L0 = R.copy(), L.copy()
    h = LD(dt) / LD(substeps)
    half, sixth = h / LD(2), h / LD(6)
    for _ in range(int(substeps)):
        s = (R, c, L, v)
        k1 = deriv(*s)
        k2 = deriv(*(a + half * k for a, k in zip(s, k1)))
        k3 = deriv(*(a + half * k for a, k in zip(s, k2)))
        k4 = deriv(*(a + h * k for a, k in zip(s, k3)))
        R, c, L, v = (a + sixth * (q1 + 2 * q2 + 2 * q3 + q4) for a, q1, q2, q3, q4 in zip(s, k1, k2, k3, k4))
    ortho = float(np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3, dtype=LD)).max())
    x1 = np.concatenate([angles(R), c, omega_of(R, L, I), v, g[:, None]], 1)
    if want_body:
        return x1, ortho, dict(R0=R0, L0=L0, R1=R, L1=L, c1=c, v1=v)
    return x1, ortho


def state_error(got, want):
    """|got - want| (B,12) over the twelve states, yaw modulo 2 pi; want: a reference x1."""
    d = np.asarray(got, LD)[:, 0:12] - np.asarray(want, LD)[:, 0:12]
    two_pi = 2 * np.arctan2(LD(0), LD(-1))
    d[:, 2] = d[:, 2] - two_pi * np.round(d[:, 2] / two_pi)
    return np.abs(d)


def reference(x, feet, u0, push, mass, inertia, dt, coarse=320, fine=640):
    """The period at `coarse` and at `fine` substeps.  The two must agree within SELF_TOL = 1e-10 on every state and stay orthogonal within it: a condition of
    use, 40 to 10^7 times under everything that is compared against the result.  Returns dict(x1 (B,13) longdouble: the finer one, self_diff, ortho, body)."""
    a, oa = integrate(x, feet, u0, push, mass, inertia, dt, coarse)
    b, ob, body = integrate(x, feet, u0, push, mass, inertia, dt, fine, want_body=True)
    diff = float(state_error(a, b).max())
    assert diff < SELF_TOL, f"the reference does not hold itself: {coarse} against {fine} substeps differ by {diff}"
    assert max(oa, ob) < SELF_TOL, f"the reference's R left SO(3) by {max(oa, ob)}"
    return dict(x1=b, self_diff=diff, ortho=max(oa, ob), body=body)


@functools.lru_cache(maxsize=None)
def _rollout(horizon=10, steps=50):
    """The twin's roll-out of its 6-robot fleet on the C oracle (what tests/test_gpu_fleet.py's `twin` fixture holds): the source of states and QP forces."""
    import fleet_twin as ft
    import srbd_oracle as orc
    f = ft.fleet()
    r = ft.rollout(orc.default_params(horizon), f["x"], f["feet"], f["stamp"], f["v_ref"], steps, ft.COM, standing=f["standing"], push=ft.fleet_push(steps, 6), solver="c")
    return r


def draws(seed, kind, horizon=10):
    """One input set of B = 77 robots, drawn as test_fleet_advance_against_the_twin draws its own: states, footholds and forces of the twin's 50-step roll-out
    (forces of solves), rolled and pitched by up to 0.3 rad more, rates disturbed.  kind:
      "test"    rates + N(0, 0.05), pushes of up to 3 N m (yaw included) and 30 N: the draw of that test;
      "yaw"     ... yaw uniform in +-pi, the push's yaw torque up to 0.3 N m;
      "rates"   ... rates + N(0, 0.5);
      "nopush"  the first without a push;
      "flight"  free flight: no forces, no push, angular rates uniform in +-2 rad/s, yaw uniform in +-pi.
    Every robot stands (no touchdown interferes), is alive, and stays inside SETTINGS' envelope; tilt <= 0.5 rad, so reading pitch out of R is well conditioned.
    Returns dict(x, feet, u0, push (or None), landing, stamp, standing, settings), read-only."""
    assert kind in KINDS
    r = _rollout(horizon)
    T = r["u0"].shape[0]
    rng = np.random.default_rng(seed)
    B = B_DRAW
    t, b = rng.integers(0, T, B), rng.integers(0, 6, B)
    x, feet, u0, landing = r["x"][t, b].copy(), r["feet"][t, b].copy(), r["u0"][t, b].copy(), r["landing"][t, b].copy()
    x[:, 0:2] += rng.uniform(-0.3, 0.3, (B, 2))
    x[:, 6:12] += rng.normal(size=(B, 6)) * (0.5 if kind == "rates" else 0.05)
    push = rng.uniform(-1.0, 1.0, (B, 6)) * np.array([3.0, 3.0, 0.3 if kind == "yaw" else 3.0, 30.0, 30.0, 30.0])
    if kind in ("yaw", "flight"):
        x[:, 2] = rng.uniform(-np.pi, np.pi, B)
    if kind == "flight":
        x[:, 6:9] = rng.uniform(-2.0, 2.0, (B, 3))
        u0[:] = 0.0
    if kind in ("nopush", "flight"):
        push = None
    assert np.abs(x[:, 0:2]).max() < 0.5
    out = dict(x=x, feet=feet, u0=u0, push=push, landing=landing, stamp=0.04 * rng.integers(0, 24, B).astype(np.float64), standing=np.ones(B, np.uint8))
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    out["settings"] = dict(SETTINGS)
    return out


def records(seed, params, B=B_DRAW):
    """Per-robot mass (25 to 45 kg) and inertia (0.7 to 1.5 times the config's) -> (mass (B,), inertia (B,3))."""
    rng = np.random.default_rng(seed)
    return rng.uniform(25.0, 45.0, B), np.array(params.inertia) * rng.uniform(0.7, 1.5, (B, 3))
