"""Test helper: the NumPy twin of the fleet roll-out (include/srbdqp_cascade.h srbdqp_fleet_advance_* / srbdqp_fleet_rollout_*).

Per control step and robot: cascade_oracle.mpc_inputs -> a CPU solve (c_oracle.solve_batch, or srbd_oracle.update with solver="numpy") -> advance(): the
SrbdPlant of tests/srbd_plant.py, extended by the push wrench, `substeps` times, then the stamp, the touchdown and the fallen flag -- the same operations in
the same order as the kernel."""
import numpy as np

import c_oracle
import cascade_oracle as co
import srbd_oracle as orc
from srbd_plant import SrbdPlant, rot_zyx, euler_rate_matrix

DEFAULTS = dict(substeps=10, foot_half_length=0.085, z_min=0.3, tilt_max=1.0, period_steps=6, double_support_steps=1, hip_offset_y=0.0645)

FEET = np.array([[0.0, 0.0645, 0.0], [0.17, 0.0645, 0.0], [0.0, -0.0645, 0.0], [0.17, -0.0645, 0.0]])
COM = np.array([0.085, 0.0, 0.598])


class PushedPlant(SrbdPlant):
    """SrbdPlant under a world wrench on the body, push = [torque about the CoM, force], beside the contact forces (None: SrbdPlant, bit for bit)."""
    push = None

    def deriv(self, x, feet, u):
        if self.push is None:
            return super().deriv(x, feet, u)
        R = rot_zyx(x[0:3])
        Iw = R @ np.diag(self.p.inertia) @ R.T
        w = x[6:9]
        F = u.reshape(4, 3)
        tau = sum(np.cross(feet[i] - x[3:6], F[i]) for i in range(4)) + self.push[0:3]
        dx = np.zeros(13)
        dx[0:3] = euler_rate_matrix(x[0:3]) @ (R.T @ w)
        dx[3:6] = x[9:12]
        dx[6:9] = np.linalg.solve(Iw, tau - np.cross(w, Iw @ w))
        dx[9:12] = F.sum(0) / self.p.mass + self.push[3:6] / self.p.mass + np.array([0, 0, x[12]])
        return dx


def first_step_flags(stamp, dt, standing, period, ds):
    """(left, right) stance flags of the horizon's first step at `stamp` -- cascade_oracle.mpc_inputs' schedule."""
    k0 = np.floor(np.asarray(stamp, np.float64) / dt + 1e-9).astype(np.int64)
    ph = k0 % (2 * period)
    left = ph < period
    dsup = (ph % period) < ds
    standing = np.asarray(standing) != 0
    return standing | left | dsup, standing | ~left | dsup


def fleet():
    """The 6-robot fleet of the roll-out tests: one stands, one steps in place, four walk; stamps staggered by one step per robot."""
    v_ref = np.array([[0.0, 0.0], [0.0, 0.0], [0.2, 0.0], [0.2, 0.0], [0.0, 0.1], [0.3, -0.05]])
    B = v_ref.shape[0]
    standing = np.zeros(B, np.uint8); standing[0] = 1
    x = np.zeros((B, 13)); x[:, 3:6] = COM; x[:, 12] = -9.80665
    x[:, 0] = 0.01 * np.arange(B) - 0.02                      # a little roll each, so that no two robots are alike
    x[:, 3] += 0.005 * np.arange(B)
    feet = np.tile(FEET.reshape(12), (B, 1))
    stamp = 0.04 * np.arange(B, dtype=np.float64)
    return dict(x=x, feet=feet, stamp=stamp, v_ref=v_ref, standing=standing)


def fleet_push(T, B, step=5):
    """A shove of one control period at step `step`: 10 N forward and 15 N to the right on every robot.  (No torque: about the vertical, where the torso's
    inertia is 0.003 kg m^2, a torque turns the last bits in which two CPU oracles differ into 1e-8 rad/s within a few steps -- the roll-out tests compare
    trajectories, and advance()'s own test covers torques.)"""
    push = np.zeros((T, B, 6))
    if step < T:
        push[step, :, 3] = 10.0; push[step, :, 4] = -15.0
    return push


def advance(params, x, feet, stamp, u0, landing, standing=None, push=None, alive=None, robots=None, **settings):
    """One control period of B robots: the twin of srbdqp_fleet_advance_*.  params: orc.SrbdParams (dt, mass, inertia); robots (B,8) records or None.
    Returns dict(x, feet, stamp, alive, moved (B,) 0 / 1 = left / 2 = right: the touchdown decisions)."""
    s = dict(DEFAULTS, **settings)
    x = np.array(x, np.float64).reshape(-1, 13)
    B = x.shape[0]
    feet = np.array(feet, np.float64).reshape(B, 12)
    stamp = np.array(stamp, np.float64).reshape(B)
    u0 = np.asarray(u0, np.float64).reshape(B, 12)
    landing = np.asarray(landing, np.float64).reshape(B, 3)
    standing = np.zeros(B, np.uint8) if standing is None else np.asarray(standing).reshape(B)
    alive = np.ones(B, np.uint8) if alive is None else np.array(np.asarray(alive) != 0, np.uint8).reshape(B)
    dt = params.dt
    stamp1 = stamp + dt
    l0, r0 = first_step_flags(stamp, dt, standing, s["period_steps"], s["double_support_steps"])
    l1, r1 = first_step_flags(stamp1, dt, standing, s["period_steps"], s["double_support_steps"])
    moved = np.zeros(B, np.int32)
    h = dt / s["substeps"]
    fhl = np.array([s["foot_half_length"], 0.0, 0.0])
    for b in range(B):
        if not alive[b] or not np.all(np.isfinite(x[b])):                     # 1. skip
            alive[b] = 0
            continue
        p = params
        if robots is not None:
            p = orc.SrbdParams(dt=dt, mass=float(robots[b, 0]), inertia=tuple(float(v) for v in robots[b, 1:4]))
        plant = PushedPlant(p)
        plant.push = None if push is None else np.asarray(push, np.float64).reshape(B, 6)[b]
        xb, fb = x[b], feet[b].reshape(4, 3).copy()
        outside0 = xb[5] < s["z_min"] or abs(xb[0]) > s["tilt_max"] or abs(xb[1]) > s["tilt_max"]      # handed over outside the envelope: fallen already
        for _ in range(s["substeps"]):                                        # 2. plant
            xb = plant.step(xb, fb, u0[b], h)
        x[b] = xb
        if not l0[b] and l1[b]:                                               # 4. touchdown
            feet[b, 0:3], feet[b, 3:6], moved[b] = landing[b] - fhl, landing[b] + fhl, 1
        elif not r0[b] and r1[b]:
            feet[b, 6:9], feet[b, 9:12], moved[b] = landing[b] - fhl, landing[b] + fhl, 2
        if outside0 or not np.all(np.isfinite(xb)) or xb[5] < s["z_min"] or abs(xb[0]) > s["tilt_max"] or abs(xb[1]) > s["tilt_max"]:   # 5. fallen
            alive[b] = 0
    return dict(x=x, feet=feet, stamp=stamp1, alive=alive, moved=moved)


def solve(params, x, inputs, solver="c"):
    """The QPs of one control step on the CPU -> dict(u0 (B,12), status, iters).  solver: "c" (c_oracle.solve_batch) or "numpy" (orc.update per robot)."""
    if solver == "c":
        r = c_oracle.solve_batch(params, x, inputs["x_ref"], inputs["foot"], inputs["contact"], pcom=inputs["pcom"])
        return dict(u0=r["u"][:, 0].copy(), status=r["status"].astype(np.int32), iters=r["iters"].astype(np.int32))
    out = [orc.update(params, x[b], inputs["x_ref"][b], inputs["foot"][b], inputs["contact"][b], pcom_hor=inputs["pcom"][b]) for b in range(x.shape[0])]
    return dict(u0=np.stack([o["u"][0] for o in out]), status=np.array([o["status"] for o in out], np.int32), iters=np.array([o["iters"] for o in out], np.int32))


def rollout(params, x0, feet, stamp, v_ref, steps, com_target, standing=None, push=None, alive=None, solver="c", horizon=10, mpc_view=None, **settings):
    """The twin of srbdqp_fleet_rollout_*: dict(x (T+1,B,13), u0 (T,B,12), feet (T+1,B,12), status, iters (T,B), landing (T,B,3), alive, stamp).
    mpc_view: what the MPC side sees of the states (B,13) -> (B,13), e.g. the round trip through the message types; default: the states themselves."""
    s = dict(DEFAULTS, **settings)
    x = np.array(x0, np.float64).reshape(-1, 13)
    B, N = x.shape[0], int(horizon)
    feet = np.array(feet, np.float64).reshape(B, 12)
    stamp = np.array(stamp, np.float64).reshape(B)
    alive = np.ones(B, np.uint8) if alive is None else np.array(np.asarray(alive) != 0, np.uint8).reshape(B)
    xs, fs, us, st, it, lps = [x.copy()], [feet.copy()], [], [], [], []
    for t in range(steps):
        xm = x if mpc_view is None else mpc_view(x)
        inp = co.mpc_inputs(xm, feet, stamp, v_ref, com_target, N, params.dt, standing=standing, period_steps=s["period_steps"],
                            double_support_steps=s["double_support_steps"], hip_offset_y=s["hip_offset_y"])
        sol = solve(params, xm, inp, solver)
        r = advance(params, x, feet, stamp, sol["u0"], inp["landing"], standing=standing, push=None if push is None else push[t], alive=alive, **settings)
        x, feet, stamp, alive = r["x"], r["feet"], r["stamp"], r["alive"]
        xs.append(x.copy()); fs.append(feet.copy()); us.append(sol["u0"]); st.append(sol["status"]); it.append(sol["iters"]); lps.append(inp["landing"])
    return dict(x=np.array(xs), u0=np.array(us), feet=np.array(fs), status=np.array(st), iters=np.array(it), landing=np.array(lps), alive=alive, stamp=stamp)
