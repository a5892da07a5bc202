"""Test helper: the NumPy twin of the momentum observer and of the observed roll-out (include/srbdqp_cascade.h srbdqp_wrench_observer_* /
srbdqp_fleet_rollout_observed_*; csrc/srbdqp_observer.hpp).

measure(): the formulas of the header, operation for operation.  observe(): the filter, the clamps, the keep rule and the horizon.  rollout(): fleet_twin's
loop with side_inputs.twin(..., ext_wrench=) as the solver and observe() behind advance() -- the estimate of period t serves solve t + 1."""
import numpy as np

import cascade_oracle as co
import fleet_twin as ft
import side_inputs as si

DEFAULTS = dict(gain=0.5, horizon_decay=1.0, torque_max=50.0, force_max=200.0)


def momentum(inertia, x):
    """L(x) = R diag(I_b) R' omega, R = Rz(yaw) Ry(pitch) Rx(roll), written out as fleet_deriv writes R."""
    sr, cr, sp, cp, sy, cy = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    R = [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
         [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
         [-sp, cp * sr, cp * cr]]
    hb = [inertia[i] * (R[0][i] * x[6] + R[1][i] * x[7] + R[2][i] * x[8]) for i in range(3)]
    return np.array([R[i][0] * hb[0] + R[i][1] * hb[1] + R[i][2] * hb[2] for i in range(3)])


def measure(mass, inertia, dt, x0, x1, feet, u0):
    """w_meas (6,) = [tau_meas, f_meas] of one robot over one period: x0 (13,) before it, x1 behind it, feet (12,) the contact points the forces u0 (12,)
    acted at."""
    x0, x1, p, f = (np.asarray(a, np.float64).reshape(-1) for a in (x0, x1, feet, u0))
    w = np.zeros(6)
    cb = np.zeros(3)
    for i in range(3):
        fs = ((f[i] + f[3 + i]) + f[6 + i]) + f[9 + i]
        w[3 + i] = mass * (x1[9 + i] - x0[9 + i]) / dt - fs
        cb[i] = x0[3 + i] + dt * (2.0 * x0[9 + i] + x1[9 + i]) / 6.0
    w[5] = w[5] - mass * x0[12]
    tc = np.zeros(3)
    for c in range(4):
        rx, ry, rz = p[3 * c] - cb[0], p[3 * c + 1] - cb[1], p[3 * c + 2] - cb[2]
        fx, fy, fz = f[3 * c], f[3 * c + 1], f[3 * c + 2]
        tc[0] += ry * fz - rz * fy
        tc[1] += rz * fx - rx * fz
        tc[2] += rx * fy - ry * fx
    L0, L1 = momentum(inertia, x0), momentum(inertia, x1)
    for i in range(3):
        w[i] = (L1[i] - L0[i]) / dt - tc[i]
    return w


def horizon(w_est, N, decay):
    """ew (B,N,6): s_0 = w_est, s_{k+1} = s_k decay -- one rounded product after the other."""
    w = np.asarray(w_est, np.float64)
    out = np.empty((w.shape[0], N, 6))
    s = w.copy()
    for k in range(N):
        out[:, k] = s
        s = s * decay
    return out


def observe(params, x_prev, x_next, feet_prev, u0, w_est, N, alive=None, robots=None, **settings):
    """The twin of srbdqp_wrench_observer_*: dict(w_est (B,6), ew (B,N,6), w_meas (B,6) -- NaN rows where the robot kept its estimate)."""
    s = dict(DEFAULTS, **settings)
    x0 = np.asarray(x_prev, np.float64).reshape(-1, 13)
    B = x0.shape[0]
    x1 = np.asarray(x_next, np.float64).reshape(B, 13)
    feet = np.asarray(feet_prev, np.float64).reshape(B, 12)
    u0 = np.asarray(u0, np.float64).reshape(B, 12)
    w = np.array(w_est, np.float64).reshape(B, 6)
    wm = np.full((B, 6), np.nan)
    lim = np.array([s["torque_max"]] * 3 + [s["force_max"]] * 3)
    for b in range(B):
        if (alive is not None and not alive[b]) or not (np.all(np.isfinite(x0[b])) and np.all(np.isfinite(x1[b]))):
            continue
        mass, inertia = (params.mass, params.inertia) if robots is None else (float(robots[b, 0]), tuple(float(v) for v in robots[b, 1:4]))
        wm[b] = measure(mass, inertia, params.dt, x0[b], x1[b], feet[b], u0[b])
        v = w[b] + s["gain"] * (wm[b] - w[b])
        w[b] = np.fmin(np.fmax(v, -lim), lim)
    return dict(w_est=w, ew=horizon(w, N, s["horizon_decay"]), w_meas=wm)


def solve(params, x, inputs, ew):
    """The QPs of one control step under the wrenches ew (B,N,6), or blind (ew None), on side_inputs.twin -> dict(u0 (B,12), status, iters)."""
    out = [si.twin(params, x[b], inputs["x_ref"][b], inputs["foot"][b], inputs["contact"][b], pcom=inputs["pcom"][b], ext_wrench=None if ew is None else ew[b])
           for b in range(x.shape[0])]
    return dict(u0=np.stack([o["u"][0] for o in out]), status=np.array([o["status"] for o in out], np.int32), iters=np.array([o["iters"] for o in out], np.int32))


def rollout(params, x0, feet, stamp, v_ref, steps, com_target, standing=None, push=None, alive=None, observer=None, w_est=None, horizon_len=10, **settings):
    """The twin of srbdqp_fleet_rollout_observed_* (observer: a dict of DEFAULTS' keys, {} for the defaults) and, with observer=None, the blind roll-out on the
    same solver: dict(x (T+1,B,13), u0, feet, status, iters, alive, stamp[, w_est (B,6), w_log (T,B,6)])."""
    s = dict(ft.DEFAULTS, **settings)
    x = np.array(x0, np.float64).reshape(-1, 13)
    B, N = x.shape[0], int(horizon_len)
    feet = np.array(feet, np.float64).reshape(B, 12)
    stamp = np.array(stamp, np.float64).reshape(B)
    alive = np.ones(B, np.uint8) if alive is None else np.array(np.asarray(alive) != 0, np.uint8).reshape(B)
    obs = None if observer is None else dict(DEFAULTS, **observer)
    w = None if obs is None else (np.zeros((B, 6)) if w_est is None else np.array(w_est, np.float64).reshape(B, 6))
    ew = None if obs is None else horizon(w, N, obs["horizon_decay"])
    xs, fs, us, st, it, wl = [x.copy()], [feet.copy()], [], [], [], []
    for t in range(steps):
        inp = co.mpc_inputs(x, feet, stamp, v_ref, com_target, N, params.dt, standing=standing, period_steps=s["period_steps"],
                            double_support_steps=s["double_support_steps"], hip_offset_y=s["hip_offset_y"])
        sol = solve(params, x, inp, ew)
        r = ft.advance(params, x, feet, stamp, sol["u0"], inp["landing"], standing=standing, push=None if push is None else push[t], alive=alive, **settings)
        if obs is not None:
            o = observe(params, x, r["x"], feet, sol["u0"], w, N, alive=r["alive"], **obs)
            w, ew = o["w_est"], o["ew"]
            wl.append(w.copy())
        x, feet, stamp, alive = r["x"], r["feet"], r["stamp"], r["alive"]
        xs.append(x.copy()); fs.append(feet.copy()); us.append(sol["u0"]); st.append(sol["status"]); it.append(sol["iters"])
    out = dict(x=np.array(xs), u0=np.array(us), feet=np.array(fs), status=np.array(st), iters=np.array(it), alive=alive, stamp=stamp)
    if obs is not None:
        out.update(w_est=w, w_log=np.array(wl))
    return out


def sustained_push(T, B, start=5, fx=10.0, fy=-25.0):
    """The push of the benefit scenario: fx N along x and fy N along y on every robot from step `start` on."""
    push = np.zeros((T, B, 6))
    push[start:, :, 3] = fx
    push[start:, :, 4] = fy
    return push
