"""Test helper: the NumPy twin of the steered fleet calls (include/srbdqp_cascade.h srbdqp_mpc_inputs_steered_*, srbdqp_fleet_advance_steered_*,
srbdqp_fleet_rollout_steered_*), built on fleet_twin and cascade_oracle: the same operations in the same order as the header states
them.  It is the specification the device is held to.

A command is (vx, vy, wz): planar velocity in the robot's heading frame, m/s, and yaw rate, rad/s."""
import numpy as np

import cascade_oracle as co
import fleet_twin as ft

COMMANDS = np.array([[0.2, 0.0, 0.0], [0.2, 0.0, 0.3], [0.2, 0.0, 0.6], [0.0, 0.0, 0.5], [0.3, -0.05, -0.4], [0.0, 0.1, 1.0]])


def rotate(theta, vx, vy):
    """v_w(theta) = Rz(theta) (vx, vy) -> (wx, wy)."""
    s, c = np.sin(theta), np.cos(theta)
    return c * vx - s * vy, s * vx + c * vy


def yaw(psi0, wz, k, dt):
    """psi0 + wz (k dt), as (wz k) dt."""
    return psi0 + (wz * k) * dt


def table(psi0, p0, vx, vy, wz, dt, N):
    """The reference table of B robots: p (B,N+1,2) with p_0 = p0 and p_{k+1} = p_k + v_w(psi0 + wz (k + 1/2) dt) dt summed in order, and
    v (B,N+1,2) = v_w(psi0 + wz k dt)."""
    B = psi0.shape[0]
    p, v = np.zeros((B, N + 1, 2)), np.zeros((B, N + 1, 2))
    p[:, 0] = p0
    for k in range(N + 1):
        v[:, k, 0], v[:, k, 1] = rotate(yaw(psi0, wz, float(k), dt), vx, vy)
        if k < N:
            mx, my = rotate(yaw(psi0, wz, k + 0.5, dt), vx, vy)
            p[:, k + 1, 0] = p[:, k, 0] + mx * dt
            p[:, k + 1, 1] = p[:, k, 1] + my * dt
    return p, v


def mpc_inputs(x0, feet, stamp, command, com_target, N, dt, standing=None, period_steps=6, double_support_steps=1, hip_offset_y=0.0645):
    """The twin of srbdqp_mpc_inputs_steered_*: dict(x_ref (B,N,13), foot (B,N,12), contact (B,N,4), pcom (B,N,3), landing (B,3), landing_yaw (B,))."""
    x0 = np.asarray(x0, np.float64).reshape(-1, 13)
    B = x0.shape[0]
    feet = np.asarray(feet, np.float64).reshape(B, 12)
    cmd = np.asarray(command, np.float64).reshape(B, 3)
    com_target = np.asarray(com_target, np.float64)
    vx, vy, wz = cmd[:, 0], cmd[:, 1], cmd[:, 2]
    psi0 = x0[:, 2]
    with np.errstate(invalid="ignore"):
        p, v = table(psi0, x0[:, 3:5], vx, vy, wz, dt, N)
        # the schedule: cascade_oracle's own, under any velocity
        base = co.mpc_inputs(x0, feet, stamp, np.zeros((B, 2)), com_target, N, dt, standing=standing, period_steps=period_steps,
                             double_support_steps=double_support_steps, hip_offset_y=hip_offset_y)
        contact = base["contact"]
        moving = (vx != 0.0) | (vy != 0.0)
        k1 = np.arange(1, N + 1, dtype=np.float64)
        xr = np.zeros((B, N, 13))
        xr[:, :, 2] = psi0[:, None] + (wz[:, None] * k1[None, :]) * dt
        xr[:, :, 3] = np.where(moving[:, None], p[:, 1:, 0], com_target[0])
        xr[:, :, 4] = np.where(moving[:, None], p[:, 1:, 1], com_target[1])
        xr[:, :, 5] = com_target[2]
        xr[:, :, 8] = wz[:, None]
        xr[:, :, 9] = v[:, 1:, 0]
        xr[:, :, 10] = v[:, 1:, 1]
        xr[:, :, 12] = x0[:, None, 12]
        pcom = np.concatenate([p[:, :N], np.repeat(x0[:, None, 5:6], N, axis=1)], axis=2)
        half_T = 0.5 * (period_steps * dt)
        psi_l = psi0 + wz * half_T
        side = np.where(contact[:, 0, 0] == 0, 1.0, -1.0)
        s, c, o = np.sin(psi_l), np.cos(psi_l), side * hip_offset_y
        landing = np.zeros((B, 3))
        landing[:, 0] = ((x0[:, 3] + (0.0 - s * o)) + half_T * x0[:, 9]) + 0.03 * (x0[:, 9] - v[:, 0, 0])
        landing[:, 1] = ((x0[:, 4] + c * o) + half_T * x0[:, 10]) + 0.03 * (x0[:, 10] - v[:, 0, 1])
    return dict(x_ref=xr, foot=base["foot"], contact=contact, pcom=pcom, landing=landing, landing_yaw=psi_l)


def touchdown(landing, landing_yaw, half):
    """heel, toe (B,3) around landing (B,3) along the heading landing_yaw (B,): z is landing's."""
    landing = np.asarray(landing, np.float64).reshape(-1, 3)
    psi = np.asarray(landing_yaw, np.float64).reshape(-1)
    hx, hy = half * np.cos(psi), half * np.sin(psi)
    heel, toe = landing.copy(), landing.copy()
    heel[:, 0], heel[:, 1] = landing[:, 0] - hx, landing[:, 1] - hy
    toe[:, 0], toe[:, 1] = landing[:, 0] + hx, landing[:, 1] + hy
    return heel, toe


def advance(params, x, feet, stamp, u0, landing, landing_yaw, terrain=None, **kw):
    """The twin of srbdqp_fleet_advance_steered_*: fleet_twin.advance -- on a map (terrain: a terrain_twin.Map) terrain_twin.advance --, whose plant, clock,
    touchdown decisions and fallen flags it keeps, with the foot that moved put down turned: heel and toe along landing_yaw, z landing's on flat ground and the
    map's sample under each of the two turned points on a map.  Returns fleet_twin.advance's dict."""
    if terrain is None:
        r = ft.advance(params, x, feet, stamp, u0, landing, **kw)
    else:
        import terrain_twin as tt
        r = tt.advance(terrain, params, x, feet, stamp, u0, landing, **kw)
    s = dict(ft.DEFAULTS, **{k: v for k, v in kw.items() if k in ft.DEFAULTS})
    heel, toe = touchdown(landing, landing_yaw, s["foot_half_length"])
    if terrain is not None:
        heel[:, 2], toe[:, 2] = tt.sample(terrain, heel[:, 0:2])[0], tt.sample(terrain, toe[:, 0:2])[0]
    for b in np.flatnonzero(r["moved"]):
        c0 = 0 if r["moved"][b] == 1 else 6
        r["feet"][b, c0:c0 + 3], r["feet"][b, c0 + 3:c0 + 6] = heel[b], toe[b]
    return r


def rollout(params, x0, feet, stamp, command, steps, com_target, standing=None, push=None, alive=None, solver="c", horizon=10, **settings):
    """The twin of srbdqp_fleet_rollout_steered_* on flat ground without an observer: command (B,3) held, or (steps,B,3) with step t reading row t.
    Returns fleet_twin.rollout's dict and landing_yaw (T,B)."""
    s = dict(ft.DEFAULTS, **settings)
    x = np.array(x0, np.float64).reshape(-1, 13)
    B, N = x.shape[0], int(horizon)
    feet = np.array(feet, np.float64).reshape(B, 12)
    stamp = np.array(stamp, np.float64).reshape(B)
    alive = np.ones(B, np.uint8) if alive is None else np.array(np.asarray(alive) != 0, np.uint8).reshape(B)
    command = np.asarray(command, np.float64)
    xs, fs, us, st, it, lps, lys = [x.copy()], [feet.copy()], [], [], [], [], []
    for t in range(steps):
        inp = mpc_inputs(x, feet, stamp, command if command.ndim == 2 else command[t], com_target, N, params.dt, standing=standing, period_steps=s["period_steps"],
                         double_support_steps=s["double_support_steps"], hip_offset_y=s["hip_offset_y"])
        sol = ft.solve(params, x, inp, solver)
        r = advance(params, x, feet, stamp, sol["u0"], inp["landing"], inp["landing_yaw"], standing=standing, push=None if push is None else push[t], alive=alive,
                    **settings)
        x, feet, stamp, alive = r["x"], r["feet"], r["stamp"], r["alive"]
        xs.append(x.copy()); fs.append(feet.copy()); us.append(sol["u0"]); st.append(sol["status"]); it.append(sol["iters"])
        lps.append(inp["landing"]); lys.append(inp["landing_yaw"])
    return dict(x=np.array(xs), u0=np.array(us), feet=np.array(fs), status=np.array(st), iters=np.array(it), landing=np.array(lps), landing_yaw=np.array(lys),
                alive=alive, stamp=stamp)


def fleet():
    """The six robots of the steering tests: the commands of DESIGN.md section 20, all walking, stamps staggered as in fleet_twin.fleet()."""
    f = ft.fleet()
    f.pop("v_ref")
    f["standing"] = np.zeros(6, np.uint8)
    f["command"] = COMMANDS.copy()
    return f
