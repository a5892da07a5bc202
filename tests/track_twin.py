"""Test helper: the NumPy twin of the tracked fleet calls (include/srbdqp_cascade.h srbdqp_mpc_inputs_tracked_*, srbdqp_fleet_rollout_tracked_*; DESIGN.md
section 21), built on steer_twin: the same operations in the same order as the header states them.  It is the specification the device is held to.

A tracked robot has a pose (qx, qy, th): a planar reference position and an unwrapped reference heading, carried from step to step."""
import numpy as np

import fleet_twin as ft
import steer_twin as stw

DEFAULTS = dict(lead_max=0.1, yaw_lead_max=0.3)


def start_pose(x0):
    """The pose a roll-out starts from where the caller has none: the measured (x0[3], x0[4], x0[2])."""
    x0 = np.asarray(x0, np.float64).reshape(-1, 13)
    return np.concatenate([x0[:, 3:5], x0[:, 2:3]], axis=1)


def bound(pose, x0, lead_max=0.1, yaw_lead_max=0.3):
    """Step 1: the pose (B,3) pulled back to within lead_max of x0[3:5] along the same direction, and to within yaw_lead_max of x0[2].  Every comparison is
    false on a NaN.  Returns (pose (B,3), engaged (B,2) bool: the position bound, the yaw bound)."""
    x0 = np.asarray(x0, np.float64).reshape(-1, 13)
    q = np.array(pose, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = q[:, 0] - x0[:, 3], q[:, 1] - x0[:, 4]
        n = np.sqrt(dx * dx + dy * dy)
        far = n > lead_max
        s = lead_max / np.where(far, n, 1.0)
        q[:, 0] = np.where(far, x0[:, 3] + dx * s, q[:, 0])
        q[:, 1] = np.where(far, x0[:, 4] + dy * s, q[:, 1])
        dth = q[:, 2] - x0[:, 2]
        hi, lo = dth > yaw_lead_max, dth < -yaw_lead_max
        q[:, 2] = np.where(hi, x0[:, 2] + yaw_lead_max, np.where(lo, x0[:, 2] - yaw_lead_max, q[:, 2]))
    return q, np.stack([far, hi | lo], axis=1)


def mpc_inputs(x0, feet, stamp, command, pose, com_target, N, dt, standing=None, period_steps=6, double_support_steps=1, hip_offset_y=0.0645, lead_max=0.1,
               yaw_lead_max=0.3):
    """The twin of srbdqp_mpc_inputs_tracked_*: steer_twin.mpc_inputs' dict with x_ref from the pose, and pose (B,3) behind the step, bounded (B,3) as it stood
    after step 1, engaged (B,2)."""
    x0 = np.asarray(x0, np.float64).reshape(-1, 13)
    B = x0.shape[0]
    cmd = np.asarray(command, np.float64).reshape(B, 3)
    com_target = np.asarray(com_target, np.float64)
    vx, vy, wz = cmd[:, 0], cmd[:, 1], cmd[:, 2]
    # 3. what belongs to where the robot is: the steered call's
    out = stw.mpc_inputs(x0, feet, stamp, cmd, com_target, N, dt, standing=standing, period_steps=period_steps, double_support_steps=double_support_steps,
                         hip_offset_y=hip_offset_y)
    # 1. the bound
    q, engaged = bound(pose, x0, lead_max, yaw_lead_max)
    th = q[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        # 2. the references from the pose
        p, v = stw.table(th, q[:, 0:2], vx, vy, wz, dt, N)
        k1 = np.arange(1, N + 1, dtype=np.float64)
        xr = np.zeros((B, N, 13))
        xr[:, :, 2] = th[:, None] + (wz[:, None] * k1[None, :]) * dt
        xr[:, :, 3] = p[:, 1:, 0]
        xr[:, :, 4] = p[:, 1:, 1]
        xr[:, :, 5] = com_target[2]
        xr[:, :, 8] = wz[:, None]
        xr[:, :, 9] = v[:, 1:, 0]
        xr[:, :, 10] = v[:, 1:, 1]
        xr[:, :, 12] = x0[:, None, 12]
        # 4. the pose moves on, where all three of its values stay finite
        nxt = np.stack([p[:, 1, 0], p[:, 1, 1], stw.yaw(th, wz, 1.0, dt)], axis=1)
    ok = np.isfinite(nxt).all(axis=1)
    out.update(x_ref=xr, pose=np.where(ok[:, None], nxt, q), bounded=q, engaged=engaged)
    return out


def rollout(params, x0, feet, stamp, command, steps, com_target, pose=None, standing=None, push=None, alive=None, solver="c", horizon=10, lead_max=0.1,
            yaw_lead_max=0.3, **settings):
    """The twin of srbdqp_fleet_rollout_tracked_* on flat ground without an observer: steer_twin.rollout with the tracked inputs.  pose (B,3) or None (the
    measured pose).  Returns steer_twin.rollout's dict, pose (B,3), pose_log (T,B,3): the pose behind step t, and engaged (T,B,2)."""
    s = dict(ft.DEFAULTS, **settings)
    x = np.array(x0, np.float64).reshape(-1, 13)
    B, N = x.shape[0], int(horizon)
    feet = np.array(feet, np.float64).reshape(B, 12)
    stamp = np.array(stamp, np.float64).reshape(B)
    alive = np.ones(B, np.uint8) if alive is None else np.array(np.asarray(alive) != 0, np.uint8).reshape(B)
    command = np.asarray(command, np.float64)
    pose = start_pose(x) if pose is None else np.array(pose, np.float64).reshape(B, 3)
    xs, fs, us, st, it, lps, lys, pl, en = [x.copy()], [feet.copy()], [], [], [], [], [], [], []
    for t in range(steps):
        inp = mpc_inputs(x, feet, stamp, command if command.ndim == 2 else command[t], pose, com_target, N, params.dt, standing=standing,
                         period_steps=s["period_steps"], double_support_steps=s["double_support_steps"], hip_offset_y=s["hip_offset_y"], lead_max=lead_max,
                         yaw_lead_max=yaw_lead_max)
        pose = inp["pose"]
        sol = ft.solve(params, x, inp, solver)
        r = stw.advance(params, x, feet, stamp, sol["u0"], inp["landing"], inp["landing_yaw"], standing=standing, push=None if push is None else push[t],
                        alive=alive, **settings)
        x, feet, stamp, alive = r["x"], r["feet"], r["stamp"], r["alive"]
        xs.append(x.copy()); fs.append(feet.copy()); us.append(sol["u0"]); st.append(sol["status"]); it.append(sol["iters"])
        lps.append(inp["landing"]); lys.append(inp["landing_yaw"]); pl.append(pose.copy()); en.append(inp["engaged"])
    return dict(x=np.array(xs), u0=np.array(us), feet=np.array(fs), status=np.array(st), iters=np.array(it), landing=np.array(lps), landing_yaw=np.array(lys),
                alive=alive, stamp=stamp, pose=pose, pose_log=np.array(pl), engaged=np.array(en))


def ideal_path(x0, command, steps, dt):
    """Where the commands lead: (T+1,B,3) = (x, y, yaw), the commands integrated from the initial state by the references' own midpoint rule --
    p_{t+1} = p_t + v_w(yaw_t + (wz 1/2) dt) dt, yaw_{t+1} = yaw_t + (wz 1) dt.  command (B,3) or (T,B,3)."""
    x0 = np.asarray(x0, np.float64).reshape(-1, 13)
    command = np.asarray(command, np.float64)
    path = [start_pose(x0)]
    for t in range(steps):
        c = command if command.ndim == 2 else command[t]
        q = path[-1]
        mx, my = stw.rotate(stw.yaw(q[:, 2], c[:, 2], 0.5, dt), c[:, 0], c[:, 1])
        path.append(np.stack([q[:, 0] + mx * dt, q[:, 1] + my * dt, stw.yaw(q[:, 2], c[:, 2], 1.0, dt)], axis=1))
    return np.array(path)
