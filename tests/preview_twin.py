"""Test helper: the NumPy twin of the previewed fleet calls (include/srbdqp_cascade.h srbdqp_mpc_inputs_previewed_*, srbdqp_terrain_inputs_previewed_*,
srbdqp_fleet_rollout_previewed_*), built on steer_twin, track_twin and terrain_twin: the same operations in the same order as the header
states them.  It is the specification the device is held to.

A previewed call is the steered call (pose None) or the tracked call (a pose) with foot[b][k] holding, for a foot that lands inside the horizon, the heel and toe
it will land on from that step on."""
import numpy as np

import fleet_twin as ft
import steer_twin as stw
import track_twin as ttw

HALF = 0.085


def phase0(stamp, dt, period_steps):
    """The phase of horizon step 0 in [0, 2 P): the gait's clock is the step index floor(stamp / dt + 1e-9)."""
    k0 = np.floor(np.asarray(stamp, np.float64) / dt + 1e-9).astype(np.int64)
    return k0 % (2 * period_steps)


def lands(p0, j, period_steps, double_support_steps):
    """The foot that touches down at horizon step j: 0 none, 1 the left, 2 the right; p0 < 0: standing."""
    if p0 < 0 or double_support_steps >= period_steps or j < 1:
        return 0
    ph = (p0 + j) % (2 * period_steps)
    return 1 if ph == 0 else (2 if ph == period_steps else 0)


def touchdown(p0, k, period_steps, double_support_steps, right):
    """The latest touchdown step j in [1, k] of the left (right: the right) foot in closed form, or 0."""
    if p0 < 0 or double_support_steps >= period_steps:
        return 0
    j = k - (p0 + k + (period_steps if right else 0)) % (2 * period_steps)
    return j if j >= 1 else 0


def foothold(psi, px, py, vx, vy, vwx, vwy, wz, side, hip_offset_y, half_T, half):
    """heel (2,), toe (2,), psi_l of a touchdown from the predicted state (heading psi, position, velocity, the command's velocity there): steer_twin's landing
    point and turned touchdown, one rounded operation at a time."""
    psi_l = psi + wz * half_T
    s, c, o = np.sin(psi_l), np.cos(psi_l), side * hip_offset_y
    lx = ((px + (0.0 - s * o)) + half_T * vx) + 0.03 * (vx - vwx)
    ly = ((py + c * o) + half_T * vy) + 0.03 * (vy - vwy)
    hx, hy = half * np.cos(psi_l), half * np.sin(psi_l)
    return np.array([lx - hx, ly - hy]), np.array([lx + hx, ly + hy]), psi_l


def mpc_inputs(x0, feet, stamp, command, com_target, N, dt, pose=None, standing=None, period_steps=6, double_support_steps=1, hip_offset_y=0.0645,
               foot_half_length=HALF, **track):
    """The twin of srbdqp_mpc_inputs_previewed_*: steer_twin.mpc_inputs' dict (pose None) or track_twin.mpc_inputs' (a pose; track: lead_max, yaw_lead_max) with
    foot previewed, previewed (B,N,4) uint8, and -- for the tests -- psi_l (B,N): the landing heading of the touchdown at step j, NaN where there is none."""
    x0 = np.asarray(x0, np.float64).reshape(-1, 13)
    B = x0.shape[0]
    cmd = np.asarray(command, np.float64).reshape(B, 3)
    kw = dict(standing=standing, period_steps=period_steps, double_support_steps=double_support_steps, hip_offset_y=hip_offset_y)
    if pose is None:
        out = stw.mpc_inputs(x0, feet, stamp, cmd, com_target, N, dt, **kw)
    else:
        out = ttw.mpc_inputs(x0, feet, stamp, cmd, pose, com_target, N, dt, **kw, **track)
    P, ds = int(period_steps), int(double_support_steps)
    p0 = phase0(stamp, dt, P).reshape(B)
    if standing is not None:
        p0 = np.where(np.asarray(standing).reshape(B) != 0, -1, p0)
    foot = np.array(out["foot"], np.float64).reshape(B, N, 12)
    previewed = np.zeros((B, N, 4), np.uint8)
    psi_log = np.full((B, N), np.nan)
    half_T = 0.5 * (P * dt)
    with np.errstate(invalid="ignore", over="ignore"):
        # the measured state's table, in tracked calls too: p_k = pcom[k], v_w(psi0 + wz k dt)
        p, v = stw.table(x0[:, 2], x0[:, 3:5], cmd[:, 0], cmd[:, 1], cmd[:, 2], dt, N)
        for b in range(B):
            wz = cmd[b, 2]
            spots = {}
            for j in range(1, N):
                f = lands(int(p0[b]), j, P, ds)
                if not f:
                    continue
                if j == 1:    # the measured state itself
                    psi, vx, vy = x0[b, 2], x0[b, 9], x0[b, 10]
                else:
                    psi, vx, vy = stw.yaw(x0[b, 2], wz, float(j - 1), dt), v[b, j - 1, 0], v[b, j - 1, 1]
                heel, toe, psi_l = foothold(psi, p[b, j - 1, 0], p[b, j - 1, 1], vx, vy, v[b, j - 1, 0], v[b, j - 1, 1], wz, 1.0 if f == 1 else -1.0, hip_offset_y,
                                            half_T, foot_half_length)
                spots[j] = (heel, toe)
                psi_log[b, j] = psi_l
            for k in range(N):
                for right in (False, True):
                    j = touchdown(int(p0[b]), k, P, ds, right)
                    if j:
                        c0 = 6 if right else 0
                        foot[b, k, c0:c0 + 3] = (spots[j][0][0], spots[j][0][1], 0.0)
                        foot[b, k, c0 + 3:c0 + 6] = (spots[j][1][0], spots[j][1][1], 0.0)
                        previewed[b, k, (2 if right else 0):(4 if right else 2)] = 1
    out.update(foot=foot, previewed=previewed, psi_l=psi_log)
    return out


def terrain_inputs(m, foot, previewed, x_ref):
    """The twin of srbdqp_terrain_inputs_previewed_*: foot (B,N,12), previewed (B,N,4) or None, x_ref (B,N,13) -> dict(foot, x_ref, normals (B,N,12))."""
    import terrain_twin as tt
    x_ref = np.array(x_ref, np.float64)
    B, N = x_ref.shape[0], x_ref.shape[1]
    foot = np.array(foot, np.float64).reshape(B, N, 4, 3)
    pv = np.zeros((B, N, 4), bool) if previewed is None else np.asarray(previewed).reshape(B, N, 4) != 0
    z, n = tt.sample(m, foot.reshape(-1, 3)[:, 0:2])
    foot[:, :, :, 2] = np.where(pv, z.reshape(B, N, 4), foot[:, :, :, 2])
    zz = foot[:, :, :, 2]
    with np.errstate(invalid="ignore"):
        x_ref[:, :, 5] = x_ref[:, :, 5] + (((zz[:, :, 0] + zz[:, :, 1]) + zz[:, :, 2]) + zz[:, :, 3]) * 0.25
    return dict(foot=foot.reshape(B, N, 12), x_ref=x_ref, normals=n.reshape(B, N, 12))


def rollout(params, x0, feet, stamp, command, steps, com_target, pose=None, track=False, terrain=None, standing=None, push=None, alive=None, solver="c",
            horizon=10, preview=True, lead_max=0.1, yaw_lead_max=0.3, **settings):
    """The twin of srbdqp_fleet_rollout_previewed_* without an observer, on flat ground or on a map (terrain: a terrain_twin.Map): steer_twin.rollout -- with
    track, track_twin.rollout -- with the previewed inputs.  preview=False: the same loop with the plain inputs (the roll-out as it was), for comparisons.
    Returns steer_twin.rollout's dict, foot (T,B,N,12) and previewed (T,B,N,4): what each solve read, and with track pose and pose_log."""
    s = dict(ft.DEFAULTS, **settings)
    x = np.array(x0, np.float64).reshape(-1, 13)
    B, N = x.shape[0], int(horizon)
    feet = np.array(feet, np.float64).reshape(B, 12)
    stamp = np.array(stamp, np.float64).reshape(B)
    alive = np.ones(B, np.uint8) if alive is None else np.array(np.asarray(alive) != 0, np.uint8).reshape(B)
    command = np.asarray(command, np.float64)
    if track:
        pose = ttw.start_pose(x) if pose is None else np.array(pose, np.float64).reshape(B, 3)
    xs, fs, us, st, it, lps, lys, pl, fo, pv = [x.copy()], [feet.copy()], [], [], [], [], [], [], [], []
    for t in range(steps):
        inp = mpc_inputs(x, feet, stamp, command if command.ndim == 2 else command[t], com_target, N, params.dt, pose=pose if track else None, standing=standing,
                         period_steps=s["period_steps"], double_support_steps=s["double_support_steps"], hip_offset_y=s["hip_offset_y"],
                         foot_half_length=s["foot_half_length"], **(dict(lead_max=lead_max, yaw_lead_max=yaw_lead_max) if track else {}))
        if not preview:
            inp["foot"] = np.repeat(feet[:, None, :], N, axis=1)
            inp["previewed"] = np.zeros((B, N, 4), np.uint8)
        if track:
            pose = inp["pose"]
        if terrain is None:
            sol = ft.solve(params, x, inp, solver)
        else:
            import terrain_twin as tt
            ti = terrain_inputs(terrain, inp["foot"], inp["previewed"], inp["x_ref"])
            inp = dict(inp, foot=ti["foot"], x_ref=ti["x_ref"])
            sol = tt.solve(params, x, inp, ti["normals"])
        r = stw.advance(params, x, feet, stamp, sol["u0"], inp["landing"], inp["landing_yaw"], terrain=terrain, standing=standing,
                        push=None if push is None else push[t], alive=alive, **settings)
        x, feet, stamp, alive = r["x"], r["feet"], r["stamp"], r["alive"]
        xs.append(x.copy()); fs.append(feet.copy()); us.append(sol["u0"]); st.append(sol["status"]); it.append(sol["iters"])
        lps.append(inp["landing"]); lys.append(inp["landing_yaw"]); fo.append(inp["foot"]); pv.append(inp["previewed"])
        if track:
            pl.append(pose.copy())
    out = dict(x=np.array(xs), u0=np.array(us), feet=np.array(fs), status=np.array(st), iters=np.array(it), landing=np.array(lps), landing_yaw=np.array(lys),
               alive=alive, stamp=stamp, foot=np.array(fo), previewed=np.array(pv))
    if track:
        out.update(pose=pose, pose_log=np.array(pl))
    return out
