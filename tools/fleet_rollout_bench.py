"""Throughput of the fleet roll-out (include/srbdqp_cascade.h srbdqp_fleet_rollout_device_f64): B = 4096 walking robots, N = 10, T = 100.

  * robot-steps/s of ONE roll-out call (T steps enqueued without a host synchronisation);
  * the same T steps driven from Python through the three public device calls with a synchronise after every step (what a user had to write before);
  * the plant step alone (srbdqp_fleet_advance_device_f64): time per launch, its share of a step of the roll-out, and its GB/s beside the 4.4 TB/s DESIGN.md
    section 8 quotes for mpc_inputs (it integrates 40 derivative evaluations per robot: it is not expected to sit at the HBM roof).

--terrain: the same fleet on rolling ground -- a height map 0.08 sin(1.5 x) cos(1.2 y) m on a 0.1 m grid, the robots spread over 4 m x
4 m of it with their feet on the ground --, the Python loop with the inputs step (terrain_inputs_device, set_contact_normals) in it.  --kernel wrench: the flat
roll-out on a SRBDQP_KERNEL_WRENCH handle, the solve family a terrain roll-out runs: the difference between the two is the cost of the terrain; the default flat
roll-out beside them gives the cost of leaving the one-wave kernel.

--observer: the observed roll-out -- the solves on wrench_f64_n10_ew under the momentum observer's estimate, one observer launch behind
every plant step --, the Python loop with the observer and the wrench buffer in it (set_external_wrench on the device buffer, once), and the observer alone: time
per launch and GB/s.  Beside --kernel wrench in the same job: the cost of observing.

--steer: the steered roll-out -- the same fleet under (vx, vy, wz) commands, wz uniform in +-0.6 rad/s, the velocities of the unsteered
run taken in the heading frame --, the Python loop through mpc_inputs_steered_device and fleet_advance_device(landing_yaw=), and the steered inputs kernel
alone: time per launch and GB/s, with mpc_inputs measured the same way beside it.  Combines with --terrain and --observer.

--track: the tracked roll-out -- --steer's fleet and commands with a reference pose carried from step to step, from the measured pose,
under the default bounds --, the Python loop through mpc_inputs_tracked_device, and the tracked inputs kernel alone beside the other two: time per launch, GB/s
and its share of a step; the fleet's distance from the path its commands lead along, beside what --steer leaves.  Implies --steer's commands.

--preview: the previewed roll-out of --steer's or --track's fleet -- rollout_device(preview=True), the Python loop through
mpc_inputs_previewed_device (and on a map terrain_inputs_previewed_device), and the previewed inputs kernel alone beside the others.

    python tools/fleet_rollout_bench.py [--robots 4096] [--steps 100] [--reps 5] [--terrain] [--observer] [--steer] [--track] [--preview] [--kernel auto|wrench] [--out profiles/<name>.json]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FEET = np.array([[0.0, 0.0645, 0.0], [0.17, 0.0645, 0.0], [0.0, -0.0645, 0.0], [0.17, -0.0645, 0.0]])
COM = np.array([0.085, 0.0, 0.598])
# bytes the plant step must move per robot: x, feet, u0, landing, stamp, push in; x, stamp out (a foothold is stored at a touchdown only: one period in six)
ADVANCE_BYTES = (13 + 12 + 12 + 3 + 1 + 6 + 13 + 1) * 8
# ... and the observer, beside the N 6 doubles of the horizon's wrench: two states, feet, u0, w_est in; w_est out
OBSERVER_BYTES = (13 + 13 + 12 + 12 + 6 + 6) * 8
# ... and the inputs step, beside the N (13 + 12 + 3) doubles and N 4 bytes of the horizons: x0, feet, stamp, the command (2 or 3 doubles) in; landing (3, and its heading) out
INPUTS_BYTES = (13 + 12 + 1 + 3) * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--terrain", action="store_true")
    ap.add_argument("--observer", action="store_true")
    ap.add_argument("--steer", action="store_true")
    ap.add_argument("--track", action="store_true")
    ap.add_argument("--preview", action="store_true")
    ap.add_argument("--kernel", choices=("auto", "wrench"), default="auto")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.terrain and a.observer:
        ap.error("--observer is flat ground: no roll-out reads normals beside a wrench")
    a.steer = a.steer or a.track or a.preview                             # (a path and a preview need commands)
    import torch
    from g1_locomotion_amd import BatchMPC, _lib
    B, T, N, dt = a.robots, a.steps, 10, 0.04
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    x0 = np.zeros((B, 13)); x0[:, 3:6] = COM + rng.normal(size=(B, 3)) * 0.003; x0[:, 12] = -9.80665
    feet0 = np.tile(FEET.reshape(12), (B, 1))
    if a.terrain:                                                         # (the flat runs draw exactly what they drew before)
        at = np.random.default_rng(1).uniform(-2.0, 2.0, (B, 2))
        x0[:, 3:5] += at
        feet0 = (FEET[None, :, :] + np.concatenate([at, np.zeros((B, 1))], 1)[:, None, :]).reshape(B, 12)
    stamp0 = dt * rng.integers(0, 12, B).astype(np.float64)
    v_ref = rng.uniform(-1.0, 1.0, (B, 2)) * np.array([0.3, 0.1])
    push = np.where(rng.random((T, B, 1)) < 0.05, rng.uniform(-1.0, 1.0, (T, B, 6)) * np.array([2.0, 2.0, 0.0, 30.0, 30.0, 10.0]), 0.0)
    up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    d_v, d_pu = up(v_ref), up(push)
    # (drawn behind everything the unsteered runs draw: they draw exactly what they drew before)
    d_cm = up(np.concatenate([v_ref, rng.uniform(-0.6, 0.6, (B, 1))], axis=1)) if a.steer else None
    ly = torch.empty(B, dtype=torch.float64, device=dev) if a.steer else None
    steer = dict(command=d_cm.data_ptr(), command_steps=1) if a.steer else {}
    # the pose starts on the robot; pose_log: where the commands have led, as far as the bounds let it
    pose0 = np.concatenate([x0[:, 3:5], x0[:, 2:3]], axis=1)
    d_po, d_pl = (torch.empty((B, 3), dtype=torch.float64, device=dev), torch.empty((T, B, 3), dtype=torch.float64, device=dev)) if a.track else (None, None)
    if a.track:
        steer.update(track=True, pose=d_po.data_ptr(), pose_log=d_pl.data_ptr())
    if a.preview:
        steer.update(preview=True)
    pvw = torch.empty((B, N, 4), dtype=torch.uint8, device=dev) if a.preview else None
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    xl, ul, fl = f64(T + 1, B, 13), f64(T, B, 12), f64(T + 1, B, 12)
    sl, il = torch.empty((T, B), dtype=torch.int32, device=dev), torch.empty((T, B), dtype=torch.int32, device=dev)
    xr, fo, pc, lp, u, xo = f64(B, N, 13), f64(B, N, 12), f64(B, N, 3), f64(B, 3), f64(B, N, 12), f64(B, N + 1, 13)
    ct = torch.empty((B, N, 4), dtype=torch.uint8, device=dev)
    st, it = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    res = dict(robots=B, steps=T, horizon=N, reps=a.reps, terrain=bool(a.terrain), observer=bool(a.observer), steer=bool(a.steer), track=bool(a.track),
               preview=bool(a.preview), kernel_setting=a.kernel)
    cn = f64(B, N, 12) if a.terrain else None
    we, wl, ew = (f64(B, 6), f64(T, B, 6), f64(B, N, 6)) if a.observer else (None, None, None)
    obs = dict(observer=True, w_est=we.data_ptr(), w_log=wl.data_ptr()) if a.observer else {}
    with BatchMPC(horizon=N, dt=dt, kernel=_lib.KERNEL_WRENCH if a.kernel == "wrench" else _lib.KERNEL_AUTO) as eng:
        if a.terrain:
            gx, gy = -4.0 + 0.1 * np.arange(81), -4.0 + 0.1 * np.arange(81)
            eng.set_terrain(0.08 * np.sin(1.5 * gx)[None, :] * np.cos(1.2 * gy)[:, None], origin=(-4.0, -4.0), cell=0.1)
            fz = feet0.reshape(B * 4, 3)
            fz[:, 2] = eng.terrain_sample(fz[:, 0:2], want_normal=False)["z"]
            feet0 = fz.reshape(B, 12)
            x0[:, 5] += eng.terrain_sample(x0[:, 3:5], want_normal=False)["z"]

        def fresh():
            return up(x0), up(feet0), up(stamp0), torch.ones(B, dtype=torch.uint8, device=dev)

        def call():
            x, feet, stamp, al = fresh()
            if a.observer:
                we.zero_()
            if a.track:
                d_po.copy_(up(pose0))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.rollout_device(B, T, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), 0 if a.steer else d_v.data_ptr(), COM, push=d_pu.data_ptr(), alive=al.data_ptr(),
                               x_log=xl.data_ptr(), u0_log=ul.data_ptr(), feet_log=fl.data_ptr(), status_log=sl.data_ptr(), iters_log=il.data_ptr(), **obs, **steer)
            t1 = time.perf_counter()
            eng.synchronize()
            return time.perf_counter() - t0, t1 - t0, al

        def loop():
            x, feet, stamp, al = fresh()
            if a.observer:
                we.zero_(); ew.zero_()
                xp, fp = torch.empty_like(x), torch.empty_like(feet)
                eng.set_external_wrench(ew)
            if a.track:
                d_po.copy_(up(pose0))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(T):
                if a.preview:
                    eng.mpc_inputs_previewed_device(B, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), d_cm.data_ptr(), COM, xr.data_ptr(), fo.data_ptr(), ct.data_ptr(),
                                                    pc.data_ptr(), landing=lp.data_ptr(), landing_yaw=ly.data_ptr(), pose=d_po.data_ptr() if a.track else 0,
                                                    previewed=pvw.data_ptr())
                elif a.track:
                    eng.mpc_inputs_tracked_device(B, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), d_cm.data_ptr(), d_po.data_ptr(), COM, xr.data_ptr(), fo.data_ptr(),
                                                  ct.data_ptr(), pc.data_ptr(), landing=lp.data_ptr(), landing_yaw=ly.data_ptr())
                elif a.steer:
                    eng.mpc_inputs_steered_device(B, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), d_cm.data_ptr(), COM, xr.data_ptr(), fo.data_ptr(), ct.data_ptr(),
                                                  pc.data_ptr(), landing=lp.data_ptr(), landing_yaw=ly.data_ptr())
                else:
                    eng.mpc_inputs_device(B, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), d_v.data_ptr(), COM, xr.data_ptr(), fo.data_ptr(), ct.data_ptr(),
                                          pc.data_ptr(), landing=lp.data_ptr())
                if a.terrain:
                    if a.preview:
                        eng.terrain_inputs_previewed_device(B, fo.data_ptr(), pvw.data_ptr(), xr.data_ptr(), cn.data_ptr())
                    else:
                        eng.terrain_inputs_device(B, feet.data_ptr(), xr.data_ptr(), cn.data_ptr())
                    eng.set_contact_normals(cn)
                eng.solve_device(B, x.data_ptr(), xr.data_ptr(), fo.data_ptr(), ct.data_ptr(), u.data_ptr(), x_out=xo.data_ptr(), status=st.data_ptr(),
                                 iters=it.data_ptr(), pcom=pc.data_ptr())
                if a.observer:                                            # (the state and the feet before the period: what a user without logs has to keep)
                    xp.copy_(x); fp.copy_(feet)
                eng.fleet_advance_device(B, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), u.data_ptr(), lp.data_ptr(), u0_stride=12 * N,
                                         push=d_pu[k].data_ptr(), alive=al.data_ptr(), landing_yaw=ly.data_ptr() if a.steer else 0)
                if a.observer:
                    eng.wrench_observer_device(B, xp.data_ptr(), x.data_ptr(), fp.data_ptr(), u.data_ptr(), we.data_ptr(), ew=ew.data_ptr(), u0_stride=12 * N,
                                               alive=al.data_ptr())
                eng.synchronize()
            dt_loop = time.perf_counter() - t0
            if a.terrain:
                eng.set_contact_normals(None)
            if a.observer:
                eng.set_external_wrench(None)
            return dt_loop

        def advance_alone():
            x, feet, stamp, al = fresh()
            u.zero_(); u[:, 0, 2::3] = 85.0                               # the robot's weight on four contacts: it stays where it is
            lp.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(T):
                eng.fleet_advance_device(B, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), u.data_ptr(), lp.data_ptr(), u0_stride=12 * N,
                                         push=d_pu[k].data_ptr(), alive=al.data_ptr())
            eng.synchronize()
            return (time.perf_counter() - t0) / T

        call(); loop(); advance_alone()                                   # warm-up: buffers, code objects
        calls = [call() for _ in range(a.reps)]
        t_call = float(np.median([c[0] for c in calls]))
        res["kernel"] = eng.kernel_name()
        if a.terrain:                                                     # the inputs step alone: B (12 + 2 N 13 + N 12) doubles moved per launch
            xs, fs, _, _ = fresh()
            eng.terrain_inputs_device(B, fs.data_ptr(), xr.data_ptr(), cn.data_ptr()); eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(T):
                eng.terrain_inputs_device(B, fs.data_ptr(), xr.data_ptr(), cn.data_ptr())
            eng.synchronize()
            t_in = (time.perf_counter() - t0) / T
            res["terrain_inputs_us_per_launch"] = t_in * 1e6
            res["terrain_inputs_gb_per_s"] = B * (12 + 2 * N * 13 + N * 12) * 8 / t_in / 1e9
        if a.observer:                                                    # the observer alone, on the logs of the last roll-out
            eng.wrench_observer_device(B, xl[0].data_ptr(), xl[1].data_ptr(), fl[0].data_ptr(), ul[0].data_ptr(), we.data_ptr(), ew=ew.data_ptr()); eng.synchronize()
            t0 = time.perf_counter()
            for k in range(T):
                eng.wrench_observer_device(B, xl[k].data_ptr(), xl[k + 1].data_ptr(), fl[k].data_ptr(), ul[k].data_ptr(), we.data_ptr(), ew=ew.data_ptr())
            eng.synchronize()
            t_ob = (time.perf_counter() - t0) / T
            res["observer_us_per_launch"] = t_ob * 1e6
            res["observer_gb_per_s"] = B * (OBSERVER_BYTES + N * 6 * 8) / t_ob / 1e9
            res["observer_share_of_a_rollout_step"] = t_ob / (t_call / T)
            res["w_est_force_rms_N"] = float(wl[:, :, 3:6].pow(2).mean().sqrt().item())
        if a.steer:                                                       # the inputs kernels alone, back to back: the steered one, and mpc_inputs the same way
            xs, fs, ss, _ = fresh()
            per = {}
            if a.track:                                                   # where the commands lead, by the references' own midpoint rule (before the launches below move the pose)
                cm = d_cm.cpu().numpy()
                q = pose0.copy()
                for _ in range(T):
                    th = q[:, 2] + (cm[:, 2] * 0.5) * dt
                    q = np.stack([q[:, 0] + (np.cos(th) * cm[:, 0] - np.sin(th) * cm[:, 1]) * dt, q[:, 1] + (np.sin(th) * cm[:, 0] + np.cos(th) * cm[:, 1]) * dt,
                                  q[:, 2] + (cm[:, 2] * 1.0) * dt], axis=1)
                up_ = calls[-1][2].cpu().numpy() != 0
                off = np.hypot(*(xl[T, :, 3:5].cpu().numpy() - q[:, 0:2]).T)[up_]
                res["distance_from_the_path_m_mean"], res["distance_from_the_path_m_max"] = float(off.mean()), float(off.max())
                res["path_length_m_mean"] = float(np.hypot(cm[:, 0], cm[:, 1]).mean() * T * dt)
                res["pose_lead_m_max"] = float(np.hypot(*(d_pl[:-1, :, 0:2] - xl[1:T, :, 3:5]).cpu().numpy()[:, up_].transpose(2, 0, 1)).max())
                res["final_yaw_error_rad_rms"] = float(np.sqrt(np.mean((xl[T, :, 2].cpu().numpy() - q[:, 2])[up_] ** 2)))
            tracked = (("mpc_inputs_tracked", lambda: eng.mpc_inputs_tracked_device(B, xs.data_ptr(), fs.data_ptr(), ss.data_ptr(), d_cm.data_ptr(), d_po.data_ptr(), COM,
                                                                                    xr.data_ptr(), fo.data_ptr(), ct.data_ptr(), pc.data_ptr(), landing=lp.data_ptr(),
                                                                                    landing_yaw=ly.data_ptr())),) if a.track else ()
            if a.preview:
                tracked = (("mpc_inputs_previewed", lambda: eng.mpc_inputs_previewed_device(B, xs.data_ptr(), fs.data_ptr(), ss.data_ptr(), d_cm.data_ptr(), COM, xr.data_ptr(),
                                                                                            fo.data_ptr(), ct.data_ptr(), pc.data_ptr(), landing=lp.data_ptr(),
                                                                                            landing_yaw=ly.data_ptr(), pose=d_po.data_ptr() if a.track else 0,
                                                                                            previewed=pvw.data_ptr())),) + tracked
            for name, launch in tracked + (("mpc_inputs_steered", lambda: eng.mpc_inputs_steered_device(B, xs.data_ptr(), fs.data_ptr(), ss.data_ptr(), d_cm.data_ptr(), COM, xr.data_ptr(),
                                                                                              fo.data_ptr(), ct.data_ptr(), pc.data_ptr(), landing=lp.data_ptr(), landing_yaw=ly.data_ptr())),
                                 ("mpc_inputs", lambda: eng.mpc_inputs_device(B, xs.data_ptr(), fs.data_ptr(), ss.data_ptr(), d_v.data_ptr(), COM, xr.data_ptr(), fo.data_ptr(),
                                                                              ct.data_ptr(), pc.data_ptr(), landing=lp.data_ptr()))):
                launch(); eng.synchronize()
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    for _ in range(T):
                        launch()
                    eng.synchronize()
                    ts.append((time.perf_counter() - t0) / T)
                per[name] = float(np.median(ts))
                res[name + "_us_per_launch"] = per[name] * 1e6
                res[name + "_gb_per_s"] = B * (INPUTS_BYTES + (48 if name == "mpc_inputs_tracked" or (name == "mpc_inputs_previewed" and a.track) else 0) + (N * 4 if name == "mpc_inputs_previewed" else 0) + N * (13 + 12 + 3) * 8 + N * 4) / per[name] / 1e9
            res["mpc_inputs_steered_share_of_a_rollout_step"] = per["mpc_inputs_steered"] / (t_call / T)
            if a.preview:
                res["mpc_inputs_previewed_share_of_a_rollout_step"] = per["mpc_inputs_previewed"] / (t_call / T)
            if a.track:
                res["mpc_inputs_tracked_share_of_a_rollout_step"] = per["mpc_inputs_tracked"] / (t_call / T)
            res["final_yaw_rms_error_rad"] = float((xl[T, :, 2] - xl[0, :, 2] - d_cm[:, 2] * (T * dt)).pow(2).mean().sqrt().item())
        res["rollout_call_s"] = t_call
        res["rollout_enqueue_s"] = float(np.median([c[1] for c in calls]))
        res["rollout_robot_steps_per_s"] = B * T / t_call
        t_loop = float(np.median([loop() for _ in range(a.reps)]))
        res["python_loop_s"] = t_loop
        res["python_loop_robot_steps_per_s"] = B * T / t_loop
        t_adv = float(np.median([advance_alone() for _ in range(a.reps)]))
        res["advance_us_per_launch"] = t_adv * 1e6
        res["advance_share_of_a_rollout_step"] = t_adv / (t_call / T)
        res["advance_gb_per_s"] = B * ADVANCE_BYTES / t_adv / 1e9
        res["advance_bytes_per_robot"] = ADVANCE_BYTES
        res["mpc_inputs_gb_per_s_design_8"] = 4400.0
        res["alive_share"] = float(calls[-1][2].float().mean().item())
        res["solved_share"] = float((sl == 1).float().mean().item())
        res["mean_iters"] = float(il.float().mean().item())
    res["library_sha256"] = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
