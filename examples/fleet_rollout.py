"""256 walking robots under random commands and random pushes for 100 control steps, in one call (BatchMPC.rollout):
prints the share of the fleet still on its feet and how well it follows the commanded velocity.

    python examples/fleet_rollout.py [--robots 256] [--steps 100] [--seed 0] [--slope 0.2] [--observer] [--yaw-rate 0.5] [--track] [--preview]

--slope s: the same fleet on the plane z = s x (BatchMPC.set_terrain): the friction pyramids tilt with the ground, a foot lands on it,
and "fallen" is the height over it.
--observer: on flat ground, a push of 10 N along x and -25 N along y on every robot during steps 5 to 29, once blind and once with the momentum observer
(BatchMPC.rollout(observer=True)): prints how far the push carried the fleet sideways in either run.
--yaw-rate W: a fleet that steers (BatchMPC.rollout(command=)) -- every robot walks a circle under (vx, 0, W), vx up to 0.3 m/s in its
own heading frame, the feet landing turned with it: prints the commanded heading W T dt against the heading reached.  With --slope the circle lies on the plane.
--track: the same commands (--yaw-rate 0.3 where none is given) without the pushes, once steered and once tracked (BatchMPC.rollout(command=, track=True);
DESIGN.md section 21) -- the references taken from a pose that moves on with the commands and is kept within 0.1 m and 0.3 rad of the robot: prints how far
either fleet ends from where its commands lead.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FEET = np.array([[0.0, 0.0645, 0.0], [0.17, 0.0645, 0.0], [0.0, -0.0645, 0.0], [0.17, -0.0645, 0.0]])   # heel, toe of the left and the right foot
COM = np.array([0.085, 0.0, 0.598])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--slope", type=float, default=0.0)
    ap.add_argument("--observer", action="store_true")
    ap.add_argument("--yaw-rate", type=float, default=0.0)
    ap.add_argument("--track", action="store_true")
    ap.add_argument("--preview", action="store_true", help="with --yaw-rate or --track: the solves read the footholds previewed along the horizon (rollout(preview=True))")
    a = ap.parse_args()
    if a.observer and a.slope:
        ap.error("--observer is flat ground")
    if a.observer and a.yaw_rate:
        ap.error("--observer and --yaw-rate: one at a time here (BatchMPC.rollout takes both)")
    if a.track and a.observer:
        ap.error("--observer and --track: one at a time here (BatchMPC.rollout takes both)")
    if (a.track or a.preview) and not a.yaw_rate:
        a.yaw_rate = 0.3
    pv = dict(preview=True) if a.preview else {}
    from g1_locomotion_amd import BatchMPC
    rng = np.random.default_rng(a.seed)
    B, T, dt = a.robots, a.steps, 0.04
    x0 = np.zeros((B, 13)); x0[:, 3:6] = COM; x0[:, 12] = -9.80665
    feet = np.tile(FEET.reshape(12), (B, 1))
    stamp = dt * rng.integers(0, 12, B)                                  # anywhere in the gait period
    v_ref = rng.uniform(-1.0, 1.0, (B, 2)) * np.array([0.3, 0.1])
    # a shove of one control period now and then: up to 40 N and 2 N m, on about one robot in twenty per step
    push = np.where(rng.random((T, B, 1)) < 0.05, rng.uniform(-1.0, 1.0, (T, B, 6)) * np.array([2.0, 2.0, 0.0, 40.0, 40.0, 10.0]), 0.0)
    ground = lambda p: a.slope * p[..., 0]
    with BatchMPC(horizon=10, dt=dt) as eng:
        if a.slope:
            # a sampled plane: 41 x 41 nodes 0.5 m apart around the start (a robot that leaves the map walks on its clamped edge); everything stands on it
            gx = -10.0 + 0.5 * np.arange(41)
            eng.set_terrain(np.tile(a.slope * gx, (41, 1)), origin=(-10.0, -10.0), cell=0.5)
            feet.reshape(B, 4, 3)[:, :, 2] = ground(feet.reshape(B, 4, 3))
            x0[:, 5] += ground(x0[:, 3:5])
        if a.observer:
            shove = np.zeros((T, B, 6)); shove[5:30, :, 3] = 10.0; shove[5:30, :, 4] = -25.0
            free = eng.rollout(x0, feet, stamp, v_ref, T, COM)
            blind = eng.rollout(x0, feet, stamp, v_ref, T, COM, push=shove)
            r = eng.rollout(x0, feet, stamp, v_ref, T, COM, push=shove, observer=True)
            for name, q in (("blind", blind), ("observed", r)):
                up = (q["alive"] != 0) & (free["alive"] != 0)
                if not up.any():
                    print(f"{name:9s}: no robot is still up after {T} steps")
                    continue
                print(f"{name:9s}: {np.mean(q['alive'] != 0):.1%} alive, pushed {np.abs(q['x'][-1, up, 4] - free['x'][-1, up, 4]).mean():.3f} m sideways on average, "
                      f"largest roll {np.abs(q['x'][:, up, 0]).max():.3f} rad, {q['iters'].mean():.1f} iterations per QP")
            k = min(29, T - 1)
            print(f"the estimate behind step {k}: force {r['w_log'][k][:, 3:6].mean(0).round(2).tolist()} N (applied: [10.0, -25.0, 0.0])")
        elif a.yaw_rate:
            command = np.stack([np.abs(v_ref[:, 0]), np.zeros(B), np.full(B, a.yaw_rate)], axis=1)
            if a.track:
                # where the commands lead: the pose of a tracked roll-out whose bounds never engage is the commands integrated from the start
                r = eng.rollout(x0, feet, stamp, None, T, COM, command=command, track=True, **pv)
                goal = eng.rollout(x0, feet, stamp, None, T, COM, command=command, track=dict(lead_max=1e9, yaw_lead_max=1e9))["pose"]
                for name, q in (("steered", eng.rollout(x0, feet, stamp, None, T, COM, command=command, **pv)), ("tracked", r)):
                    up = q["alive"] != 0
                    off, yaw = np.hypot(*(q["x"][-1, up, 3:5] - goal[up, 0:2]).T), np.abs(q["x"][-1, up, 2] - goal[up, 2])
                    print(f"{name}: {up.mean():.1%} alive, {off.mean():.3f} m from the commanded path on average ({off.max():.3f} m at most) after "
                          f"{np.abs(command[up, 0]).mean() * T * dt:.2f} m of it, heading {yaw.mean():.3f} rad off ({yaw.max():.3f} rad at most)")
            else:
                r = eng.rollout(x0, feet, stamp, None, T, COM, push=push, command=command, **pv)
        else:
            r = eng.rollout(x0, feet, stamp, v_ref, T, COM, push=push)
    r["x"][:, :, 5] -= ground(r["x"][:, :, 3:5])                         # heights below are over the ground
    alive = r["alive"] != 0
    if a.yaw_rate:
        print(f"{B} robots, {T} steps: {alive.mean():.1%} alive, solved {np.mean(r['status'] == 1):.2%} of {r['status'].size} QPs at {r['iters'].mean():.1f} iterations")
        if alive.any():
            yaw, speed = r["x"][-1, alive, 2], np.linalg.norm(r["x"][-1, alive, 9:11], axis=1)
            print(f"heading commanded {a.yaw_rate * T * dt:.3f} rad, reached {yaw.mean():.3f} rad on average ({yaw.min():.3f} to {yaw.max():.3f}); "
                  f"speed commanded {command[alive, 0].mean():.3f} m/s on average, at the end {speed.mean():.3f} m/s (lowest CoM {r['x'][:, alive, 5].min():.3f} m)")
        return
    half = T // 2                                                        # the mean velocity over the second half of the roll-out, robots still up
    v = (r["x"][-1, :, 3:5] - r["x"][half, :, 3:5]) / ((T - half) * dt)
    err = np.linalg.norm(v - v_ref, axis=1)
    print(f"{B} robots, {T} steps: {alive.mean():.1%} alive, solved {np.mean(r['status'] == 1):.2%} of {r['status'].size} QPs at {r['iters'].mean():.1f} iterations")
    if alive.any():
        print(f"mean velocity error of the robots still up: {err[alive].mean():.3f} m/s (commands up to 0.3 m/s; lowest CoM {r['x'][:, alive, 5].min():.3f} m)")


if __name__ == "__main__":
    main()
