#!/usr/bin/env python3
"""What the foothold preview buys: the six robots of the steering fleet over 150 control steps, the commands of DESIGN.md section 20 with
0.4 m/s forward added, steered and tracked, with and without the 25 N push of section 21 (steps 40 to 59, along y), each with preview and without.

    tools/preview_study.py            the NumPy twin with the C solver (tests/preview_twin.py): no GPU
    tools/preview_study.py --device   BatchMPC.rollout(preview=) on the GPU

Per run and robot, as they come out: the mean planar velocity error against v_w at the robot's own heading, the distance from the path the commands lead
along at the end (track_twin.ideal_path), whether the robot fell, the mean solver iterations.  One JSON line per run, then a table."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

T, N, DT = 150, 10, 0.04


def figures(r, cmd, ideal):
    x = r["x"]
    th = x[:-1, :, 2]
    vwx = np.cos(th) * cmd[None, :, 0] - np.sin(th) * cmd[None, :, 1]
    vwy = np.sin(th) * cmd[None, :, 0] + np.cos(th) * cmd[None, :, 1]
    with np.errstate(invalid="ignore"):
        verr = np.nanmean(np.hypot(x[:-1, :, 9] - vwx, x[:-1, :, 10] - vwy), axis=0)
        dist = np.hypot(x[-1, :, 3] - ideal[-1, :, 0], x[-1, :, 4] - ideal[-1, :, 1])
    return dict(velocity_error=verr.round(4).tolist(), path_distance=dist.round(4).tolist(), fallen=int((np.asarray(r["alive"]) == 0).sum()),
                alive=np.asarray(r["alive"]).tolist(), mean_iters=np.asarray(r["iters"]).mean(axis=0).round(2).tolist(),
                unsolved=int((np.asarray(r["status"]) != 1).sum()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", action="store_true", help="run BatchMPC.rollout on the GPU instead of the twin")
    ap.add_argument("--forward", type=float, default=0.4, help="m/s added to every command's vx")
    a = ap.parse_args()
    import fleet_twin as ft
    import steer_twin as stw
    import track_twin as ttw
    f = stw.fleet()
    cmd = f["command"].copy()
    cmd[:, 0] += a.forward
    ideal = ttw.ideal_path(f["x"], cmd, T, DT)
    push = np.zeros((T, 6, 6)); push[40:60, :, 4] = 25.0
    if a.device:
        from g1_locomotion_amd import BatchMPC
        eng = BatchMPC(horizon=N)
        run = lambda track, preview, pu: eng.rollout(f["x"], f["feet"], f["stamp"], None, T, ft.COM, standing=f["standing"], push=pu, command=cmd,
                                                     track=True if track else None, preview=True if preview else None)
    else:
        import preview_twin as pvt
        import srbd_oracle as orc
        p = orc.default_params(N)
        run = lambda track, preview, pu: pvt.rollout(p, f["x"], f["feet"], f["stamp"], cmd, T, ft.COM, track=track, standing=f["standing"], push=pu,
                                                     preview=preview)
    rows = []
    for track in (False, True):
        for pushed in (False, True):
            for preview in (False, True):
                with np.errstate(all="ignore"):
                    r = run(track, preview, push if pushed else None)
                row = dict(where="device" if a.device else "twin", form="tracked" if track else "steered", pushed=pushed, preview=preview, **figures(r, cmd, ideal))
                rows.append(row)
                print(json.dumps(row), flush=True)
    print("\nform     pushed preview fallen  mean |v - v_w|  mean path distance  mean iters")
    for r in rows:
        print(f"{r['form']:8s} {str(r['pushed']):6s} {str(r['preview']):7s} {r['fallen']:6d}  {np.nanmean(r['velocity_error']):14.4f}  "
              f"{np.nanmean(r['path_distance']):18.4f}  {np.mean(r['mean_iters']):10.2f}")


if __name__ == "__main__":
    main()
