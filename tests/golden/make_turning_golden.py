#!/usr/bin/env python3
"""Generates tests/golden/srbd_turning_golden.npz with THIS repo's fp64 oracle (oracle/srbd_oracle.py) on the inputs of
tests/scenarios.py::turning_batch: a yaw that changes from step to step, footholds that move and lie at different heights,
non-zero roll / pitch / angular-velocity / v_z references.  Same layout as make_golden.py / srbd_qp_golden.npz (inputs, the
QP's gradient and bounds, diagonal and row sums of P, the exact optimum, the ADMM twin's iterate).  Re-run only when the
specification (DESIGN.md "Problem specification") changes:   python tests/golden/make_turning_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import srbd_oracle as orc  # noqa: E402
import scenarios as sc  # noqa: E402

CASES = [  # name, N, yaw kind, schedule, seed, index in the seeded batch
    ("n10_turn_single", 10, "turn", "single", 5242, 0),
    ("n10_wrap_mixed", 10, "wrap", "mixed", 5243, 3),
    ("n10_turn_double", 10, "turn", "double", 5244, 0),
    ("n8_wrap_mixed", 8, "wrap", "mixed", 5245, 0),
    ("n4_random_double", 4, "random", "double", 5246, 1),
    ("n20_turn_double", 20, "turn", "double", 5247, 0),
]


def main():
    p = orc.SrbdParams()
    out = {"params_json": np.array(repr(sorted(p.as_dict().items())))}
    for name, N, yaw, sched, seed, idx in CASES:
        assert orc.params_for(N) == p
        x0, xr, ft, ct = (a[idx] for a in sc.turning_batch(4, N, seed, sched, yaw=yaw))
        qp = orc.build_qp(p, x0, xr, ft, ct)
        xs, ys = orc.solve_reference(p, qp)
        kr = orc.kkt_residuals(qp["P"], qp["q"], qp["A"], qp["l"], qp["u"], xs, ys)
        assert max(kr.values()) < 1e-8 * max(1.0, np.abs(qp["q"]).max()), (name, kr)      # (relative to the gradient: |q| grows with the horizon)
        tw = orc.update(p, x0, xr, ft, ct)
        assert tw["status"] == orc.STATUS_SOLVED, (name, "pick a QP the fixed-rho twin solves")
        assert sc.bound_active(xs * p.force_scale, ct, p), (name, "pick a QP with a force on a bound")
        out[f"{name}/x0"] = x0; out[f"{name}/x_ref"] = xr; out[f"{name}/foot"] = ft; out[f"{name}/contact"] = ct
        out[f"{name}/q"] = qp["q"]; out[f"{name}/l"] = qp["l"]; out[f"{name}/u"] = qp["u"]
        out[f"{name}/P_diag"] = np.diag(qp["P"]).copy(); out[f"{name}/P_rowsum"] = qp["P"].sum(1)
        out[f"{name}/u_exact"] = (xs * p.force_scale).reshape(N, 12)
        out[f"{name}/y_exact"] = ys
        out[f"{name}/x_exact"] = orc.rollout(qp, x0, xs, p.force_scale)
        out[f"{name}/u_admm"] = tw["u"]; out[f"{name}/iters_admm"] = np.int32(tw["iters"])
        print(name, "iters", tw["iters"], "max|u_admm-u_exact|", np.abs(tw["u"] - out[f"{name}/u_exact"]).max())
    np.savez_compressed(os.path.join(HERE, "srbd_turning_golden.npz"), **out)
    print("wrote", os.path.join(HERE, "srbd_turning_golden.npz"))


if __name__ == "__main__":
    main()
