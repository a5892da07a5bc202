"""What the tests of the per-QP cost weights share (include/srbdqp.h srbdqp_weights, srbdqp_set_weights): the seeded draw of the records, the oracle's
parameters for one record (orc.params_for(N, q_diag=..., r_diag=...) builds and solves the QP with any weights -- no new oracle code), and -- shared with
the robot records' suite, tests/test_gpu_robots.py, whose docstring states the bars -- the batches and the per-QP check.

The draw, per QP: every q_diag entry is the default times a log-uniform factor in [0.25, 4], r_diag the default times a log-uniform factor in [0.1, 10];
QP 0 has zero angular weights (q[0:3] = q[6:9] = 0) and QP 1 all q = 0 (only the regularisation remains).

The seeds: batch 900 + N and weights 2900 + N, except the cases of BATCH_SEED.  They were fixed on the CPU oracle (default restart rule, B = 16) so that in
every case of N in {4, 8, 10, 12, 16, 20} x {single, double, mixed, three} at least 14 of 16 QPs end SOLVED and no QP's iteration count lies within
check_every of the 250 cap (where the GPU's count, allowed one check interval of difference, could end on the other side of the cap)."""
import numpy as np

import srbd_oracle as orc

TOL_TWIN_N = 2e-3
TOL_EXACT_N = 5e-2
HORIZONS = (4, 8, 10, 12, 16, 20)          # (N = 24: the setters refuse it)
SCHEDULES = ("single", "double", "mixed", "three")

# (N, schedule) -> batch seed where 900 + N has a QP that ends at exactly 250 iterations
BATCH_SEED = {(4, "single"): 804, (10, "double"): 810, (10, "three"): 810}


def batch_seed(N, schedule):
    return BATCH_SEED.get((N, schedule), 900 + N)


def weights_seed(N):
    return 2900 + N


def batch(B, N, seed, schedule):
    """The batches of the robots, weights and contact-normals suites (test_gpu_robots.py and normals_twin.py import this one), built as
    tests/test_gpu_wrench.py::_batch builds its own ("three": steps with exactly 3 stance contacts)."""
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=seed, schedule="mixed" if schedule == "three" else schedule)
    if schedule == "three":
        rng = np.random.default_rng(seed)
        for b in range(B):
            for k in range(N):
                if ct[b, k].sum() == 4 or rng.random() < 0.3:
                    ct[b, k] = 1
                    ct[b, k, rng.integers(0, 4)] = 0
    return x0, xr, ft, ct


def ragged_inputs(B, horizons, seed):
    """B QPs with horizons drawn from `horizons`, shuffled across the buckets, packed step-major: (N_per_qp, x0, x_ref, foot, contact)."""
    rng = np.random.default_rng(seed)
    Nq = rng.choice(horizons, B).astype(np.int32)
    X0, XR, FT, CT = [], [], [], []
    for i, N in enumerate(Nq):
        x0, xr, ft, ct = batch(1, int(N), seed * 1000 + i, SCHEDULES[i % 4])
        X0.append(x0[0]); XR.append(xr[0]); FT.append(ft[0]); CT.append(ct[0])
    return Nq, np.stack(X0), np.concatenate(XR), np.concatenate(FT), np.concatenate(CT)


def draw(B, seed):
    """(B, 16) records of the draw above (the layout of g1_locomotion_amd.weights_array, built here so that the CPU tests need no library)."""
    p = orc.SrbdParams()
    rng = np.random.default_rng(seed)
    out = np.zeros((B, 16), np.float64)
    out[:, :13] = np.asarray(p.q_diag) * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 13)))
    out[:, 13] = p.r_diag * np.exp(rng.uniform(np.log(0.1), np.log(10.0), B))
    if B > 0:
        out[0, 0:3] = 0.0
        out[0, 6:9] = 0.0
    if B > 1:
        out[1, :13] = 0.0
    return out


def params(N, rec, robot=None):
    """The oracle's parameters of one QP: its weights record, its robot record (tests/test_gpu_robots.py::_draw rows) if any, the engine's default restart."""
    r_iter, r_count = orc.default_restart(N)
    kw = dict(q_diag=tuple(float(v) for v in rec[:13]), r_diag=float(rec[13]), rho_restart_iter=r_iter, rho_restart_count=r_count)
    if robot is not None:
        kw.update(mass=float(robot[0]), inertia=tuple(float(v) for v in robot[1:4]), mu=float(robot[4]), fz_min=float(robot[5]), fz_max=float(robot[6]))
    return orc.params_for(N, **kw)


def check_qp(out, b, N, p, x0, xr, ft, ct):
    """QP b of the engine's out against the oracle with parameters p, by the bars in the docstring of tests/test_gpu_robots.py; -> the oracle's result."""
    ref = orc.update(p, x0[b], xr[b], ft[b], ct[b])
    assert out["status"][b] == ref["status"] and ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER), (b, out["status"][b], ref["status"])
    assert abs(int(out["iters"][b]) - ref["iters"]) <= p.check_every, (b, out["iters"][b], ref["iters"])
    assert np.abs(out["u"][b] - ref["u"]).max() <= TOL_TWIN_N, (b, np.abs(out["u"][b] - ref["u"]).max())
    assert np.abs(out["x"][b] - ref["x"]).max() <= 1e-5
    kq, vi, ri = orc.presolve(ref["qp"], ct[b])
    if ref["status"] == orc.STATUS_SOLVED:
        xs, ys = orc.solve_reference(p, ref["qp"])
        # (a drawn robot whose ADMM solution -- the oracle twin's too -- stops farther than 5e-2 N from the optimum at eps 1e-6 is held to the twin's
        #  own distance: one QP of N = 20 single support, 0.0503 N on the GPU and the twin alike)
        twin_gap = np.abs(ref["u"].reshape(-1) - xs * p.force_scale).max()
        assert np.abs(out["u"][b].reshape(-1) - xs * p.force_scale).max() <= max(TOL_EXACT_N, twin_gap + TOL_TWIN_N)
        kr = orc.kkt_residuals(kq["P"], kq["q"], kq["A"], kq["l"], kq["u"], out["u"][b].reshape(-1)[vi] / p.force_scale, out["y"][b][ri])
        assert kr["primal"] <= 1e-4 and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(ref["qp"]["q"]).max()), kr
    off = np.setdiff1d(np.arange(12 * N), vi)
    assert np.all(out["u"][b].reshape(-1)[off] == 0.0)
    offr = np.setdiff1d(np.arange(20 * N), ri)
    assert np.all(out["y"][b][offr] == 0.0)
    return ref
