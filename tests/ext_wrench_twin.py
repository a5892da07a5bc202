"""What the tests of the external wrench share (include/srbdqp.h srbdqp_set_external_wrench): the seeded draw, the CPU twin -- no new oracle code: the
oracle's own linearise / build_qp / presolve / solve_with_restart / rollout around the affine term -- and the per-QP check with the bars of
tests/weights_twin.py, unchanged.

The model.  wrench[k] = [tau_k (3), f_k (3)], world frame, acts during horizon step k:
    x_{k+1} = A_k x_k + B_k u_k + e_k,   e_k = dt [0; 0; I_w,k^-1 tau_k; f_k / m; 0],   I_w,k = R_z(psi_k) I_b R_z(psi_k)',  psi_k = x_ref[k][2].
P, A, l, u of the QP do not change; with D the state response to the e_k alone (D_0 = 0, D_{k+1} = A_k D_k + e_k) the gradient gains (B_qp s)' (Q o D) and
the roll-out gains D.

The draw, per QP: a constant push plus a per-step part -- torque uniform +-4 N m plus +-1 N m, force uniform +-40 N plus +-10 N.

The seeds: batches from weights_twin.batch with weights_twin.batch_seed(N, schedule) except the cases of BATCH_SEED below, wrench 4900 + N, B = 16.  Fixed
on this twin so that in every case of N in {4, 8, 10, 12, 16, 20} x {single, double, mixed, three} at least 14 of 16 QPs end SOLVED, no QP ends SOLVED within
check_every of the 250 cap (where the GPU's count, allowed one check interval of difference, could end on the other side of the cap), every QP's forces move by more than 1 N against the solve without the wrench, and at N = 10 the slowest QP
is past the restart mark (tests/test_ext_wrench_cpu.py asserts all of it)."""
import numpy as np

import srbd_oracle as orc
import weights_twin as wt

HORIZONS = wt.HORIZONS
SCHEDULES = wt.SCHEDULES
B16 = 16
TAU_CONST, TAU_STEP, F_CONST, F_STEP = 4.0, 1.0, 40.0, 10.0

# (N, schedule) -> batch seed where weights_twin.batch_seed(N, schedule) breaks a condition under the drawn wrench: N = 20 single and three leave 13 of 16
# SOLVED, and N = 16 mixed / single / three and N = 20 mixed have a QP that ends SOLVED at 245 or 250 iterations
BATCH_SEED = {(16, "mixed"): 1116, (16, "single"): 1116, (16, "three"): 1116, (20, "mixed"): 1320, (20, "single"): 1320, (20, "three"): 1320}


def batch_seed(N, schedule):
    return BATCH_SEED.get((N, schedule), wt.batch_seed(N, schedule))


def wrench_seed(N):
    return 4900 + N


def draw(B, N, seed):
    """(B, N, 6) wrenches of the draw above (the torques first: constant part, per-step part; then the forces)."""
    rng = np.random.default_rng(seed)
    tau = rng.uniform(-TAU_CONST, TAU_CONST, (B, 1, 3)) + rng.uniform(-TAU_STEP, TAU_STEP, (B, N, 3))
    f = rng.uniform(-F_CONST, F_CONST, (B, 1, 3)) + rng.uniform(-F_STEP, F_STEP, (B, N, 3))
    return np.concatenate([tau, f], axis=2)


def params(N, robot=None, rec=None):
    """The oracle's parameters of one QP with the engine's default restart: its robot record (tests/test_gpu_robots.py::_draw rows) and its weights record
    (weights_twin.draw rows) where given."""
    if rec is not None:
        return wt.params(N, rec, robot)
    r_iter, r_count = orc.default_restart(N)
    kw = dict(rho_restart_iter=r_iter, rho_restart_count=r_count)
    if robot is not None:
        kw.update(mass=float(robot[0]), inertia=tuple(float(v) for v in robot[1:4]), mu=float(robot[4]), fz_min=float(robot[5]), fz_max=float(robot[6]))
    return orc.params_for(N, **kw)


def affine(p, x_ref, w):
    """e_k (N, 13) of the wrench w (N, 6)."""
    x_ref, w = np.asarray(x_ref, np.float64), np.asarray(w, np.float64)
    N = x_ref.shape[0]
    e = np.zeros((N, orc.NX))
    Ib_inv = np.diag(1.0 / np.asarray(p.inertia, dtype=np.float64))
    for k in range(N):
        Rz = orc.rot_z(float(x_ref[k, 2]))
        e[k, 6:9] = p.dt * (Rz @ Ib_inv @ Rz.T @ w[k, 0:3])
        e[k, 9:12] = p.dt * w[k, 3:6] / p.mass
    return e


def response(p, x_ref, w):
    """D (N, 13), row k = D_{k+1}: the state response to the e_k alone, D_0 = 0, D_{k+1} = A_k D_k + e_k (A_k from orc.linearise; it does not depend on the
    lever arms)."""
    x_ref = np.asarray(x_ref, np.float64)
    N = x_ref.shape[0]
    e = affine(p, x_ref, w)
    D = np.zeros((N, orc.NX))
    d = np.zeros(orc.NX)
    for k in range(N):
        A, _ = orc.linearise(p, float(x_ref[k, 2]), np.zeros((orc.NC, 3)))
        d = A @ d + e[k]
        D[k] = d
    return D


def update(p, x0, x_ref, foot, contact, w, pcom=None):
    """The twin of a solve under the wrench w (N, 6): orc.update's steps with q += (B_qp s)' (Q o D) and the roll-out + D; -> orc.update's dict."""
    x_ref = np.asarray(x_ref, np.float64)
    N = x_ref.shape[0]
    qp = orc.build_qp(p, x0, x_ref, foot, contact, pcom)
    D = response(p, x_ref, w)
    Qd = np.tile(np.asarray(p.q_diag, dtype=np.float64), N)
    qp["q"] = qp["q"] + (qp["B_qp"] * p.force_scale).T @ (Qd * D.reshape(-1))
    n, m = qp["P"].shape[0], qp["A"].shape[0]
    red, vi, ri = orc.presolve(qp, contact)
    uh, y = np.zeros(n), np.zeros(m)
    if len(vi) == 0:
        iters, status = 0, orc.STATUS_SOLVED
    else:
        xr_, _, yr_, iters, status = orc.solve_with_restart(p, red["P"], red["q"], red["A"], red["l"], red["u"])
        uh[vi] = xr_
        y[ri] = yr_
    x = orc.rollout(qp, x0, uh, p.force_scale)
    x[1:] += D
    return dict(u=(uh * p.force_scale).reshape(N, orc.NU), x=x, iters=iters, status=status, u_hat=uh, y=y, qp=qp)


def check_qp(out, b, N, p, x0, xr, ft, ct, w, ref=None):
    """QP b of the engine's out against the twin with parameters p under the wrench w (N, 6) (ref: its update(), where the caller has it already), by the
    bars of weights_twin.check_qp; -> the twin's result."""
    if ref is None:
        ref = update(p, x0[b], xr[b], ft[b], ct[b], w)
    assert out["status"][b] == ref["status"] and ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER), (b, out["status"][b], ref["status"])
    assert abs(int(out["iters"][b]) - ref["iters"]) <= p.check_every, (b, out["iters"][b], ref["iters"])
    assert np.abs(out["u"][b] - ref["u"]).max() <= wt.TOL_TWIN_N, (b, np.abs(out["u"][b] - ref["u"]).max())
    assert np.abs(out["x"][b] - ref["x"]).max() <= 1e-5, (b, np.abs(out["x"][b] - ref["x"]).max())
    kq, vi, ri = orc.presolve(ref["qp"], ct[b])
    if ref["status"] == orc.STATUS_SOLVED:
        xs, ys = orc.solve_reference(p, ref["qp"])
        twin_gap = np.abs(ref["u"].reshape(-1) - xs * p.force_scale).max()
        assert np.abs(out["u"][b].reshape(-1) - xs * p.force_scale).max() <= max(wt.TOL_EXACT_N, twin_gap + wt.TOL_TWIN_N)
        kr = orc.kkt_residuals(kq["P"], kq["q"], kq["A"], kq["l"], kq["u"], out["u"][b].reshape(-1)[vi] / p.force_scale, out["y"][b][ri])
        assert kr["primal"] <= 1e-4 and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(ref["qp"]["q"]).max()), kr
    off = np.setdiff1d(np.arange(12 * N), vi)
    assert np.all(out["u"][b].reshape(-1)[off] == 0.0)
    offr = np.setdiff1d(np.arange(20 * N), ri)
    assert np.all(out["y"][b][offr] == 0.0)
    return ref
