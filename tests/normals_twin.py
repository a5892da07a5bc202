"""The oracle twin of a solve with contact normals (include/srbdqp.h srbdqp_set_contact_normals), shared by tests/test_contact_normals_cpu.py and
tests/test_gpu_contact_normals.py.  It needs nothing new from the oracle: the QP of orc.build_qp in the local force variables f_loc = R' f of every
contact's frame R = contact_frames(normal),

    P_loc = sym(T' P T),  q_loc = T' q,  T = blockdiag(R),  A, l, u unchanged,

through the same presolve and restarted ADMM orc.update runs; u_world = s T u_loc, and the roll-out is the world-frame one.  With every normal
(0, 0, 1) T is the identity and the twin is orc.update bit for bit."""
import numpy as np

import srbd_oracle as orc
from weights_twin import batch  # noqa: F401  (the batches of the robots and weights suites: one copy)
from g1_locomotion_amd import contact_frames

TOL_TWIN_N = 2e-3
TOL_EXACT_N = 5e-2
HORIZONS = (4, 8, 10, 12, 16, 20)
SCHEDULES = ("single", "double", "mixed", "three")


def params(N):
    r_iter, r_count = orc.default_restart(N)
    return orc.params_for(N, rho_restart_iter=r_iter, rho_restart_count=r_count)


def flat_normals(B, N):
    nr = np.zeros((B, N, 4, 3))
    nr[..., 2] = 1.0
    return nr.reshape(B, N, 12)


def foot_normals(B, N, left, right):
    """One normal per foot for the whole horizon: contacts 0, 1 are the left foot's heel and toe, 2, 3 the right foot's (g1_locomotion_amd/synth.py)."""
    nr = np.zeros((B, N, 4, 3))
    nr[:, :, 0:2] = np.asarray(left, float)
    nr[:, :, 2:4] = np.asarray(right, float)
    return nr.reshape(B, N, 12)


def ridge_normals(B, N, angle=0.6):
    """The feet either side of a ridge: left-foot normals (0, sin a, cos a), right-foot normals (0, -sin a, cos a)."""
    return foot_normals(B, N, (0.0, np.sin(angle), np.cos(angle)), (0.0, -np.sin(angle), np.cos(angle)))


def wedge_normals(B, N, angle=0.3):
    """The feet on the two faces of a wedge: the normals lean inward."""
    return foot_normals(B, N, (0.0, -np.sin(angle), np.cos(angle)), (0.0, np.sin(angle), np.cos(angle)))


def drawn_normals(B, N, rng, per_step, max_tilt=0.35):
    """One normal per foot, tilt uniform in [0, max_tilt] rad, any azimuth; constant over the horizon, or redrawn at every step."""
    shape = (B, N if per_step else 1, 2)
    tilt, az = rng.uniform(0.0, max_tilt, shape), rng.uniform(-np.pi, np.pi, shape)
    n = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], -1)          # (B, N or 1, 2, 3)
    n = np.broadcast_to(n, (B, N, 2, 3))
    return np.repeat(n, 2, axis=2).reshape(B, N, 12).copy()


def frames_matrix(normals):
    """T = blockdiag(R) of one QP's normals (N, 12): 12 N x 12 N."""
    R = contact_frames(np.asarray(normals, float).reshape(-1, 3))
    T = np.zeros((3 * len(R), 3 * len(R)))
    for i, Ri in enumerate(R):
        T[3 * i:3 * i + 3, 3 * i:3 * i + 3] = Ri
    return T


def twin(p, x0, x_ref, foot, contact, normals, pcom=None):
    """dict(u (N, 12) world newtons, x (N + 1, 13), iters, status, u_loc (12 N,) scaled local forces, y (20 N,), qp, qp_loc, T)."""
    qp = orc.build_qp(p, x0, x_ref, foot, contact, pcom)
    T = frames_matrix(normals)
    P = T.T @ qp["P"] @ T
    loc = dict(qp, P=0.5 * (P + P.T), q=T.T @ qp["q"])
    n, m = loc["P"].shape[0], loc["A"].shape[0]
    red, vi, ri = orc.presolve(loc, contact)
    uh, y = np.zeros(n), np.zeros(m)
    if len(vi) == 0:
        iters, status = 0, orc.STATUS_SOLVED
    else:
        xr_, _, yr_, iters, status = orc.solve_with_restart(p, red["P"], red["q"], red["A"], red["l"], red["u"])
        uh[vi] = xr_
        y[ri] = yr_
    N = np.asarray(x_ref).shape[0]
    return dict(u=(p.force_scale * (T @ uh)).reshape(N, 12), x=orc.rollout(qp, x0, T @ uh, p.force_scale), iters=iters, status=status, u_loc=uh, y=y,
                qp=qp, qp_loc=loc, T=T)


def cone_violation(p, qp, T, u_world):
    """By how much (scaled variables) the world-frame forces u_world (newtons) leave the pyramids of the frames T: max over the rows of l - A x, A x - u."""
    ax = qp["A"] @ (T.T @ np.asarray(u_world, float).reshape(-1) / p.force_scale)
    return max(0.0, float(np.max(qp["l"] - ax)), float(np.max(ax - qp["u"])))


def friction_row_active(p, T, u_world, contact, tol=0.05):
    """A stance contact of some step on a friction row of its own frame (|f_loc,x| or |f_loc,y| = mu f_loc,z, to tol newtons)."""
    f = (T.T @ np.asarray(u_world, float).reshape(-1)).reshape(-1, 4, 3)
    st = np.asarray(contact).reshape(-1, 4) != 0
    fz = f[..., 2]
    return bool(np.any(st & (np.maximum(np.abs(f[..., 0]), np.abs(f[..., 1])) >= p.mu * fz - tol) & (fz > tol)))


def check_qp(out, b, N, p, ref, contact):
    """The per-QP checks and tolerances of tests/test_gpu_robots.py::_check_qp on the local QP: out = the engine's dict(u, x, y, status, iters), ref = twin()."""
    assert out["status"][b] == ref["status"] and ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER), (b, out["status"][b], ref["status"])
    assert abs(int(out["iters"][b]) - ref["iters"]) <= p.check_every, (b, out["iters"][b], ref["iters"])
    assert np.abs(out["u"][b] - ref["u"]).max() <= TOL_TWIN_N, (b, np.abs(out["u"][b] - ref["u"]).max())
    assert np.abs(out["x"][b] - ref["x"]).max() <= 1e-5, (b, np.abs(out["x"][b] - ref["x"]).max())
    kq, vi, ri = orc.presolve(ref["qp_loc"], contact)
    s, T = p.force_scale, ref["T"]
    u_loc = T.T @ out["u"][b].reshape(-1) / s                          # the engine's forces in the local, scaled variables
    if ref["status"] == orc.STATUS_SOLVED:
        xs, ys = orc.solve_reference(p, ref["qp_loc"])
        twin_gap = np.abs(ref["u_loc"] - xs).max() * s
        assert np.abs(u_loc - xs).max() * s <= max(TOL_EXACT_N, twin_gap + TOL_TWIN_N), (b, np.abs(u_loc - xs).max() * s, twin_gap)
        kr = orc.kkt_residuals(kq["P"], kq["q"], kq["A"], kq["l"], kq["u"], u_loc[vi], out["y"][b][ri])
        assert kr["primal"] <= 1e-4 and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(ref["qp_loc"]["q"]).max()), (b, kr)
    off = np.setdiff1d(np.arange(12 * N), vi)
    assert np.all(out["u"][b].reshape(-1)[off] == 0.0), b
    offr = np.setdiff1d(np.arange(20 * N), ri)
    assert np.all(out["y"][b][offr] == 0.0), b
