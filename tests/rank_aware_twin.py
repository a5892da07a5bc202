"""The oracle twin of the general kernel's rank-aware wrench steps (include/srbdqp.h SRBDQP_FLAG_RANK_AWARE; srbdqp_wrench.hpp, MODE = 5) -- TEST INFRASTRUCTURE
ONLY (plain module, imported by tests/test_rank_aware_cpu.py and tests/test_gpu_rank_aware.py).  It needs nothing new from the oracle.

A wrench step keeps E = Y D^-1 Y' = [A B; B' G] (G diagonal on flat ground).  Where the conditioning guard's quantity orc.step_pivot_ratio(E) is not above
SELECT_RATIO = 1e-4 (the kernel's kRankAwareRatio: 400 x orc.GUARD_RATIO_F64, below every healthy stance of the suite, 4e-4 ... 2e-2) the step takes the
normalised coordinates of E = R R' instead of inverting E:

    Sc = A - B G^-1 B' = L L',   R = [L, B G^-1/2; 0, G^1/2],   R^-1 = [L^-1, -L^-1 B G^-1; 0, G^-1/2]
    g coordinates: the columns of R;   T_jj = R' S_jj R + I,  T_jm = R_j' S_jm R_m;   V = R^-1 Y D^-1;   Bd = D^-1 - V' V

(the rows of V D^1/2 are orthonormal; the step's part of K^-1 is Bd + V' T^-1 V = D^-1 + V'(T^-1 - I) V).  A pivot d of Sc with d <= DROP_RATIO A_jj -- rounding
level: about ten times the rounding of the pivot's own cancellation -- takes reciprocal root 0: a zero column of L, a zero row of V, an identity row of T.  Nothing
coarser may be dropped: the torque about the contact line is physically real, and a column dropped at the guard's threshold leaves the forces up to 2.5 N wrong
("Rank-aware wrench steps").  The selection is wider than the guard's own threshold because E^-1 loses accuracy as 1 / ratio well before the guard
refuses it: the forces stay within the suite's 5e-2 N down to the guard, the stationarity residual does not (20 steps at ratio 2.5e-6: 53 here against the
suite's bound 1e-3 max|q| = 49; 1e-2 in normalised coordinates).  Steps above SELECT_RATIO keep T = S + E^-1, V = E^-1 Y D^-1, Bd = D^-1 - D^-1 Y' V exactly as orc.wrench_reduce forms them;
a QP may mix both kinds, and one without a step at or below SELECT_RATIO gets orc.wrench_reduce's result back unchanged.
"""
from dataclasses import replace

import numpy as np

import srbd_oracle as orc

DROP_RATIO = 1.0e-14
SELECT_RATIO = 1.0e-4
NC, NU = 4, 12


def step_factor(E, drop=DROP_RATIO):
    """R and R^-1 of one wrench step's E = [A B; B' G], G diagonal, as the kernel forms them: (R, Rinv, dropped pivots)."""
    A, Bm, g = E[:3, :3], E[:3, 3:], np.diag(E)[3:]
    BG = Bm / g                                                     # B G^-1
    Sc = A - BG @ Bm.T
    L, r = np.zeros((3, 3)), np.zeros(3)
    for j in range(3):
        d = Sc[j, j] - L[j, :j] @ L[j, :j]
        r[j] = 1.0 / np.sqrt(d) if d > drop * A[j, j] else 0.0
        L[j, j] = d * r[j]
        L[j + 1:, j] = (Sc[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) * r[j]
    Li = np.zeros((3, 3))                                           # forward substitution; the row of a dropped pivot stays 0
    for j in range(3):
        Li[j, j] = r[j]
        for i in range(j + 1, 3):
            Li[i, j] = -(L[i, j:i] @ Li[j:i, j]) * r[i]
    gq = np.sqrt(g)
    R = np.zeros((6, 6)); Rinv = np.zeros((6, 6))
    R[:3, :3], R[:3, 3:], R[3:, 3:] = L, BG * gq, np.diag(gq)
    Rinv[:3, :3], Rinv[:3, 3:], Rinv[3:, 3:] = Li, -Li @ BG, np.diag(1.0 / gq)
    return R, Rinv, int(np.sum(r == 0.0))


def _step_wrench_maps(p, x_ref, foot_hor, contact_hor, pcom):
    """W_k = [I_w^-1 [r]x ... ; I I ...] of every step over its stance contacts (orc.wrench_reduce's Y of a wrench step)."""
    N = x_ref.shape[0]
    Ib_inv = np.diag(1.0 / np.asarray(p.inertia, dtype=np.float64))
    out = []
    for k in range(N):
        cs = [i for i in range(NC) if contact_hor[k, i]]
        Rz = orc.rot_z(float(x_ref[k, 2]))
        blk = np.zeros((6, 3 * len(cs)))
        for q, i in enumerate(cs):
            blk[0:3, 3 * q:3 * q + 3] = Rz @ Ib_inv @ Rz.T @ orc.skew(foot_hor[k, i] - pcom[k])
            blk[3:6, 3 * q:3 * q + 3] = np.eye(3)
        out.append(blk)
    return out


def rank_aware_reduce(p, x_ref, foot_hor, contact_hor, pcom_hor=None, rho=None, drop=DROP_RATIO, threshold=None, every_step=False):
    """orc.wrench_reduce with the steps whose pivot ratio is not above threshold (default SELECT_RATIO; every_step: all wrench steps) in normalised coordinates.
    Returns wrench_reduce's dict, plus ra_steps (their indices) and dropped (pivots dropped in all)."""
    thr = SELECT_RATIO if threshold is None else threshold
    with np.errstate(all="ignore"):
        wr = orc.wrench_reduce(p, x_ref, foot_hor, contact_hor, pcom_hor, rho)
    x_ref = np.asarray(x_ref, dtype=np.float64)
    N = x_ref.shape[0]
    foot = np.asarray(foot_hor, dtype=np.float64).reshape(N, NC, 3)
    ct = np.asarray(contact_hor).reshape(N, NC) != 0
    pcom = x_ref[:, 3:6] if pcom_hor is None else np.asarray(pcom_hor, dtype=np.float64).reshape(N, 3)
    W = _step_wrench_maps(p, x_ref, foot, ct, pcom)
    csz, goff, D = wr["csz"], wr["goff"], wr["D"]
    uoff = np.concatenate([[0], np.cumsum(3 * csz)]).astype(int)
    steps, E_of = [], {}
    for k in range(N):
        if csz[k] < 3:
            continue
        Dk = D[uoff[k]:uoff[k + 1]]
        E_of[k] = (W[k] / Dk) @ W[k].T
        if every_step or not orc.step_pivot_ratio(E_of[k]) > thr:
            steps.append(k)
    if not steps:
        return dict(wr, ra_steps=[], dropped=0)
    n_g = wr["n_g"]
    Rb = np.eye(n_g)
    T_add = np.zeros((n_g, n_g))
    V, Bd = wr["V"].copy(), wr["Bd"].copy()
    dropped = 0
    for k in range(N):
        if wr["gsz"][k] == 0:
            continue
        gs, us = slice(goff[k], goff[k + 1]), slice(uoff[k], uoff[k + 1])
        Dk = D[us]
        if k in steps:
            R, Rinv, nd = step_factor(E_of[k], drop)
            dropped += nd
            Rb[gs, gs] = R
            T_add[gs, gs] = np.eye(6)
            V[gs, us] = Rinv @ (W[k] / Dk)
            Bd[us, us] = np.diag(1.0 / Dk) - V[gs, us].T @ V[gs, us]
        else:                                                       # as orc.wrench_reduce: E^-1 of the step (the identity coordinates of a step with <= 2 contacts: E = D^-1)
            Y = W[k] if csz[k] >= 3 else np.eye(3 * csz[k])
            Einv = np.linalg.inv((Y / Dk) @ Y.T)
            T_add[gs, gs] = 0.5 * (Einv + Einv.T)
    T = Rb.T @ wr["S"] @ Rb
    T = 0.5 * (T + T.T) + T_add
    return dict(wr, T=T, V=V, Bd=Bd, ra_steps=steps, dropped=dropped)


def update_rank_aware(p, x0, x_ref, foot_hor, contact_hor, pcom_hor=None, warm=None, drop=DROP_RATIO, threshold=None, every_step=False):
    """orc.update_split(dtype=float64, guard=False) on rank_aware_reduce: the same admm_solve_split and the same restart rule (every pass re-factors with its rho,
    and so decides per pass which steps are normalised).  A T without a Cholesky factor gives STATUS_NUMERICAL with zero forces, as the kernel does."""
    qp = orc.build_qp(p, x0, x_ref, foot_hor, contact_hor, pcom_hor)
    n, m = qp["P"].shape[0], qp["A"].shape[0]
    red, vi, ri = orc.presolve(qp, contact_hor)
    uh = np.zeros(n); y = np.zeros(m)
    ra_steps = []

    def reduce_(pc):
        w = rank_aware_reduce(pc, x_ref, foot_hor, contact_hor, pcom_hor, drop=drop, threshold=threshold, every_step=every_step)
        ra_steps.append(list(w["ra_steps"]))
        return w

    if len(vi) == 0:
        iters, status = 0, orc.STATUS_SOLVED
    else:
        xi, yi = (None, None) if warm is None else (np.asarray(warm[0])[vi], np.asarray(warm[1])[ri])
        args = (red["P"], red["q"], red["A"], red["l"], red["u"])
        try:
            w = reduce_(p)
            if 0 < p.rho_restart_iter < p.max_iter:
                nre = max(int(p.rho_restart_count), 1)
                pc, xs_, ys_, iters = p, xi, yi, 0
                for k in range(nre + 1):
                    left = p.max_iter - iters
                    cap = p.rho_restart_iter if (k < nre and p.rho_restart_iter < left) else left
                    info = {}
                    xr_, _, yr_, it, status = orc.admm_solve_split(replace(pc, max_iter=cap), *args, w, xs_, ys_, dtype=np.float64, info=info)
                    iters += it
                    if status != orc.STATUS_MAX_ITER or cap == left:
                        break
                    pc = replace(pc, rho=orc.restart_rho(pc, info))
                    w = reduce_(pc)
                    xs_, ys_ = xr_, yr_
            else:
                xr_, _, yr_, iters, status = orc.admm_solve_split(p, *args, w, xi, yi, dtype=np.float64)
        except np.linalg.LinAlgError:
            iters, status = 0, orc.STATUS_NUMERICAL
            xr_, yr_ = np.zeros(len(vi)), np.zeros(len(ri))
        uh[vi] = xr_
        y[ri] = yr_
    N = np.asarray(x_ref).shape[0]
    return dict(u=(uh * p.force_scale).reshape(N, NU), x=orc.rollout(qp, x0, uh, p.force_scale), iters=iters, status=status, u_hat=uh, y=y, qp=qp,
                ra_steps=ra_steps)
