"""Seeded inputs of a robot that turns, steps and walks on uneven ground -- TEST INFRASTRUCTURE ONLY (plain module, imported by
tests/test_oracle_turning.py, tests/test_gpu_turning.py and tests/golden/make_turning_golden.py).

synthetic_batch() (g1_locomotion_amd/synth.py: what bench.py, smoke() and the older tests draw from) holds the linearisation yaw, the
footholds and six reference columns constant over the horizon.  With a constant yaw C_i - C_m = (i - m) Rz', so a kernel that reads the yaw
or the foothold of the wrong step computes bit-identical results.  turning_batch() starts from the same contact schedules and x0 ranges and
varies exactly those inputs from step to step.
"""
import numpy as np

import srbd_oracle as orc
from g1_locomotion_amd.synth import HIP_Y, HEEL_X, TOE_X, synthetic_batch

YAW_KINDS = ("turn", "wrap", "random")
ZERO_COLUMNS = (0, 1, 6, 7, 11)         # roll, pitch, omega_x, omega_y, v_z: 0 in synthetic_batch(); with omega_z (8) the six formerly-zero columns


def turning_batch(B, N, seed, schedule="single", dt=0.04, yaw="turn", terrain=0.08, pcom=False):
    """x0 (B,13), x_ref (B,N,13), foot (B,N,12), contact (B,N,4) uint8 [, pcom (B,N,3) when pcom=True].

    yaw: "turn"   yaw_k = yaw_0 + r k dt, r uniform in +-2 rad/s per QP, x_ref[:, 8] = r
         "wrap"   a +-1.5 rad/s ramp that crosses +-pi in the middle of the horizon, values wrapped to (-pi, pi]
         "random" independent uniform (-pi, pi) per step (unphysical: the hardest case for the tables' cancellation)
    x_ref: roll / pitch +-0.1 rad, omega_x,y +-0.3 rad/s, v_z +-0.2 m/s, CoM height +-0.03 m, all per step ("random": omega_z +-0.3 rad/s too)
    foot: a new foothold for a foot at step 0 and at every touch-down inside the horizon, under the reference CoM of that step, turned by that
          step's yaw plus a foot yaw of +-0.3 rad, +-8 cm fore-aft / +-3 cm lateral jitter, height +-terrain and +-0.01 m between heel and toe;
          held while the foot stands.  schedule "double" has no touch-down: each foot is re-placed once at a random step >= 1 instead.
    pcom: x_ref's CoM +-0.03 m per step and axis (an explicit p_com_horizon)."""
    if yaw not in YAW_KINDS:
        raise ValueError(f"yaw must be one of {YAW_KINDS}")
    x0, xr, ft, ct = (a.copy() for a in synthetic_batch(B, N, seed, schedule, dt=dt))
    rng = np.random.default_rng(seed + 77777)
    k = np.arange(1, N + 1)[None, :]
    if yaw == "turn":
        rate = rng.uniform(-2.0, 2.0, (B, 1))
        xr[:, :, 2] = x0[:, 2:3] + rate * k * dt
        xr[:, :, 8] = rate
    elif yaw == "wrap":
        rate = rng.choice([-1.5, 1.5], (B, 1))
        start = np.sign(rate) * (np.pi - 0.5 * np.abs(rate) * N * dt)
        x0[:, 2] = start[:, 0]
        psi = start + rate * k * dt
        xr[:, :, 2] = np.pi - (np.pi - psi) % (2 * np.pi)             # wrapped to (-pi, pi]
        xr[:, :, 8] = rate
    else:
        xr[:, :, 2] = rng.uniform(-np.pi, np.pi, (B, N))
        xr[:, :, 8] = rng.uniform(-0.3, 0.3, (B, N))
    xr[:, :, 0:2] = rng.uniform(-0.1, 0.1, (B, N, 2))
    xr[:, :, 6:8] = rng.uniform(-0.3, 0.3, (B, N, 2))
    xr[:, :, 11] = rng.uniform(-0.2, 0.2, (B, N))
    xr[:, :, 5] += rng.uniform(-0.03, 0.03, (B, N))
    replace_at = rng.integers(1, N, (B, 2)) if schedule == "double" else np.full((B, 2), -1)
    for b in range(B):
        for f in range(2):
            hold = None
            for kk in range(N):
                on = ct[b, kk, 2 * f] or ct[b, kk, 2 * f + 1]
                touch_down = on and kk > 0 and not (ct[b, kk - 1, 2 * f] or ct[b, kk - 1, 2 * f + 1])
                if hold is None or touch_down or kk == replace_at[b, f]:
                    psi_k = xr[b, kk, 2]
                    c, s = np.cos(psi_k), np.sin(psi_k)
                    fyaw = rng.uniform(-0.3, 0.3)
                    cf, sf = np.cos(psi_k + fyaw), np.sin(psi_k + fyaw)
                    py = (HIP_Y if f == 0 else -HIP_Y) + rng.uniform(-0.03, 0.03)
                    px = rng.uniform(-0.08, 0.08)
                    z = rng.uniform(-terrain, terrain)
                    cx, cy = xr[b, kk, 3] + c * px - s * py, xr[b, kk, 4] + s * px + c * py
                    hold = [[cx + cf * off, cy + sf * off, z + rng.uniform(-0.01, 0.01)] for off in (HEEL_X, TOE_X)]
                for h in range(2):
                    i = 2 * f + h
                    ft[b, kk, 3 * i:3 * i + 3] = hold[h]
    if pcom:
        return x0, xr, ft, ct, xr[:, :, 3:6] + rng.uniform(-0.03, 0.03, (B, N, 3))
    return x0, xr, ft, ct


def three_contacts(ct, seed):
    """Steps with exactly 3 stance contacts, as tests/test_gpu_wrench.py::_batch makes its "three" pattern from a "mixed" schedule."""
    ct = ct.copy()
    rng = np.random.default_rng(seed)
    for b in range(ct.shape[0]):
        for k in range(ct.shape[1]):
            if ct[b, k].sum() == 4 or rng.random() < 0.3:
                ct[b, k] = 1
                ct[b, k, rng.integers(0, 4)] = 0
    return ct


def batch(B, N, seed, schedule, yaw="turn", **kw):
    """turning_batch() with the general kernel's fourth pattern: "three" = "mixed" footholds, contacts through three_contacts()."""
    out = list(turning_batch(B, N, seed, "mixed" if schedule == "three" else schedule, yaw=yaw, **kw))
    if schedule == "three":
        out[3] = three_contacts(out[3], seed)
    return tuple(out)


def refined_inverse(K, tol=1e-11):
    """inv(K) to more digits than np.linalg.inv gives (cond K reaches 2e8 here, so float64 inversion alone costs ~2e-9 of the 1e-8 operator bound):
    Newton-Schulz steps X <- X + X (I - K X) in np.longdouble until the residual max|I - K X| stops falling.  The residual reached is asserted
    (<= tol) before X is handed out; returns (X as float64, residual)."""
    Kl = np.asarray(K, dtype=np.longdouble)
    I = np.eye(Kl.shape[0], dtype=np.longdouble)
    X = np.linalg.inv(np.asarray(K, dtype=np.float64)).astype(np.longdouble)
    R = I - Kl @ X
    res = float(np.abs(R).max())
    for _ in range(8):
        Xn = X + X @ R
        Rn = I - Kl @ Xn
        rn = float(np.abs(Rn).max())
        if not rn < res:
            break
        X, R, res = Xn, Rn, rn
    assert res <= tol, f"reference inverse: residual {res:.2e} after refinement"
    return np.asarray(X, dtype=np.float64), res


def dense_k(p, red):
    """The oracle's dense reduced-KKT matrix of a presolved QP: P + sigma I + A' rho A."""
    rho = orc.rho_vector(p, red["l"], red["u"])
    return red["P"] + p.sigma * np.eye(red["P"].shape[0]) + (red["A"].T * rho) @ red["A"]


def wrench_blocks_reference_error(p, x_ref, foot, contact, pcom=None):
    """How far orc.wrench_reduce()'s own float64 V and Bd blocks are from the same blocks formed in np.longdouble (E^-1 refined there), relative to
    max|V| and max(max|Bd|, 1e-3) as the assembly tests scale them: (error of V, error of Bd, largest cond(E)).  A step whose three stance contacts are
    nearly collinear has cond(E) ~ 1e8, and the float64 reference is then off by 1e-11 itself: such an input cannot hold a kernel to 1e-11."""
    L = np.longdouble
    N = x_ref.shape[0]
    ft = np.asarray(foot, dtype=L).reshape(N, 4, 3)
    on = np.asarray(contact).reshape(N, 4) != 0
    pc = np.asarray(x_ref[:, 3:6] if pcom is None else pcom, dtype=L).reshape(N, 3)
    wr = orc.wrench_reduce(p, x_ref, foot, contact, pcom_hor=pcom)
    s, rho = p.force_scale, p.rho
    dxy = L(p.r_diag) * s * s + p.sigma + 2.0 * rho
    dz = L(p.r_diag) * s * s + p.sigma + (4.0 * L(p.mu) ** 2 + p.rho_fz_scale) * rho
    sV, sB = np.abs(wr["V"]).max(), max(np.abs(wr["Bd"]).max(), 1e-3)
    eV = eB = cond = 0.0
    uoff = 0
    for k in range(N):
        cs = [i for i in range(4) if on[k, i]]
        n = 3 * len(cs)
        if len(cs) >= 3:
            c, sn = np.cos(L(x_ref[k, 2])), np.sin(L(x_ref[k, 2]))
            Rz = np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1]], dtype=L)
            Iw_inv = Rz @ np.diag(1 / np.asarray(p.inertia, dtype=L)) @ Rz.T
            Y = np.zeros((6, n), dtype=L)
            for q, i in enumerate(cs):
                r = ft[k, i] - pc[k]
                Y[0:3, 3 * q:3 * q + 3] = Iw_inv @ np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], dtype=L)
                Y[3:6, 3 * q:3 * q + 3] = np.eye(3, dtype=L)
            D = np.tile(np.array([dxy, dxy, dz], dtype=L), len(cs))
            E = (Y / D) @ Y.T
            X = np.linalg.inv(E.astype(np.float64)).astype(L)
            for _ in range(6):
                X = X + X @ (np.eye(6, dtype=L) - E @ X)
            V = X @ (Y / D)
            Bd = np.diag(1 / D) - (Y / D).T @ V
            gs = slice(wr["goff"][k], wr["goff"][k + 1])
            eV = max(eV, float(np.abs(wr["V"][gs, uoff:uoff + n] - V).max() / sV))
            eB = max(eB, float(np.abs(wr["Bd"][uoff:uoff + n, uoff:uoff + n] - Bd).max() / sB))
            cond = max(cond, float(np.linalg.cond(E.astype(np.float64))))
        uoff += n
    return eV, eB, cond


def bound_active(u, ct, p, tol=0.05):
    """Some stance contact of some step on a friction-pyramid row (|f_x| or |f_y| = mu f_z) or on an fz bound."""
    f = np.asarray(u, dtype=np.float64).reshape(-1, 4, 3)
    st = np.asarray(ct).reshape(-1, 4) != 0
    fz = f[..., 2]
    fric = np.maximum(np.abs(f[..., 0]), np.abs(f[..., 1])) >= p.mu * fz - tol
    return bool(np.any(st & (fric | (fz >= p.fz_max - tol) | (fz <= p.fz_min + tol))))


# ---- deliberately wrong views of the inputs: what a kernel with an off-by-one step index would compute ---------------------------------
def yaw_of_next_step(xr):
    """x_ref with the yaw of step k + 1 in the place of step k's (the last step keeps its own)."""
    out = xr.copy()
    out[..., :-1, 2] = xr[..., 1:, 2]
    return out


def foothold_of_step0(ft):
    """foot with the row of step 0 on every step."""
    return np.broadcast_to(ft[..., 0:1, :], ft.shape).copy()


# ---- nearly collinear stance contacts: where the general kernel's wrench coordinates lose rank ------------------------------------------
EPS_LADDER = (1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 1e-4, 1e-5, 1e-6, 1e-8, 0.0)
COLLINEAR_KINDS = ("tandem", "point")


def wrench_steps(contact):
    """Indices of the steps the general kernel keeps in wrench coordinates: three or four stance contacts."""
    return [int(k) for k in np.nonzero((np.asarray(contact).reshape(-1, 4) != 0).sum(axis=1) >= 3)[0]]


def collinear_contacts(foot, contact, eps, kind, steps=None):
    """foot (N, 12) of ONE QP with the contact points of `steps` (default: every wrench step) moved to within eps metres of one line; a copy.

    kind: "tandem" the right foot is put on the line through the left foot's heel and toe, 3 cm ahead of the left toe, offset sideways by eps
          "point"  point feet: each toe is put at its heel + eps sideways of the line through the two heels
    All four points of a step are moved whether they stand or swing (a swing point's position never enters the QP); heights are kept.  With eps = 0 the
    stance points of a deformed step lie exactly on one line: E = Y D^-1 Y' of that step has rank 5, while the QP itself stays well posed."""
    if kind not in COLLINEAR_KINDS:
        raise ValueError(f"kind must be one of {COLLINEAR_KINDS}")
    ft = np.array(foot, dtype=np.float64).reshape(-1, 4, 3)
    for k in (wrench_steps(contact) if steps is None else steps):
        a, b = (ft[k, 0, :2], ft[k, 1, :2]) if kind == "tandem" else (ft[k, 0, :2], ft[k, 2, :2])
        d = (b - a) / np.linalg.norm(b - a)
        side = np.array([-d[1], d[0]])
        if kind == "tandem":
            length = np.linalg.norm(ft[k, 3, :2] - ft[k, 2, :2])
            ft[k, 2, :2] = b + 0.03 * d + eps * side
            ft[k, 3, :2] = ft[k, 2, :2] + length * d
        else:
            ft[k, 1, :2] = ft[k, 0, :2] + eps * side
            ft[k, 3, :2] = ft[k, 2, :2] + eps * side
    return ft.reshape(np.shape(foot))


def collinear_ladder(N, schedule, seed, kind, placement="all", rungs=EPS_LADDER):
    """One base QP of synthetic_batch() ("three": "mixed" footholds, contacts through three_contacts()) deformed at every eps of `rungs`.
    placement: "all" wrench steps, only the "first" or only the "last" one.  Returns x0 (R,13), x_ref (R,N,13), foot (R,N,12), contact (R,N,4)."""
    x0, xr, ft, ct = synthetic_batch(1, N, seed, "mixed" if schedule == "three" else schedule)
    if schedule == "three":
        ct = three_contacts(ct, seed)
    ws = wrench_steps(ct[0])
    assert ws, "the base QP has no wrench step"
    steps = {"all": ws, "first": ws[:1], "last": ws[-1:]}[placement]
    R = len(rungs)
    foot = np.stack([collinear_contacts(ft[0], ct[0], e, kind, steps) for e in rungs])
    return np.repeat(x0, R, 0), np.repeat(xr, R, 0), foot, np.repeat(ct, R, 0)
