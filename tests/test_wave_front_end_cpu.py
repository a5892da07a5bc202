"""CPU restatement of the one-wave kernel's set-up tables on step PAIRS (csrc/srbdqp_setup1.hpp, setup1_pass and gt_tables).

The kernel gives every pair (m, i >= m) of horizon steps a lane: pair p = r (N + 1) + c, r < N / 2, is (r, r + c) for c < N - r and
(N - 1 - r, c - 1) behind that, so that the pairs of one m are neighbours in ascending i from slot pair_base(m) on.  The pair lane forms
C_i - C_m and the terms of T1 / T2 (and, per call of gt_tables, the three torque terms of the G'v table) once; lane m adds up its slots
in ascending i and forms the last step's t2zz term itself (one multiply-add in the kernel, as the loop had it).  These tests check
  * the mapping: every pair once, the slots of one m consecutive and ascending in i;
  * that the sums over the slots are the SAME float64 numbers as the step loop they replace (lane m walking over i with exact zeros in
    front of m): NumPy has no fused operation in either form, so equality is exact;
  * T1 / T2 / D / E and the gradient the tables give against the oracle's step-loop expressions.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import srbd_oracle as orc  # noqa: E402

EPS = np.finfo(float).eps


# ---- the kernel's pair mapping ----------------------------------------------------------------------------------------------------
def pair_of_lane(p, N):
    r, c = divmod(p, N + 1)
    if c < N - r:
        m, s = r, c
    else:
        m, s = N - 1 - r, c - (N - r)
    return m, m + s


def pair_base(m, N):
    return m * (N + 1) if 2 * m < N else (N - m) * N


def prefix_cc_cs(yaw):
    """lane k: cc_k, cs_k summed over all N steps in order, the steps past k adding exact zeros"""
    N = len(yaw)
    c, s = np.cos(yaw), np.sin(yaw)
    cc, cs = np.zeros(N), np.zeros(N)
    for lane in range(N):
        a = b = 0.0
        for k in range(N):
            a += c[k] if k <= lane else 0.0
            b += s[k] if k <= lane else 0.0
        cc[lane], cs[lane] = a, b
    return cc, cs


# ---- T1 / T2: the step loop (the kernel until round 12) and the pair lanes ---------------------------------------------------------
def six_sums_loop(cc, cs, w):
    N = len(cc)
    out = np.zeros((N, 6))
    for m in range(N):
        t = [0.0] * 6
        for i in range(N):
            on = i >= m
            da, db, dz = cc[i] - cc[m], cs[i] - cs[m], float(i - m)
            terms = (da, db, (w[0] * da) * da + (w[1] * db) * db, (w[0] * da) * db - (w[1] * db) * da, (w[0] * db) * db + (w[1] * da) * da, (w[2] * dz) * dz)
            for k in range(6):
                t[k] += terms[k] if on else 0.0
        out[m] = t
    return out


def six_sums_pairs(cc, cs, w):
    N = len(cc)
    NP = N * (N + 1) // 2
    slot = np.full((N * N // 2 + N, 6), np.nan)           # (slots no pair owns are never summed: NaN would show)
    dab = np.zeros((NP, 2))
    for p in range(NP):
        m, i = pair_of_lane(p, N)
        da, db, dz = cc[i] - cc[m], cs[i] - cs[m], float(i - m)
        dab[p] = da, db
        # (the t2zz term of the LAST step stays on lane m -- the kernel's loop fused it with the accumulator, and lane m still does: the pair stores +0)
        slot[p] = (da, db, (w[0] * da) * da + (w[1] * db) * db, (w[0] * da) * db - (w[1] * db) * da, (w[0] * db) * db + (w[1] * da) * da,
                   0.0 if i == N - 1 else (w[2] * dz) * dz)
    out = np.zeros((N, 6))
    for m in range(N):
        t = np.zeros(6)
        for s in range(N):
            if s < N - m:
                t = t + slot[pair_base(m, N) + s]
        dzl = float(N - 1 - m)
        t[5] = t[5] + (w[2] * dzl) * dzl
        out[m] = t
    return out, dab


def de_from_six(six, cc, cs, sq, dt, N):
    """de_step (srbdqp_common.hpp): D_m, E_m from C_m, T1(m), T2(m)"""
    D, E = np.zeros((N, 3, 3)), np.zeros((N, 3, 3))
    d4 = (dt * dt) * (dt * dt)
    for m in range(N):
        t1a, t1b, t2aa, t2ab, t2bb, t2zz = six[m]
        Cm = [cc[m], cs[m], 0.0, -cs[m], cc[m], 0.0, 0.0, 0.0, float(m + 1)]
        t1 = [t1a, t1b, 0.0, -t1b, t1a, 0.0, 0.0, 0.0, float(((N - m) * (N - m - 1)) // 2)]
        t2 = [t2aa, t2ab, 0.0, t2ab, t2bb, 0.0, 0.0, 0.0, t2zz]
        for k in range(9):
            p, q = divmod(k, 3)
            e = [sq[0] * sq[0] * t1[q], sq[1] * sq[1] * t1[3 + q], sq[2] * sq[2] * t1[6 + q]]
            v = (t2[k] + Cm[p] * e[0] + Cm[3 + p] * e[1] + Cm[6 + p] * e[2]) * d4
            if p == q:
                v += float(N - m) * (dt * dt) * sq[6 + p] * sq[6 + p]
            D[m, p, q] = v
            E[m, p, q] = d4 * e[p]
    return D, E


# ---- the G'v tables: the step loops and the pair lanes ----------------------------------------------------------------------------
def gv_loop(cc, cs, sq, vec, dt):
    N = len(cc)
    dt2 = dt * dt
    C = np.zeros((N, 9))
    for k in range(N):
        C[k] = [cc[k], cs[k], 0.0, -cs[k], cc[k], 0.0, 0.0, 0.0, float(k + 1)]
    gv = np.zeros((N, 9))
    for j in range(N):
        for comp in range(3):
            acc = 0.0
            for i in range(N):
                v = vec[12 * i:12 * i + 12]
                term = dt2 * ((C[i][comp] - C[j][comp]) * (sq[0] * v[0]) + (C[i][3 + comp] - C[j][3 + comp]) * (sq[1] * v[1])
                              + (C[i][6 + comp] - C[j][6 + comp]) * (sq[2] * v[2])) + dt * (sq[6 + comp] * v[6 + comp])
                acc += term if i >= j else 0.0
            gv[j, comp] = acc
        for comp in range(3, 9):
            off = comp if comp < 6 else 3 + comp
            acc = 0.0
            for i in range(N):
                v = vec[12 * i + off]
                term = float(i - j) * v if comp < 6 else v
                acc += term if i >= j else 0.0
            gv[j, comp] = acc
    return gv


def gv_pairs(dab, sq, vec, dt, N):
    dt2 = dt * dt
    NP = N * (N + 1) // 2
    slot = np.full((N * N // 2 + N, 3), np.nan)
    for p in range(NP):
        m, i = pair_of_lane(p, N)
        da, db = dab[p]
        v = vec[12 * i:12 * i + 12]
        p0, p1, p2, dz = sq[0] * v[0], sq[1] * v[1], sq[2] * v[2], float(i - m)
        slot[p] = (dt2 * (da * p0 + (-db) * p1) + dt * (sq[6] * v[6]), dt2 * (db * p0 + da * p1) + dt * (sq[7] * v[7]), dt2 * (dz * p2) + dt * (sq[8] * v[8]))
    gv = np.zeros((N, 9))
    for lane in range(3 * N):
        j, comp = divmod(lane, 3)
        acc = 0.0
        for s in range(N):
            if s < N - j:
                acc += slot[pair_base(j, N) + s][comp]
        gv[j, comp] = acc
    for lane in range(6 * N):
        j, c6 = divmod(lane, 6)
        comp = 3 + c6
        off = comp if comp < 6 else 3 + comp
        winc = 1.0 if comp < 6 else 0.0
        acc, wt = 0.0, (0.0 if comp < 6 else 1.0)
        for s in range(N):
            if s < N - j:
                acc += wt * vec[12 * (j + s) + off]
            wt += winc
        gv[j, comp] = acc
    return gv


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def yaw_cases(N):
    rng = np.random.default_rng(300 + N)
    yield "zero", np.zeros(N)
    yield "constant", np.full(N, 0.3)
    yield "turn_more_than_pi", np.linspace(-0.2, 1.3 * np.pi - 0.2, N)
    yield "turn_back", -np.linspace(0.0, 1.1 * np.pi, N)
    yield "random", rng.uniform(-np.pi, np.pi, N)
    yield "slow", np.cumsum(rng.normal(0.0, 0.05, N)) + 0.7


HORIZONS = [4, 8, 10]


@pytest.mark.parametrize("N", HORIZONS)
def test_every_pair_has_one_lane_and_the_pairs_of_a_step_are_consecutive(N):
    NP = N * (N + 1) // 2
    assert NP <= 64
    pairs = [pair_of_lane(p, N) for p in range(NP)]
    assert sorted(pairs) == [(m, i) for m in range(N) for i in range(m, N)]
    for m in range(N):
        for s in range(N - m):
            assert pairs[pair_base(m, N) + s] == (m, m + s)
        assert pair_base(m, N) + N - 1 < N * N // 2 + N       # the last slot lane m could address


@pytest.mark.parametrize("N", HORIZONS)
def test_pair_sums_are_the_step_loops_sums_bit_for_bit(N):
    p = orc.default_params(N)
    sq = np.sqrt(np.asarray(p.q_diag, dtype=np.float64)[:12])
    w = sq[:3] * sq[:3]
    rng = np.random.default_rng(400 + N)
    for name, yaw in yaw_cases(N):
        cc, cs = prefix_cc_cs(yaw)
        loop = six_sums_loop(cc, cs, w)
        pairs, dab = six_sums_pairs(cc, cs, w)
        assert np.array_equal(loop, pairs), name
        vec = rng.normal(0.0, 1.0, 12 * N) * np.tile(sq, N)
        assert np.array_equal(gv_loop(cc, cs, sq, vec, p.dt), gv_pairs(dab, sq, vec, p.dt, N)), name


@pytest.mark.parametrize("N", HORIZONS)
def test_tables_against_the_oracles_step_loop_form(N):
    """T1 / T2 / D / E as closed_form_hessian_rank6 forms them (3 x 3 matrices, a loop over i >= m per step).  Every entry is a sum of at most N + 6 rounded terms, so
    it is held to 64 ulps of the size of its largest term (T1, T2: of the table's largest entry at that step)."""
    p = orc.default_params(N)
    wq = np.asarray(p.q_diag, dtype=np.float64)[:12]
    sq = np.sqrt(wq)
    W_th, W_om, dt = np.diag(wq[0:3]), np.diag(wq[6:9]), p.dt
    for name, yaw in yaw_cases(N):
        cc, cs = prefix_cc_cs(yaw)
        six, _ = six_sums_pairs(cc, cs, sq[:3] * sq[:3])
        D, E = de_from_six(six, cc, cs, sq, dt, N)
        C = np.cumsum(np.array([orc.rot_z(float(y)).T for y in yaw]), axis=0)
        for m in range(N):
            T1 = sum((C[i] - C[m] for i in range(m, N)), np.zeros((3, 3)))
            T2 = sum(((C[i] - C[m]).T @ W_th @ (C[i] - C[m]) for i in range(m, N)), np.zeros((3, 3)))
            t1a, t1b, t2aa, t2ab, t2bb, t2zz = six[m]
            mine1 = np.array([[t1a, t1b, 0.0], [-t1b, t1a, 0.0], [0.0, 0.0, float(((N - m) * (N - m - 1)) // 2)]])
            mine2 = np.array([[t2aa, t2ab, 0.0], [t2ab, t2bb, 0.0], [0.0, 0.0, t2zz]])
            assert np.abs(mine1 - T1).max() <= 64 * EPS * max(np.abs(T1).max(), 1e-300), (name, m)
            assert np.abs(mine2 - T2).max() <= 64 * EPS * max(np.abs(T2).max(), 1e-300), (name, m)
            Dm = dt ** 4 * (T2 + C[m].T @ W_th @ T1) + (N - m) * dt ** 2 * W_om
            Em = dt ** 4 * W_th @ T1
            scale = dt ** 4 * (np.abs(T2).max() + 3 * np.abs(C[m]).max() * wq[0:3].max() * np.abs(T1).max()) + (N - m) * dt ** 2 * wq[6:9].max()
            assert np.abs(D[m] - Dm).max() <= 64 * EPS * scale, (name, m)
            assert np.abs(E[m] - Em).max() <= 64 * EPS * max(np.abs(Em).max(), 1e-300), (name, m)


@pytest.mark.parametrize("N", HORIZONS)
def test_gradient_from_the_pair_tables_against_the_oracle(N):
    """q = s (J'g + ...) from the G'v table of the pair lanes against closed_form_hessian_gradient(), to the 1e-11 of the largest entry the assembly tests hold
    the kernels to."""
    p = orc.default_params(N)
    wq = np.asarray(p.q_diag, dtype=np.float64)[:12]
    sq = np.sqrt(wq)
    dt, s, inv_m = p.dt, p.force_scale, 1.0 / p.mass
    x0b, xrb, ftb, ctb = orc.synthetic_batch(6, N, seed=500 + N, schedule="single")
    for b, (name, yaw) in enumerate(yaw_cases(N)):
        x0, xr, ft, ct = x0b[b], xrb[b].copy(), ftb[b], ctb[b]
        xr[:, 2] = yaw
        _, q_ref, _ = orc.closed_form_hessian_gradient(p, x0, xr, ft, ct)
        cc, cs = prefix_cc_cs(yaw)
        _, dab = six_sums_pairs(cc, cs, sq[:3] * sq[:3])
        xf = np.asarray(x0, dtype=np.float64).reshape(13).copy()
        vec = np.zeros(12 * N)
        for i in range(N):
            xf = orc.linearise(p, float(xr[i, 2]), np.zeros((4, 3)))[0] @ xf
            vec[12 * i:12 * i + 12] = sq * (xf[:12] - xr[i, :12])
        gv = gv_pairs(dab, sq, vec, dt, N)
        Ib_inv = np.diag(1.0 / np.asarray(p.inertia, dtype=np.float64))
        foot = np.asarray(ft, dtype=np.float64).reshape(N, 4, 3)
        q = []
        for k in range(N):
            for i in range(4):
                if np.asarray(ct).reshape(N, 4)[k, i]:
                    Rz = orc.rot_z(float(xr[k, 2]))
                    J = Rz @ Ib_inv @ Rz.T @ orc.skew(foot[k, i] - xr[k, 3:6])
                    for ax in range(3):
                        q.append(s * (J[:, ax] @ gv[k, 0:3] + sq[3 + ax] * dt * dt * inv_m * gv[k, 3 + ax] + sq[9 + ax] * dt * inv_m * gv[k, 6 + ax]))
        q = np.array(q)
        assert q.shape == q_ref.shape and q.size > 0, name
        assert np.abs(q - q_ref).max() <= 1e-11 * np.abs(q_ref).max(), (name, np.abs(q - q_ref).max(), np.abs(q_ref).max())
