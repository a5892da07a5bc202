"""CPU tests of the oracles on turning, stepping and uneven-ground horizons (tests/scenarios.py::turning_batch): the references must hold
their own bounds on these inputs before tests/test_gpu_turning.py may judge a kernel with them, and the inputs must be of the kind that
exposes a kernel reading the wrong step's yaw or foothold.

Bounds, all taken from the existing CPU tests of the same kind (tests/test_oracle.py):
  * closed-form assembly vs the dense products: 1e-12 relative (P and q); rank-6 form: 1e-12 vs the pair form, 2e-12 vs the dense products
  * condensation vs step-by-step simulation: rtol = atol = 1e-12
  * C oracle vs NumPy oracle: status equal, iterations within one check interval, forces < 1e-6 N where the iteration counts are equal
    (two QPs that stop one check apart differ by what five ADMM iterations move: held to the twin bound of the GPU tests, 2e-3 N)
  * fp64 twin vs the exact optimum 5e-2 N, fp32 twin (either tile rule) 1e-1 N: the GPU files' TOL_EXACT_N / TOL32_EXACT_N
  * wrench_reduce's Bd + V' T^-1 V vs the inverse of the dense K: 1e-8 relative, against a reference inverse refined in extended precision
"""
import os

import numpy as np
import pytest

import scenarios as sc
import srbd_oracle as orc

KINDS = sc.YAW_KINDS
HORIZONS = (4, 8, 10, 12, 16, 20, 24)
SCHEDULES = ("single", "double", "mixed")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "srbd_turning_golden.npz")
GOLDEN_CASES = [("n10_turn_single", 10), ("n10_wrap_mixed", 10), ("n10_turn_double", 10), ("n8_wrap_mixed", 8), ("n4_random_double", 4),
                ("n20_turn_double", 20)]


def _seed(N, schedule, yaw):
    return 3000 + 10 * N + 3 * SCHEDULES.index(schedule) + KINDS.index(yaw)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("yaw", KINDS)
def test_generator_varies_what_the_old_one_holds_constant(yaw, schedule):
    """What turning_batch() is for: yaw differs between steps, the footholds differ between at least two steps of most QPs, some foot height is
    non-zero, and the six reference columns synthetic_batch() leaves at 0 are not 0.  The contact schedule and the x0 ranges are the old ones."""
    B, N = 32, 10
    x0, xr, ft, ct = sc.turning_batch(B, N, 11, schedule, yaw=yaw)
    o0, oxr, oft, oct_ = orc.synthetic_batch(B, N, 11, schedule)
    np.testing.assert_array_equal(ct, oct_)
    keep = [0, 1] + list(range(3, 13))
    np.testing.assert_array_equal(x0[:, keep], o0[:, keep])
    assert yaw == "turn" or np.all(np.abs(xr[:, :, 2]) <= np.pi)          # ("turn" is a plain ramp from x0's yaw: it may leave (-pi, pi])
    assert np.all(np.ptp(np.cos(xr[:, :, 2]), axis=1) > 0) and np.all(np.ptp(np.sin(xr[:, :, 2]), axis=1) > 0)
    for b in range(B):
        assert len(np.unique(xr[b, :, 2])) == N, "the yaw of every step is its own"
    if yaw == "wrap":                                          # crosses +-pi inside the horizon: a jump of ~2 pi between two neighbours
        assert np.all(np.abs(np.diff(xr[:, :, 2], axis=1)).max(1) > 6.0)
    moved = np.array([np.abs(ft[b] - ft[b, 0]).max() > 0.01 for b in range(B)])
    assert moved.mean() >= 0.75, moved.mean()
    assert np.abs(ft.reshape(B, N, 4, 3)[..., 2]).max() > 0.02 and (ft.reshape(B, N, 4, 3)[..., 2] != 0).mean() > 0.99
    heel_toe = ft.reshape(B, N, 2, 2, 3)
    assert np.abs(heel_toe[:, :, :, 0, 2] - heel_toe[:, :, :, 1, 2]).max() > 0
    for col in sc.ZERO_COLUMNS + (8,):
        assert np.all(oxr[:, :, col] == 0.0)
        assert (xr[:, :, col] != 0.0).mean() > 0.99, col
    assert np.all(np.ptp(xr[:, :, 5], axis=1) > 0)
    # heel-toe lines of the two feet are not parallel (a foot yaw of its own)
    d = heel_toe[:, 0, :, 1, :2] - heel_toe[:, 0, :, 0, :2]
    cross = d[:, 0, 0] * d[:, 1, 1] - d[:, 0, 1] * d[:, 1, 0]
    assert (np.abs(cross) > 1e-4).mean() > 0.9
    x0p, xrp, ftp, ctp, pc = sc.turning_batch(B, N, 11, schedule, yaw=yaw, pcom=True)
    np.testing.assert_array_equal(ftp, ft)
    assert 0.0 < np.abs(pc - xr[:, :, 3:6]).max() <= 0.03


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("N", HORIZONS)
@pytest.mark.parametrize("yaw", KINDS)
def test_closed_form_and_rank6_assembly_equal_the_dense_products(yaw, N, schedule):
    p = orc.params_for(N)
    x0, xr, ft, ct, pc = sc.turning_batch(3, N, _seed(N, schedule, yaw), schedule, yaw=yaw, pcom=True)
    for b in range(3):
        pcom = pc[b] if b == 2 else None
        red, vi, ri = orc.presolve(orc.build_qp(p, x0[b], xr[b], ft[b], ct[b], pcom_hor=pcom), ct[b])
        P, q, vi2 = orc.closed_form_hessian_gradient(p, x0[b], xr[b], ft[b], ct[b], pcom_hor=pcom)
        np.testing.assert_array_equal(vi, vi2)
        sP = np.abs(red["P"]).max()
        assert np.abs(P - red["P"]).max() <= 1e-12 * sP
        assert np.abs(q - red["q"]).max() <= 1e-12 * max(1.0, np.abs(red["q"]).max())
        P6 = orc.closed_form_hessian_rank6(p, xr[b], ft[b], ct[b], pcom_hor=pcom)
        assert np.abs(P6 - P).max() <= 1e-12 * sP and np.abs(P6 - red["P"]).max() <= 2e-12 * sP


@pytest.mark.parametrize("yaw,N,schedule", [("turn", 10, "single"), ("wrap", 10, "mixed"), ("random", 8, "double"), ("wrap", 24, "mixed"), ("turn", 20, "double")])
def test_condensation_equals_step_by_step_simulation(yaw, N, schedule):
    p = orc.SrbdParams()
    x0, xr, ft, ct, pc = (a[0] for a in sc.turning_batch(1, N, _seed(N, schedule, yaw), schedule, yaw=yaw, pcom=True))
    A_qp, B_qp = orc.condense(p, xr[:, 2], ft, pc)
    U = np.random.default_rng(1).normal(size=(N, 12)) * 30
    x = x0.copy()
    for k in range(N):
        A, B = orc.linearise(p, xr[k, 2], ft[k].reshape(4, 3) - pc[k])
        x = A @ x + B @ U[k]
        assert np.allclose((A_qp @ x0 + B_qp @ U.reshape(-1))[13 * k:13 * (k + 1)], x, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("yaw,N,schedule", [("turn", 10, "single"), ("wrap", 10, "mixed"), ("random", 10, "double"), ("turn", 4, "double"), ("wrap", 8, "single"),
                                            ("turn", 16, "single"), ("wrap", 20, "double"), ("turn", 24, "mixed")])
def test_c_restatement_agrees_with_numpy_oracle(yaw, N, schedule, restart):
    import c_oracle
    B = 6
    x0, xr, ft, ct = sc.turning_batch(B, N, _seed(N, schedule, yaw), schedule, yaw=yaw)
    p = orc.default_params(N) if restart else orc.params_for(N)
    out = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=4)
    for b in range(B):
        o = orc.update(p, x0[b], xr[b], ft[b], ct[b])
        assert o["status"] == out["status"][b] and abs(o["iters"] - int(out["iters"][b])) <= p.check_every, (b, o["iters"], out["iters"][b])
        err = np.abs(o["u"] - out["u"][b]).max()
        assert err < (1e-6 if o["iters"] == out["iters"][b] else 2e-3), (b, err)
        assert np.abs(o["x"] - out["x"][b]).max() < 1e-6
    a = c_oracle.assemble(p, x0[0], xr[0], ft[0], ct[0])
    qp = orc.build_qp(p, x0[0], xr[0], ft[0], ct[0])
    assert np.allclose(a["q"], qp["q"], rtol=1e-11, atol=1e-8) and np.allclose(a["P"], qp["P"], rtol=1e-11, atol=1e-8)


@pytest.mark.parametrize("yaw,N,schedule", [("turn", 10, "double"), ("wrap", 12, "mixed"), ("random", 8, "mixed"), ("turn", 20, "double"), ("wrap", 16, "single")])
def test_twins_stop_within_their_bounds_of_the_exact_optimum(yaw, N, schedule):
    """The NumPy ADMM twins the GPU tests compare with -- fp64 dense (orc.update), fp32 split with fp64 tiles and with the fp32-tile rule
    (orc.update_split) -- against the independent exact optimum, on the QPs each of them solves."""
    B = 4
    x0, xr, ft, ct = sc.turning_batch(B, N, _seed(N, schedule, yaw), schedule, yaw=yaw)
    p, p32 = orc.params_for(N), orc.params_for(N, eps_abs=2e-6, eps_rel=2e-6)
    solved = 0
    for b in range(B):
        qp = orc.build_qp(p, x0[b], xr[b], ft[b], ct[b])
        xs, _ = orc.solve_reference(p, qp)
        kr = orc.kkt_residuals(qp["P"], qp["q"], qp["A"], qp["l"], qp["u"], xs, _)
        assert max(kr.values()) < 1e-8 * max(1.0, np.abs(qp["q"]).max()), kr
        for ref, tol in ((orc.update(p, x0[b], xr[b], ft[b], ct[b]), 5e-2),
                         (orc.update_split(p32, x0[b], xr[b], ft[b], ct[b], dtype=np.float32), 1e-1),
                         (orc.update_split(p32, x0[b], xr[b], ft[b], ct[b], dtype=np.float32, tile_dtype="auto"), 1e-1)):
            assert ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER)
            if ref["status"] == orc.STATUS_SOLVED:
                solved += 1
                assert np.abs(ref["u"].reshape(-1).astype(np.float64) - xs * p.force_scale).max() <= tol, (b, tol)
    assert solved >= 9, solved


@pytest.mark.parametrize("yaw,N,schedule", [("turn", 4, "double"), ("wrap", 8, "mixed"), ("random", 10, "single"), ("turn", 10, "three"), ("wrap", 12, "mixed"),
                                            ("random", 16, "double"), ("turn", 20, "three"), ("wrap", 24, "mixed"), ("random", 24, "double")])
def test_wrench_reduction_is_the_inverse_of_the_dense_k(yaw, N, schedule):
    p = orc.params_for(N)
    x0, xr, ft, ct, pc = sc.batch(2, N, _seed(N, "mixed" if schedule == "three" else schedule, yaw), schedule, yaw=yaw, pcom=True)
    for b in range(2):
        pcom = pc[b] if b else None
        wr = orc.wrench_reduce(p, xr[b], ft[b], ct[b], pcom_hor=pcom)
        red, vi, ri = orc.presolve(orc.build_qp(p, x0[b], xr[b], ft[b], ct[b], pcom_hor=pcom), ct[b])
        np.testing.assert_array_equal(vi, wr["vi"])
        Kinv, res = sc.refined_inverse(sc.dense_k(p, red))
        assert res <= 1e-11
        Kw = wr["Bd"] + wr["V"].T @ np.linalg.solve(wr["T"], wr["V"])
        assert np.abs(Kw - Kinv).max() <= 1e-8 * np.abs(Kinv).max(), np.abs(Kw - Kinv).max() / np.abs(Kinv).max()


def test_wrench_reference_holds_the_assembly_bound_on_the_gpu_inputs():
    """tests/test_gpu_turning.py holds the general kernel's V and Bd blocks to 1e-11 of orc.wrench_reduce()'s.  That reference inverts a 6 x 6 matrix E
    per step in float64; where the three stance contacts of a step are nearly collinear cond(E) reaches 1e8 and the reference itself is 1e-11 off (seen
    on the first draw of the N = 20 "three" random-yaw case: 1.1e-11, cond E = 9.9e7).  On every input of the GPU assembly test the reference's own
    error, against the same blocks formed in extended precision, stays under 3e-12: at least 7/10 of the bound is the kernel's."""
    import test_gpu_turning as t
    worst = 0.0
    for N, schedule in t.WRENCH_ASM:
        p = orc.params_for(N)
        for yaw in KINDS:
            x0, xr, ft, ct, pc = t._inputs(N, schedule, yaw, t.B_ASM)
            for b in range(t.B_ASM):
                for pcom in (None, pc[b]):
                    eV, eB, cond = sc.wrench_blocks_reference_error(p, xr[b], ft[b], ct[b], pcom=pcom)
                    worst = max(worst, eV, eB)
                    assert max(eV, eB) <= 3e-12, (N, schedule, yaw, b, eV, eB, cond)
    print(f"reference's own error in V / Bd on the GPU assembly inputs: {worst:.1e}")


def test_refined_inverse_beats_the_float64_one():
    """The helper refines: on the worst-conditioned K of the set (N = 24) its residual is far below np.linalg.inv's, and a K it cannot invert
    to its tolerance is refused, not handed out."""
    p = orc.params_for(24)
    x0, xr, ft, ct = (a[0] for a in sc.turning_batch(1, 24, 5, "mixed", yaw="wrap"))
    red, vi, ri = orc.presolve(orc.build_qp(p, x0, xr, ft, ct), ct)
    K = sc.dense_k(p, red)
    X, res = sc.refined_inverse(K)
    plain = np.abs(np.eye(len(K), dtype=np.longdouble) - K.astype(np.longdouble) @ np.linalg.inv(K).astype(np.longdouble)).max()
    assert res <= 1e-11 and res < 1e-2 * plain, (res, plain)
    with pytest.raises(AssertionError):
        sc.refined_inverse(K, tol=1e-30)


@pytest.mark.parametrize("yaw", ["turn", "wrap"])
def test_a_wrong_step_index_is_invisible_on_the_old_inputs_and_visible_on_these(yaw):
    """Why this generator exists, without touching a kernel: the ORACLE is fed a deliberately wrong view of the inputs -- the yaw of step k + 1
    in the place of step k's; the foothold row of step 0 on every step -- and compared with itself on the true inputs (N = 10, mixed).
    On synthetic_batch() both mutations change nothing at all: P, q and the forces are bit-identical, which is the gap.  On turning_batch()
    they move the Hessian of every QP by more than 100 x the GPU assembly bound (1e-11 relative) and the forces by more than 100 x the GPU twin
    bound (2e-3 N; measured: yaw shift dP 2e-5 .. 2e-4 of max|P|, forces 0.09 .. 0.33 N turn / 5 .. 13 N wrap; stale foothold 13 .. 140 N), so a kernel with either fault cannot pass tests/test_gpu_turning.py, and the generator cannot drift back to inputs that hide it."""
    p = orc.params_for(10)
    B, N = 6, 10
    TOL_ASM, TOL_TWIN_N = 1e-11, 2e-3                       # the bounds of tests/test_gpu_turning.py

    def both(x0, xr, ft, ct):
        qp = orc.build_qp(p, x0, xr, ft, ct)
        return qp["P"], qp["q"], orc.solve_reference(p, qp)[0] * p.force_scale

    x0, xr, ft, ct = orc.synthetic_batch(B, N, 21, "mixed")
    for b in range(B):
        P, q, u = both(x0[b], xr[b], ft[b], ct[b])
        for xm, fm in ((sc.yaw_of_next_step(xr[b]), ft[b]), (xr[b], sc.foothold_of_step0(ft[b]))):
            Pm, qm, um = both(x0[b], xm, fm, ct[b])
            assert np.array_equal(Pm, P) and np.array_equal(qm, q) and np.array_equal(um, u)
    x0, xr, ft, ct = sc.turning_batch(B, N, 21, "mixed", yaw=yaw)
    dP_yaw, du_yaw, du_foot = [], [], []
    for b in range(B):
        P, q, u = both(x0[b], xr[b], ft[b], ct[b])
        Pm, qm, um = both(x0[b], sc.yaw_of_next_step(xr[b]), ft[b], ct[b])
        dP_yaw.append(np.abs(Pm - P).max() / np.abs(P).max()); du_yaw.append(np.abs(um - u).max())
        Pm, qm, um = both(x0[b], xr[b], sc.foothold_of_step0(ft[b]), ct[b])
        du_foot.append(np.abs(um - u).max())
    print(f"{yaw}: yaw shift dP/|P| {min(dP_yaw):.1e} .. {max(dP_yaw):.1e}, du {min(du_yaw):.2f} .. {max(du_yaw):.2f} N; stale foothold du {min(du_foot):.1f} .. {max(du_foot):.1f} N")
    assert min(dP_yaw) >= 100 * TOL_ASM, dP_yaw
    # forces: the batch's worst QP by 100 x the bound, and EVERY QP by more than the bound itself (a QP that turns slowly moves little under the
    # yaw shift -- the deviation scales with its yaw rate -- but still fails on its own)
    assert max(du_yaw) >= 100 * TOL_TWIN_N and min(du_yaw) > TOL_TWIN_N, du_yaw
    assert min(du_foot) >= 100 * TOL_TWIN_N, du_foot


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("name,N", GOLDEN_CASES)
def test_turning_golden_vectors_are_reproduced(gold, name, N):
    """tests/golden/srbd_turning_golden.npz (tests/golden/make_turning_golden.py), as tests/test_oracle.py::test_golden_vectors_are_reproduced
    holds the constant-yaw file: QP data, exact optimum and the ADMM twin's iterate do not move when the oracle is edited."""
    p = orc.params_for(N)
    x0, xr, ft, ct = (gold[f"{name}/{k}"] for k in ("x0", "x_ref", "foot", "contact"))
    assert len(np.unique(xr[:, 2])) == N and np.abs(ft - ft[0]).max() > 0.01
    qp = orc.build_qp(p, x0, xr, ft, ct)
    assert np.allclose(qp["q"], gold[f"{name}/q"], rtol=1e-12, atol=1e-9)
    assert np.allclose(np.diag(qp["P"]), gold[f"{name}/P_diag"], rtol=1e-12)
    assert np.allclose(qp["P"].sum(1), gold[f"{name}/P_rowsum"], rtol=1e-11, atol=1e-6)
    xs, ys = orc.solve_reference(p, qp)
    assert np.abs(xs * p.force_scale - gold[f"{name}/u_exact"].reshape(-1)).max() < 1e-6
    assert np.abs(orc.rollout(qp, x0, xs, p.force_scale) - gold[f"{name}/x_exact"]).max() < 1e-8
    tw = orc.update(p, x0, xr, ft, ct)
    assert tw["status"] == orc.STATUS_SOLVED and tw["iters"] == int(gold[f"{name}/iters_admm"])
    assert np.abs(tw["u"] - gold[f"{name}/u_admm"]).max() < 1e-7
    assert np.abs(tw["u"] - gold[f"{name}/u_exact"]).max() < 5e-3
