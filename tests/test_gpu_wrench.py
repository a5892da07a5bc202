"""GPU parity of the general kernel (srbdqp_wrench.hpp: any contact pattern, N = 4 ... 24, fp64 or fp32 iterations)
through the C-ABI against the CPU oracle on the same seeded inputs.

Tolerances, stated once:
  fp64 (srbdqp_solve_batch_f64, kernel = SRBDQP_KERNEL_WRENCH)
    * forces vs the oracle's ADMM twin (orc.update, dense presolved K):  <= 2e-3 N, iteration counts within one check interval
    * forces vs the independent exact QP optimum:                        <= 5e-2 N
  fp32 (srbdqp_solve_batch_f32; fp32 buffers and iterations, fp64 set-up; batches >= 512: T of the QPs without
        force-variable steps factored in fp32 tiles + one fp64 refinement step of x_q -- same tolerances)
    * forces vs the fp32 twin (orc.update_split, float32):               <= 2e-2 N, iteration counts within two check intervals
      (the twin's NumPy mat-vecs sum in another order than the kernel's; in fp32 that moves an iterate near the stopping
      threshold more often than in fp64)
    * forces vs the exact optimum of the QP built from the fp32-rounded inputs: <= 1e-1 N (5e-4 of a 200 N stance force)
    * KKT of the returned primal/dual pair, evaluated in fp64 on that QP: primal <= 1e-4, stationarity <= 1e-3 |q|_inf
"""
import numpy as np
import pytest

import srbd_oracle as orc
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TOL_TWIN_N = 2e-3
TOL_EXACT_N = 5e-2
TOL32_TWIN_N = 2e-2
TOL32_EXACT_N = 1e-1


def _engine(N, **kw):
    from g1_locomotion_amd import BatchMPC, _lib
    kw.setdefault("kernel", _lib.KERNEL_WRENCH)
    kw.setdefault("rho_restart_iter", -1)       # off unless the test is about it (the general kernel's default is 100)
    return BatchMPC(horizon=N, **kw)


def _batch(B, N, seed, schedule):
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=seed, schedule="mixed" if schedule == "three" else schedule)
    if schedule == "three":          # steps with exactly 3 stance contacts (6 wrench coordinates from 9 variables)
        rng = np.random.default_rng(seed)
        for b in range(B):
            for k in range(N):
                if ct[b, k].sum() == 4 or rng.random() < 0.3:
                    ct[b, k] = 1
                    ct[b, k, rng.integers(0, 4)] = 0
    return x0, xr, ft, ct


CASES = [(10, "single", 8), (10, "double", 8), (10, "mixed", 12), (10, "three", 8), (8, "mixed", 6), (4, "double", 6),
         (12, "mixed", 6), (16, "double", 6), (20, "double", 8), (20, "mixed", 6), (20, "three", 4), (24, "single", 4), (24, "mixed", 6)]


@pytest.mark.parametrize("N,schedule", [(4, "double"), (8, "mixed"), (10, "single"), (10, "double"), (10, "three"), (12, "mixed"), (16, "double"),
                                        (20, "double"), (20, "three"), (24, "mixed")])
def test_wrench_assembly_matches_oracle(torch_first, built_lib, N, schedule):
    """Rows a5-a8 on the general kernel as it ships (srbdqp_assemble_wrench_f64 = the solve kernel stopped before its
    factorisation): T = S + E^-1, the per-step blocks V and Bd, the gradient and the coordinate map against
    orc.wrench_reduce() at 1e-11, and the operator they define, K^-1 = Bd + V' T^-1 V, against the inverse of the oracle's
    DENSE K = B'QB + R + sigma I + A' rho A (the products north_star names) at 1e-8."""
    B = 4
    x0, xr, ft, ct = _batch(B, N, 500 + N, schedule)
    with _engine(N) as eng:
        d = eng.assemble_wrench(x0, xr, ft, ct)
    p = orc.params_for(N)
    for b in range(B):
        wr = orc.wrench_reduce(p, xr[b], ft[b], ct[b])
        ng, vi, goff = wr["n_g"], wr["vi"], wr["goff"]
        np.testing.assert_array_equal(d["goff"][b], goff)
        T = d["T"][b]
        assert np.abs(T[:ng, :ng] - wr["T"]).max() <= 1e-11 * np.abs(wr["T"]).max()
        assert np.all(T[ng:, :] == 0.0) and np.all(T[:, ng:] == 0.0)
        qp = orc.build_qp(p, x0[b], xr[b], ft[b], ct[b])
        red, vi2, ri = orc.presolve(qp, ct[b])
        assert np.abs(d["q"][b][vi] - red["q"]).max() <= 1e-11 * max(1.0, np.abs(red["q"]).max())
        off = np.setdiff1d(np.arange(12 * N), vi)
        assert np.all(d["q"][b][off] == 0.0) and np.all(d["Bd"][b][off] == 0.0) and np.all(d["Vcol"][b][off] == 0.0)
        # rebuild V (n_g x n_u) and Bd (n_u x n_u) from the per-variable rows the lanes hold
        nu = len(vi)
        V = np.zeros((ng, nu)); Bd = np.zeros((nu, nu))
        for idx, v in enumerate(vi):
            k = v // 12
            same = [i for i, vv in enumerate(vi) if vv // 12 == k]
            Bd[idx, same] = d["Bd"][b][v][[vi[i] % 12 for i in same]]
            V[goff[k]:goff[k + 1], idx] = d["Vcol"][b][v][:goff[k + 1] - goff[k]]
        assert np.abs(V - wr["V"]).max() <= 1e-11 * np.abs(wr["V"]).max()
        assert np.abs(Bd - wr["Bd"]).max() <= 1e-11 * max(np.abs(wr["Bd"]).max(), 1e-3)
        rho = orc.rho_vector(p, red["l"], red["u"])
        Kinv = np.linalg.inv(red["P"] + p.sigma * np.eye(nu) + (red["A"].T * rho) @ red["A"])
        Kw = Bd + V.T @ np.linalg.solve(T[:ng, :ng], V)
        assert np.abs(Kw - Kinv).max() <= 1e-8 * np.abs(Kinv).max()


@pytest.mark.parametrize("N,schedule,B", CASES)
def test_wrench_f64_matches_oracle_and_exact_optimum(torch_first, built_lib, N, schedule, B):
    x0, xr, ft, ct = _batch(B, N, 300 + N, schedule)
    with _engine(N) as eng:
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}", eng.kernel_name()
    p = orc.params_for(N)
    for b in range(B):
        ref = orc.update(p, x0[b], xr[b], ft[b], ct[b])
        assert out["status"][b] == ref["status"] and ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER), (b, out["status"][b], ref["status"])
        solved = ref["status"] == orc.STATUS_SOLVED
        assert abs(int(out["iters"][b]) - ref["iters"]) <= p.check_every, (b, out["iters"][b], ref["iters"])
        assert np.abs(out["u"][b] - ref["u"]).max() <= TOL_TWIN_N, (b, np.abs(out["u"][b] - ref["u"]).max())
        assert np.abs(out["x"][b] - ref["x"]).max() <= 1e-5
        kq, vi, ri = orc.presolve(ref["qp"], ct[b])
        if solved:   # a QP that ends at the iteration cap (status MAX_ITER, on the oracle too) is only held to its twin
            xs, ys = orc.solve_reference(p, ref["qp"])
            assert np.abs(out["u"][b].reshape(-1) - xs * p.force_scale).max() <= TOL_EXACT_N
            kr = orc.kkt_residuals(kq["P"], kq["q"], kq["A"], kq["l"], kq["u"], out["u"][b].reshape(-1)[vi] / p.force_scale, out["y"][b][ri])
            assert kr["primal"] <= 1e-4 and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(ref["qp"]["q"]).max()), kr
        off = np.setdiff1d(np.arange(12 * N), vi)
        assert np.all(out["u"][b].reshape(-1)[off] == 0.0)              # swing contacts carry exactly zero force
        offr = np.setdiff1d(np.arange(20 * N), ri)
        assert np.all(out["y"][b][offr] == 0.0)


@pytest.mark.parametrize("N,schedule,B", [(20, "double", 12), (20, "mixed", 6), (10, "double", 8), (10, "single", 8), (16, "three", 4), (24, "mixed", 4)])
def test_wrench_f32_matches_twin_and_exact_optimum(torch_first, built_lib, N, schedule, B):
    """BASELINE.json configs[2] shape (N = 20, 4-contact double support, fp32) and the other patterns through the _f32
    entry points."""
    x0, xr, ft, ct = _batch(B, N, 400 + N, schedule)
    with _engine(N) as eng:
        out = eng.solve(x0, xr, ft, ct, want_y=True, dtype=np.float32)
        assert eng.kernel_name() == f"wrench_f32_n{N}", eng.kernel_name()
    assert out["u"].dtype == np.float32 and out["x"].dtype == np.float32
    p = orc.params_for(N, eps_abs=2e-6, eps_rel=2e-6)       # the fp32 path's tolerance floor
    for b in range(B):
        ref = orc.update_split(p, x0[b], xr[b], ft[b], ct[b], dtype=np.float32)
        assert out["status"][b] == ref["status"] == orc.STATUS_SOLVED, (b, out["status"][b], ref["status"], out["iters"][b], ref["iters"])
        assert abs(int(out["iters"][b]) - ref["iters"]) <= 2 * p.check_every, (b, out["iters"][b], ref["iters"])
        assert np.abs(out["u"][b] - ref["u"]).max() <= TOL32_TWIN_N, (b, np.abs(out["u"][b] - ref["u"]).max())
        assert np.abs(out["x"][b] - ref["x"]).max() <= 1e-3          # fp32 roll-out of forces that agree to TOL32_TWIN_N
        xs, ys = orc.solve_reference(p, ref["qp"])
        assert np.abs(out["u"][b].reshape(-1).astype(np.float64) - xs * p.force_scale).max() <= TOL32_EXACT_N
        kq, vi, ri = orc.presolve(ref["qp"], ct[b])
        kr = orc.kkt_residuals(kq["P"], kq["q"], kq["A"], kq["l"], kq["u"], out["u"][b].reshape(-1).astype(np.float64)[vi] / p.force_scale,
                               out["y"][b].astype(np.float64)[ri])
        assert kr["primal"] <= 1e-4 and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(ref["qp"]["q"]).max()), kr


@pytest.mark.parametrize("N,schedule,B", [(20, "double", 12), (24, "double", 4), (16, "three", 6), (12, "double", 6), (10, "double", 8), (8, "three", 6), (4, "double", 6), (20, "mixed", 8)])
def test_wrench_f32_tiles_match_twin_and_exact_optimum(torch_first, built_lib, N, schedule, B):
    """The fp32-tile instantiation (what an _f32 call of >= 512 QPs runs for the QPs whose steps all have 0 or >= 3 stance
    contacts; SRBDQP_FLAG_F32_TILES forces it at test sizes): T factored and inverted in fp32 MFMA tiles, x_q refined
    once with the fp64 residual.  Against the twin with the same rule (tile_dtype="auto": float32 Cholesky of T + the
    refinement step) and the exact optimum; the "mixed" batch sends its QPs through both launches of the call."""
    from g1_locomotion_amd import _lib
    x0, xr, ft, ct = _batch(B, N, 500 + N, "double" if schedule == "three" else schedule)
    if schedule == "three":                          # 3 or 4 stance contacts on every step
        rng = np.random.default_rng(N)
        for b in range(B):
            for k in range(N):
                if rng.random() < 0.5:
                    ct[b, k, rng.integers(0, 4)] = 0
    if schedule == "mixed":
        ct[::2] = 1                                  # every other QP in full double support: eligible for fp32 tiles
        ct[0, 3:5] = 0                               # ... one of them with a flight phase (0 contacts: still eligible)
    with _engine(N, flags=_lib.FLAG_F32_TILES) as eng:
        out = eng.solve(x0, xr, ft, ct, want_y=True, dtype=np.float32)
        assert eng.kernel_name() == f"wrench_f32_n{N}", eng.kernel_name()
    p = orc.params_for(N, eps_abs=2e-6, eps_rel=2e-6)
    n32 = 0
    for b in range(B):
        n32 += orc.fp32_tiles_ok(ct[b])
        ref = orc.update_split(p, x0[b], xr[b], ft[b], ct[b], dtype=np.float32, tile_dtype="auto")
        assert out["status"][b] == ref["status"] == orc.STATUS_SOLVED, (b, out["status"][b], ref["status"], out["iters"][b], ref["iters"])
        assert abs(int(out["iters"][b]) - ref["iters"]) <= 2 * p.check_every, (b, out["iters"][b], ref["iters"])
        assert np.abs(out["u"][b] - ref["u"]).max() <= TOL32_TWIN_N, (b, np.abs(out["u"][b] - ref["u"]).max())
        assert np.abs(out["x"][b] - ref["x"]).max() <= 1e-3
        xs, ys = orc.solve_reference(p, ref["qp"])
        assert np.abs(out["u"][b].reshape(-1).astype(np.float64) - xs * p.force_scale).max() <= TOL32_EXACT_N
        kq, vi, ri = orc.presolve(ref["qp"], ct[b])
        kr = orc.kkt_residuals(kq["P"], kq["q"], kq["A"], kq["l"], kq["u"], out["u"][b].reshape(-1).astype(np.float64)[vi] / p.force_scale,
                               out["y"][b].astype(np.float64)[ri])
        assert kr["primal"] <= 1e-4 and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(ref["qp"]["q"]).max()), kr
        off = np.setdiff1d(np.arange(12 * N), vi)
        assert np.all(out["u"][b].reshape(-1)[off] == 0.0)
    assert n32 == (B if schedule != "mixed" else B // 2), n32          # the case exercises what its name says


def test_f32_tile_flags_select_the_factorisation(torch_first, built_lib):
    """SRBDQP_FLAG_F64_TILES / _F32_TILES and the batch threshold: same QPs, forces within the fp32 path's twin tolerance of
    each other, and not bit-identical between the two factorisations (so the flag really switches the kernel)."""
    from g1_locomotion_amd import _lib
    N, B = 20, 16
    x0, xr, ft, ct = _batch(B, N, 61, "double")
    res = {}
    for name, flags in (("default", 0), ("f32", _lib.FLAG_F32_TILES), ("f64", _lib.FLAG_F64_TILES)):
        with _engine(N, flags=flags) as eng:
            res[name] = eng.solve(x0, xr, ft, ct, dtype=np.float32)
    assert np.array_equal(res["default"]["u"], res["f64"]["u"])        # below 512 QPs a call stays on fp64 tiles
    assert not np.array_equal(res["f32"]["u"], res["f64"]["u"])
    assert np.abs(res["f32"]["u"].astype(np.float64) - res["f64"]["u"]).max() <= TOL32_TWIN_N
    assert (res["f32"]["status"] == orc.STATUS_SOLVED).all()


def test_f32_host_call_above_the_tile_threshold_takes_both_launches(torch_first, built_lib):
    """A host-buffer _f32 call of >= 512 QPs with mixed patterns: the eligible QPs go through the fp32-tile launch, the others
    through the fp64-tile one (no flag set).  Every QP is solved by exactly one of them: statuses / iteration counts are
    written once, the eligible QPs differ from an all-fp64-tile solve only within the twin tolerance and the others not at all."""
    from g1_locomotion_amd import _lib
    N, B = 12, 640
    x0, xr, ft, ct = _batch(B, N, 71, "mixed")
    ct[::2] = 1                                      # every other QP in full double support
    with _engine(N) as eng:
        auto = eng.solve(x0, xr, ft, ct, dtype=np.float32)
    with _engine(N, flags=_lib.FLAG_F64_TILES) as eng:
        ref = eng.solve(x0, xr, ft, ct, dtype=np.float32)
    elig = np.array([orc.fp32_tiles_ok(ct[b]) for b in range(B)])
    assert elig.sum() == B // 2
    assert (auto["status"] == orc.STATUS_SOLVED).mean() >= 0.99 and (auto["iters"] > 0).all()
    assert np.array_equal(auto["u"][~elig], ref["u"][~elig]) and np.array_equal(auto["iters"][~elig], ref["iters"][~elig])
    both = elig & (auto["status"] == orc.STATUS_SOLVED) & (ref["status"] == orc.STATUS_SOLVED)
    assert not np.array_equal(auto["u"][elig], ref["u"][elig])
    assert np.abs(auto["u"][both].astype(np.float64) - ref["u"][both]).max() <= TOL32_TWIN_N


def test_wrench_warm_start_and_edge_cases(torch_first, built_lib):
    N, B = 20, 6
    x0, xr, ft, ct = _batch(B, N, 77, "double")
    ct[1] = 0                                    # flight over the whole horizon: nothing to solve
    ct[2, 5:9] = 0                               # a flight phase inside the horizon
    with _engine(N) as eng:
        cold = eng.solve(x0, xr, ft, ct, want_y=True)
        warm = eng.solve(x0, xr, ft, ct, warm_u=cold["u"].reshape(B, -1), warm_y=cold["y"], want_y=True)
    assert cold["status"][1] == orc.STATUS_SOLVED and cold["iters"][1] == 0 and np.all(cold["u"][1] == 0.0)
    p = orc.params_for(N)
    for b in range(B):
        ref = orc.update(p, x0[b], xr[b], ft[b], ct[b])
        assert cold["status"][b] == ref["status"]
        assert np.abs(cold["u"][b] - ref["u"]).max() <= TOL_TWIN_N
        assert np.abs(cold["x"][b] - ref["x"]).max() <= 1e-5
    assert (warm["status"] == orc.STATUS_SOLVED).all()
    ok = (cold["status"] == orc.STATUS_SOLVED)
    assert (warm["iters"][ok] <= 10).all(), (warm["iters"], cold["iters"], cold["status"])
    assert np.abs(warm["u"][ok] - cold["u"][ok]).max() <= TOL_TWIN_N


@pytest.mark.parametrize("N,schedule,B,dtype", [(20, "single", 48, np.float64), (24, "mixed", 32, np.float64), (20, "mixed", 32, np.float32)])
def test_wrench_in_kernel_rho_restart_matches_the_oracle(torch_first, built_lib, N, schedule, B, dtype):
    """rho_restart_iter on the general kernel: the stragglers repeat their set-up with OSQP's re-balanced rho inside the
    same launch.  Against the oracle twin with the same rule; the long single-support horizons are where the tail is."""
    x0, xr, ft, ct = _batch(B, N, 900 + N, schedule)
    f32 = dtype == np.float32
    kw = dict(rho_restart_iter=60, max_iter=300)
    with _engine(N, **kw) as eng:
        out = eng.solve(x0, xr, ft, ct, want_y=True, dtype=dtype)
    p = orc.params_for(N, **kw, **(dict(eps_abs=2e-6, eps_rel=2e-6) if f32 else {}))
    restarted = 0
    for b in range(B):
        ref = orc.update_split(p, x0[b], xr[b], ft[b], ct[b], dtype=dtype)
        restarted += ref["iters"] > 60
        assert out["status"][b] == ref["status"], (b, out["status"][b], ref["status"], out["iters"][b], ref["iters"])
        # (a restarted fp32 QP: rho' comes from fp32 maxima, so rounding differences of the first pass move the second pass's
        # stopping mark by up to a few check intervals; the forces are held to the twin all the same)
        slack = (4 if ref["iters"] > 60 else 2) if f32 else 1
        assert abs(int(out["iters"][b]) - ref["iters"]) <= slack * p.check_every, (b, out["iters"][b], ref["iters"])
        assert np.abs(out["u"][b] - ref["u"]).max() <= (TOL32_TWIN_N if f32 else TOL_TWIN_N), (b, np.abs(out["u"][b] - ref["u"]).max())
    assert restarted >= 3, restarted          # the case must exercise the second pass


def test_auto_routes_four_contact_long_horizons_to_the_general_kernel(torch_first, built_lib):
    """What round 1 answered with SRBDQP_CONTACT_BOUND: > 2 stance contacts per step at N > 10."""
    from g1_locomotion_amd import BatchMPC
    N, B = 20, 4
    x0, xr, ft, ct = _batch(B, N, 5, "double")
    with BatchMPC(horizon=N) as eng:
        out = eng.solve(x0, xr, ft, ct)
        assert eng.kernel_name() == "wrench_f64_n20"
    assert (out["status"] == orc.STATUS_SOLVED).all()


def test_full_size_f32_batch_properties(torch_first, built_lib):
    """configs[2] at its full size (B = 65,536, N = 20, double support, fp32 buffers resident in HBM): size-independent
    properties -- every QP solved, every force inside its friction cone and normal-force bounds, the roll-out consistent
    with the forces (linear model re-applied on the host for a sample), and a 64-QP sample against the exact optimum."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    N, B = 20, 65536
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=2026, schedule="double")
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(v.astype(np.float32) if v.dtype == np.float64 else v).to(dev) for v in (x0, xr, ft, ct)]
    u = torch.zeros((B, N, 12), dtype=torch.float32, device=dev)
    xo = torch.zeros((B, N + 1, 13), dtype=torch.float32, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    it = torch.zeros(B, dtype=torch.int32, device=dev)
    with BatchMPC(horizon=N) as eng:                    # defaults: rho = 0.7 / 2.8 (friction / normal-force rows) at this horizon, rho restart after 125 iterations
        eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), x_out=xo.data_ptr(),
                         status=st.data_ptr(), iters=it.data_ptr(), f32=True)
        eng.synchronize()
        assert eng.kernel_name() == "wrench_f32_n20"
    u, xo, st, it = u.cpu().numpy().astype(np.float64), xo.cpu().numpy().astype(np.float64), st.cpu().numpy(), it.cpu().numpy()
    assert (st == orc.STATUS_SOLVED).mean() >= 0.998, np.bincount(st + 2)   # (measured 0.9989 with the round-3 penalties, 0.9995 with round 2's at 1.6 x the iterations)
    p = orc.params_for(N)
    f = u.reshape(B, N, 4, 3)
    ok = st == orc.STATUS_SOLVED
    fz = f[ok][..., 2]
    assert fz.min() >= p.fz_min - 2e-2 and fz.max() <= p.fz_max + 2e-2
    assert (np.abs(f[ok][..., 0]) <= p.mu * fz + 2e-2).all() and (np.abs(f[ok][..., 1]) <= p.mu * fz + 2e-2).all()
    assert np.isfinite(u).all() and np.isfinite(xo).all()
    rng = np.random.default_rng(0)
    for b in rng.choice(np.where(ok)[0], 64, replace=False):
        xin = [np.asarray(v[b], np.float32).astype(np.float64) for v in (x0, xr, ft)]
        qp = orc.build_qp(p, xin[0], xin[1], xin[2], ct[b])
        xs, _ = orc.solve_reference(p, qp)
        assert np.abs(u[b].reshape(-1) - xs * p.force_scale).max() <= TOL32_EXACT_N
        assert np.abs(xo[b] - orc.rollout(qp, xin[0], u[b].reshape(-1) / p.force_scale, p.force_scale)).max() <= 1e-4
