"""GPU parity tests proper: the HIP path (through the C-ABI) against the CPU oracle on the same seeded inputs.

Tolerances (fp64 path), stated once:
  * assembly (H, g, bounds) vs oracle:           relative 1e-11 of the matrix' max entry
  * forces vs the oracle's ADMM twin:            <= 2e-3 N when the iteration counts agree within one check interval
                                                 (the two differ only by summation order; an iterate landing within
                                                 rounding of the stopping threshold may stop one check later)
  * forces vs the independent exact QP optimum:  <= 5e-2 N  (2.5e-4 of a nominal 200 N stance force; ADMM stops
                                                 at eps_abs = eps_rel = 1e-6 in the scaled variables)
"""
import os

import numpy as np
import pytest

import srbd_oracle as orc
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TOL_TWIN_N = 2e-3
TOL_EXACT_N = 5e-2


def _engine(N, **kw):
    from g1_locomotion_amd import BatchMPC
    kw.setdefault("rho_restart_iter", -1)       # off unless the test is about it (the default at N > 10 is 100 / 125)
    return BatchMPC(horizon=N, **kw)


@pytest.mark.parametrize("kernel", ["compact", "wave"])
@pytest.mark.parametrize("N,schedule", [(10, "single"), (10, "double"), (10, "mixed"), (8, "single"), (8, "mixed"), (4, "double"), (4, "single"),
                                        (12, "single"), (16, "single"), (20, "single")])
def test_assembly_matches_oracle(torch_first, built_lib, N, schedule, kernel):
    """Rows a5-a8 on the kernels that SHIP: srbdqp_assemble_f64 starts the kernel a solve of the batch would run (4-wave
    compact, or the one-wave batch kernel) in dump mode, right before its factorisation.  The closed-form Hessian and
    gradient of the presolved QP against the oracle's dense products B'QB + R, q = B'Q(A x0 - x_ref), entry by entry."""
    from g1_locomotion_amd import _lib
    B = 6
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=100 + N, schedule=schedule)
    one_wave = kernel == "wave" and (schedule == "single" and N <= 10 or N == 4)     # <= 64 presolved variables, <= 4 x 4 tiles
    with _engine(N, kernel=_lib.KERNEL_WAVE if kernel == "wave" else _lib.KERNEL_COMPACT) as eng:
        got = eng.assemble(x0, xr, ft, ct)
        assert eng.kernel_name().startswith("wave_" if one_wave else "compact_"), eng.kernel_name()
    p = orc.params_for(N)
    for b in range(B):
        qp = orc.build_qp(p, x0[b], xr[b], ft[b], ct[b])
        red, vi, ri = orc.presolve(qp, ct[b])
        sP = np.abs(red["P"]).max()
        assert np.abs(got["P"][b][np.ix_(vi, vi)] - red["P"]).max() <= 1e-11 * sP
        assert np.abs(got["q"][b][vi] - red["q"]).max() <= 1e-11 * max(1.0, np.abs(red["q"]).max())
        off = np.setdiff1d(np.arange(12 * N), vi)
        assert np.all(got["P"][b][off, :] == 0.0) and np.all(got["P"][b][:, off] == 0.0) and np.all(got["q"][b][off] == 0.0)
        np.testing.assert_array_equal(got["l"][b], qp["l"])
        np.testing.assert_array_equal(got["u"][b], qp["u"])


# kernel variants of the presolved family; the general kernel has its own file (test_gpu_wrench.py)
@pytest.mark.parametrize("kernel", ["auto", "split", "wave"])
@pytest.mark.parametrize("N,schedule,B", [(10, "single", 24), (10, "double", 8), (10, "mixed", 16), (8, "mixed", 8), (8, "single", 8), (4, "single", 6), (4, "double", 6)])
def test_solve_matches_oracle_and_exact_optimum(torch_first, built_lib, kernel, N, schedule, B):
    from g1_locomotion_amd import _lib
    kid = {"auto": _lib.KERNEL_AUTO, "split": _lib.KERNEL_SPLIT, "wave": _lib.KERNEL_WAVE}[kernel]
    presolved = True
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=200 + N, schedule=schedule)
    with _engine(N, kernel=kid) as eng:
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        # wave = the whole solve on one wave per QP, split = the same as two kernels with a hand-over through HBM; both
        # exist for <= 64 presolved variables, else fall back to compact
        assert eng.kernel_name().startswith({"auto": ("compact_", "wave_"), "split": ("split_", "compact_"), "wave": ("wave_", "compact_")}[kernel]), eng.kernel_name()
        if kernel == "auto":     # (round 4: AUTO runs <= 64 presolved variables on the one-wave kernel at every batch size, the rest of these small batches on the 4-wave one)
            assert eng.kernel_name().startswith("wave_" if (schedule == "single" or N == 4) else "compact_"), eng.kernel_name()
        if kernel in ("split", "wave") and (schedule == "single" or N == 4):     # <= 64 presolved variables
            assert eng.kernel_name().startswith(kernel + "_")
    p = orc.SrbdParams(eliminate_swing=presolved)
    for b in range(B):
        ref = orc.update(p, x0[b], xr[b], ft[b], ct[b])
        assert out["status"][b] == ref["status"] and ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER)
        solved = ref["status"] == orc.STATUS_SOLVED      # the rare QP that hits the iteration cap is flagged, and looser
        assert abs(int(out["iters"][b]) - ref["iters"]) <= p.check_every, (b, out["iters"][b], ref["iters"])
        assert np.abs(out["u"][b] - ref["u"]).max() <= TOL_TWIN_N
        assert np.abs(out["x"][b] - ref["x"]).max() <= 1e-5
        xs, ys = orc.solve_reference(p, ref["qp"])
        assert np.abs(out["u"][b].reshape(-1) - xs * p.force_scale).max() <= (TOL_EXACT_N if solved else 10 * TOL_EXACT_N)
        # solver-independent acceptance: KKT residuals of the GPU primal/dual pair in the scaled problem
        qp = ref["qp"]
        # (on the presolved problem: duals of the eliminated swing-contact rows are not returned)
        kq = orc.presolve(qp, ct[b])[0] if presolved else qp
        vi = orc.presolve(qp, ct[b])[1] if presolved else np.arange(12 * N)
        ri = orc.presolve(qp, ct[b])[2] if presolved else np.arange(20 * N)
        kr = orc.kkt_residuals(kq["P"], kq["q"], kq["A"], kq["l"], kq["u"], out["u"][b].reshape(-1)[vi] / p.force_scale, out["y"][b][ri])
        assert kr["primal"] <= (1e-4 if solved else 1e-2) and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(qp["q"]).max()), kr
        if presolved:
            off = np.setdiff1d(np.arange(12 * N), vi)
            assert np.all(out["u"][b].reshape(-1)[off] == 0.0)          # swing contacts carry exactly zero force


def test_warm_start_reduces_iterations(torch_first, built_lib):
    N, B = 10, 16
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=321, schedule="single")
    with _engine(N) as eng:
        cold = eng.solve(x0, xr, ft, ct, want_y=True)
        warm = eng.solve(x0, xr, ft, ct, warm_u=cold["u"].reshape(B, -1), warm_y=cold["y"], want_y=True)
    assert (warm["status"] == orc.STATUS_SOLVED).all()
    assert (warm["iters"] <= 10).all() and warm["iters"].mean() < 0.35 * cold["iters"].mean(), (warm["iters"], cold["iters"])
    assert np.abs(warm["u"] - cold["u"]).max() <= TOL_TWIN_N


def test_contact_bound_and_empty_contact_set(torch_first, built_lib):
    """Edge cases of the presolve: a QP with no stance contact at all (all forces 0, state = free fall roll-out) and
    a QP that violates a promised per-step contact bound (reported, not mis-solved)."""
    from g1_locomotion_amd import _lib
    N, B = 10, 4
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=77, schedule="double")
    ct[1] = 0                                   # flight phase over the whole horizon
    with _engine(N) as eng:
        out = eng.solve(x0, xr, ft, ct)
    assert out["status"][1] == orc.STATUS_SOLVED and out["iters"][1] == 0 and np.all(out["u"][1] == 0.0)
    ref = orc.update(orc.SrbdParams(), x0[1], xr[1], ft[1], ct[1])
    assert np.abs(out["x"][1] - ref["x"]).max() <= 1e-9
    for b in (0, 2, 3):
        ref = orc.update(orc.SrbdParams(), x0[b], xr[b], ft[b], ct[b])
        assert np.abs(out["u"][b] - ref["u"]).max() <= TOL_TWIN_N
    with _engine(N, max_contacts_per_step=2) as eng:      # promise single support, feed double support
        out = eng.solve(x0, xr, ft, ct)
    assert (out["status"][[0, 2, 3]] == _lib.CONTACT_BOUND).all() and out["status"][1] == orc.STATUS_SOLVED
    assert np.all(out["u"][[0, 2, 3]] == 0.0)


def test_mpc_update_drop_in_path(torch_first, built_lib):
    """The reference caller's sequence (g1_mujoco_sim/src/run_simulation.py:73-111) through MPC.update(): shapes of
    what comes back, parity with the oracle, and a second control step from the predicted state."""
    from g1_locomotion_amd import mpc
    N = 10
    x0, xr, ft, ct = (a[0] for a in orc.synthetic_batch(1, N, seed=55, schedule="double"))
    with pytest.raises(TypeError):
        mpc.MPC(dt=0.04, warm_start=True)               # removed in round 5 (profiles/r05_warm_start_sweep.txt)
    MPC = mpc.MPC(dt=0.04)
    MPC.init_matrices()
    MPC.x0[:] = x0.reshape(13, 1)
    MPC.x_ref_hor[:] = xr
    c_horizon = [ft[k].copy() for k in range(MPC.HORIZON_LENGTH)]
    contact_horizon = [np.array([1, 1, 1, 1]) for _ in range(MPC.HORIZON_LENGTH)]
    p_com_horizon = MPC.x_ref_hor[:, 3:6].copy()
    u_opt0, x_opt1 = MPC.update(contact_horizon, c_horizon, p_com_horizon, x_current=MPC.x0, one_rollout=True)
    assert u_opt0.flatten().shape == (12,) and x_opt1.shape == (N + 1, 13) and x_opt1[1, 3:6].flatten().shape == (3,)
    ref = orc.update(orc.SrbdParams(), x0, xr, ft, ct, pcom_hor=p_com_horizon)
    assert MPC.status == ref["status"] == orc.STATUS_SOLVED
    assert np.abs(u_opt0.flatten() - ref["u"][0]).max() <= TOL_TWIN_N
    assert np.abs(x_opt1 - ref["x"]).max() <= 1e-5
    # next control step: same scene, state moved to the predicted one
    MPC.x0[:] = x_opt1[1].reshape(13, 1)
    u2, _ = MPC.update(contact_horizon, c_horizon, p_com_horizon, x_current=MPC.x0, one_rollout=False)
    assert MPC.status == orc.STATUS_SOLVED
    ref2 = orc.update(orc.SrbdParams(eps_abs=1e-8, eps_rel=1e-8, max_iter=3000), x_opt1[1], xr, ft, ct, pcom_hor=p_com_horizon)
    assert np.abs(u2.flatten() - ref2["u"][0]).max() <= TOL_EXACT_N
    MPC.close()


def test_ragged_horizons_bucketed_launch(torch_first, built_lib):
    """BASELINE.json configs[4]: mixed horizons N in {8, 12, 16, 24}, per-QP contact schedules of every kind, one C-ABI call
    (srbdqp_solve_ragged_f64: bucket permutation + one launch per horizon bucket, all in flight together); every QP against
    the oracle twin and the exact optimum, in the caller's order."""
    from g1_locomotion_amd import RaggedMPC
    rng = np.random.default_rng(5)
    problems = []
    for i in range(40):
        N = int(rng.choice([8, 12, 16, 24]))
        x0, xr, ft, ct = (a[0] for a in orc.synthetic_batch(1, N, seed=900 + i, schedule=str(rng.choice(["single", "mixed", "double"]))))
        problems.append(dict(x0=x0, x_ref=xr, foot=ft, contact=ct))
    eng = RaggedMPC(horizons=(8, 12, 16, 24), rho_restart_iter=-1)
    res = eng.solve(problems)
    res2 = eng.solve(problems[::-1])[::-1]            # another order, other buckets sizes per position: same answers
    eng.close()
    for pr, r, r2 in zip(problems, res, res2):
        p = orc.params_for(pr["x_ref"].shape[0])
        ref = orc.update(p, pr["x0"], pr["x_ref"], pr["foot"], pr["contact"])
        assert r["status"] == ref["status"] and abs(r["iters"] - ref["iters"]) <= p.check_every
        assert r["u"].shape == pr["foot"].shape and np.abs(r["u"] - ref["u"]).max() <= TOL_TWIN_N
        assert r["x"].shape == (pr["foot"].shape[0] + 1, 13) and np.abs(r["x"] - ref["x"]).max() <= 1e-5
        np.testing.assert_array_equal(r["u"], r2["u"])
        if ref["status"] == orc.STATUS_SOLVED:
            xs, _ = orc.solve_reference(p, ref["qp"])
            assert np.abs(r["u"].reshape(-1) - xs * p.force_scale).max() <= TOL_EXACT_N


def test_ragged_device_call_does_not_block_and_buckets_overlap(torch_first, built_lib):
    """The device-buffer ragged entry returns before the work is done (the caller's stream waits through events) and a
    second call may follow at once; results equal the per-horizon engines' on the same QPs."""
    torch = torch_first
    from g1_locomotion_amd import RaggedMPC, BatchMPC, _lib
    rng = np.random.default_rng(11)
    hz = (8, 12, 16, 24)
    Bq = 600
    Nq = rng.choice(hz, Bq).astype(np.int32)
    parts = [[a[0] for a in orc.synthetic_batch(1, int(N), seed=7000 + i, schedule="mixed")] for i, N in enumerate(Nq)]
    x0 = np.stack([p[0] for p in parts]); xr = np.concatenate([p[1] for p in parts]); ft = np.concatenate([p[2] for p in parts]); ct = np.concatenate([p[3] for p in parts])
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(v).to(dev) for v in (x0, xr, ft, ct)]
    rows = int(Nq.sum())
    u = torch.zeros((rows, 12), dtype=torch.float64, device=dev); st = torch.zeros(Bq, dtype=torch.int32, device=dev); it = torch.zeros(Bq, dtype=torch.int32, device=dev)
    eng = RaggedMPC(horizons=hz, rho_restart_iter=-1)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        for _ in range(2):                              # back to back, nothing waited for in between
            eng.solve_device(Bq, Nq, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), status=st.data_ptr(),
                             iters=it.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    eng.close()
    u, st, it = u.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(Nq)])
    for N in hz:
        idx = np.where(Nq == N)[0]
        with BatchMPC(horizon=int(N), kernel=_lib.KERNEL_WRENCH, rho_restart_iter=-1) as one:
            ref = one.solve(x0[idx], np.stack([xr[off[i]:off[i + 1]] for i in idx]), np.stack([ft[off[i]:off[i + 1]] for i in idx]),
                            np.stack([ct[off[i]:off[i + 1]] for i in idx]))
        np.testing.assert_array_equal(st[idx], ref["status"])
        np.testing.assert_array_equal(it[idx], ref["iters"])
        for j, i in enumerate(idx):
            np.testing.assert_array_equal(u[off[i]:off[i + 1]], ref["u"][j])


def test_schedule_hint_only_reorders_work(torch_first, built_lib):
    """Longest-first dispatch from the previous step's iteration counts: bit-identical results in the caller's order."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC
    N, B = 10, 300
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=31, schedule="single")
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(v).to(dev) for v in (x0, xr, ft, ct)]
    outs = []
    with BatchMPC(horizon=N, max_contacts_per_step=2) as eng:
        it_prev = None
        for rep in range(3):
            u = torch.zeros((B, N, 12), dtype=torch.float64, device=dev)
            it = torch.zeros(B, dtype=torch.int32, device=dev)
            st = torch.zeros(B, dtype=torch.int32, device=dev)
            eng.set_schedule_hint(it_prev.data_ptr() if it_prev is not None else 0, B)
            eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(),
                             status=st.data_ptr(), iters=it.data_ptr())
            eng.synchronize()
            outs.append((u.cpu().numpy(), it.cpu().numpy(), st.cpu().numpy()))
            it_prev = it if rep == 0 else (it_prev.flip(0).contiguous())      # second round: a deliberately wrong hint
    for u, it, st in outs[1:]:
        np.testing.assert_array_equal(u, outs[0][0])
        np.testing.assert_array_equal(it, outs[0][1])
        np.testing.assert_array_equal(st, outs[0][2])


@pytest.mark.parametrize("N,pattern,B", [(10, "single", 2048), (10, "mixed", 1024), (10, "random", 1024), (8, "random", 512), (8, "single", 1024), (4, "random", 1024), (16, "single", 256)])
def test_large_batch_against_c_oracle(torch_first, built_lib, N, pattern, B):
    """Statistical parity at scale against the compiled oracle: every QP of a large seeded batch, including arbitrary
    per-point contact patterns (steps with 0, 1 or 3 stance points, whole-horizon flight)."""
    import c_oracle
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=4000 + N, schedule="single" if pattern == "random" else pattern)
    if pattern == "random":
        rng = np.random.default_rng(17)
        ct = (rng.random(ct.shape) < 0.6).astype(np.uint8)
        ct[0] = 0; ct[1] = 1; ct[2, :, 1:] = 0            # flight, full double support, a single heel point
    p = orc.params_for(N)
    ref = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=8)
    with _engine(N) as eng:
        out = eng.solve(x0, xr, ft, ct)
        # AUTO: the one-wave kernel (<= 2 stance contacts per step), the general kernel (more, batches >= 768) or compact
        assert eng.kernel_name().startswith(("compact_", "wave_", "wrench_"))
    np.testing.assert_array_equal(out["status"], ref["status"])
    assert np.abs(out["iters"].astype(int) - ref["iters"].astype(int)).max() <= p.check_every
    same = out["iters"] == ref["iters"]
    assert same.mean() > 0.97
    err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
    assert err[same].max() <= 1e-4 and err.max() <= TOL_TWIN_N, (err[same].max(), err.max())
    assert np.abs(out["x"] - ref["x"]).max() <= 1e-5
    assert np.all(out["u"].reshape(B, N, 4, 3)[ct == 0] == 0.0)


@pytest.mark.parametrize("restart", [False, True])
def test_full_size_batch_properties(torch_first, built_lib, restart):
    """BASELINE.json's full per-GPU size (configs[3]: 65,536 QPs per GPU, N=10) through size-independent properties:
    feasibility of every returned force, exact zeros on swing contacts, bitwise permutation invariance of the batch,
    idempotence under a warm start from the own solution, and oracle parity on a seeded subset.  With fixed rho (restart off) and as the engine runs the
    batch by default (rho re-balanced in place by the one-wave kernel: 99.9 % solved)."""
    import c_oracle
    from g1_locomotion_amd import BatchMPC
    N, B = 10, 65536
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=4242, schedule="single")
    r_iter, r_count = orc.default_restart(N, one_wave=True) if restart else (0, 1)
    p = orc.params_for(N, rho_restart_iter=r_iter, rho_restart_count=r_count)
    with (BatchMPC(horizon=N, max_contacts_per_step=2) if restart else _engine(N)) as eng:
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        perm = np.random.default_rng(3).permutation(B)
        out_p = eng.solve(x0[perm], xr[perm], ft[perm], ct[perm])
        warm = eng.solve(x0, xr, ft, ct, warm_u=out["u"].reshape(B, -1), warm_y=out["y"])
    st, it = out["status"], out["iters"]
    assert set(np.unique(st)) <= {orc.STATUS_SOLVED, orc.STATUS_MAX_ITER} and (st == orc.STATUS_SOLVED).mean() > (0.999 if restart else 0.99)
    f = out["u"].reshape(B, N, 4, 3)
    on = ct != 0
    assert np.all(f[~on] == 0.0)
    solved = (st == orc.STATUS_SOLVED)[:, None, None] & on
    tol = 5e-3                                                   # N; ADMM's primal residual at eps 1e-6 is far below
    assert np.all(np.abs(f[..., 0])[solved] <= p.mu * f[..., 2][solved] + tol)
    assert np.all(np.abs(f[..., 1])[solved] <= p.mu * f[..., 2][solved] + tol)
    assert f[..., 2][solved].min() >= p.fz_min - tol and f[..., 2][solved].max() <= p.fz_max + tol
    # a batch is a set: permuting the QPs permutes the results bit for bit
    np.testing.assert_array_equal(out_p["u"], out["u"][perm])
    np.testing.assert_array_equal(out_p["iters"], it[perm])
    np.testing.assert_array_equal(out_p["x"], out["x"][perm])
    # restarting a solved QP from its own primal/dual solution stops at the first check with the same forces
    ok = st == orc.STATUS_SOLVED
    if restart:   # (a QP that re-balanced converged under ANOTHER rho: from its own (x, y) under the first one it may need a few checks more)
        first = ok & (it <= r_iter)
        assert (warm["iters"][first] == p.check_every).mean() > 0.999 and (warm["iters"][ok] == p.check_every).mean() > 0.95
        assert (warm["status"][ok] == orc.STATUS_SOLVED).mean() > 0.9995
    else:
        assert (warm["iters"][ok] == p.check_every).mean() > 0.999
    same_rho = ok & (it <= r_iter) if restart else ok
    assert np.abs(warm["u"][same_rho] - out["u"][same_rho]).max() < 5e-3     # (five more iterations move the forces by no more than the stopping rule leaves to the optimum)
    assert np.abs(warm["u"][ok] - out["u"][ok]).max() < 3 * TOL_EXACT_N     # (... a re-balanced QP by no more than ITS stopping point is from the optimum)
    # seeded subset against the compiled oracle
    idx = np.random.default_rng(4).choice(B, 512, replace=False)
    ref = c_oracle.solve_batch(p, x0[idx], xr[idx], ft[idx], ct[idx], nthreads=8)
    np.testing.assert_array_equal(st[idx], ref["status"])
    assert np.abs(it[idx].astype(int) - ref["iters"].astype(int)).max() <= p.check_every
    assert np.abs(out["u"][idx] - ref["u"]).max() <= TOL_TWIN_N


def test_two_streams_pipeline_distinct_batches_through_one_handle(torch_first, built_lib):
    """What bench.py does, with DIFFERENT batches in flight: consecutive solves of one handle alternate over two HIP
    streams without synchronising in between (split pipeline + dispatch hint: per-stream hand-over workspace and
    dispatch order).  Every result must equal, bit for bit, the result of the same batch solved alone."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC
    N, B = 10, 1024
    dev = torch.device("cuda", 0)
    batches = [[torch.from_numpy(v).to(dev) for v in orc.synthetic_batch(B, N, seed=700 + i, schedule="single")] for i in range(4)]
    from g1_locomotion_amd import _lib
    with BatchMPC(horizon=N, max_contacts_per_step=2, kernel=_lib.KERNEL_SPLIT) as eng:
        def solve(d, stream=0, hint=None):
            u = torch.zeros((B, N, 12), dtype=torch.float64, device=dev)
            it = torch.zeros(B, dtype=torch.int32, device=dev)
            st = torch.zeros(B, dtype=torch.int32, device=dev)
            eng.set_schedule_hint(hint.data_ptr() if hint is not None else 0, B)
            eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(),
                             status=st.data_ptr(), iters=it.data_ptr(), stream=stream)
            return u, it, st
        alone = []
        for d in batches:
            r = solve(d)
            eng.synchronize()
            alone.append([t.clone() for t in r])
        assert eng.kernel_name().startswith("split_")
        streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        torch.cuda.synchronize(dev)
        outs = []
        for rep in range(3):
            for i, d in enumerate(batches):
                s = streams[i % 2]
                with torch.cuda.stream(s):
                    outs.append((i, solve(d, stream=s.cuda_stream, hint=alone[i][1])))
        torch.cuda.synchronize(dev)
        eng.set_schedule_hint(0)
    for i, (u, it, st) in outs:
        assert torch.equal(u, alone[i][0]) and torch.equal(it, alone[i][1]) and torch.equal(st, alone[i][2]), i


@pytest.mark.parametrize("kernel", ["compact", "split", "wave"])
def test_rho_restart_matches_the_oracle(torch_first, built_lib, kernel):
    """rho_restart_iter = 100: QPs that reach the cap of the first pass are re-factored with the re-balanced rho and
    continue from their own (x, y).  Same rule in the oracle (solve_with_restart / srbd_oracle.c), so statuses and
    iteration counts agree, nearly every QP ends solved, and the forces stay within the exact-optimum tolerance."""
    import c_oracle
    from g1_locomotion_amd import _lib
    N, B = 10, 2048
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=1000, schedule="single")
    p = orc.SrbdParams(rho_restart_iter=100)
    ref = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=8)
    assert (ref["iters"] > 100).sum() >= 20 and (ref["status"] == orc.STATUS_SOLVED).mean() > 0.997
    kid = {"compact": _lib.KERNEL_COMPACT, "split": _lib.KERNEL_SPLIT, "wave": _lib.KERNEL_WAVE}[kernel]
    with _engine(N, kernel=kid, rho_restart_iter=100) as eng:
        out = eng.solve(x0, xr, ft, ct)
        assert eng.kernel_name().startswith(kernel + "_")
    np.testing.assert_array_equal(out["status"], ref["status"])
    assert np.abs(out["iters"].astype(int) - ref["iters"].astype(int)).max() <= p.check_every
    same = out["iters"] == ref["iters"]
    assert same.mean() > 0.97
    err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
    assert err[same].max() <= 1e-3 and err.max() <= 2 * TOL_TWIN_N, (err[same].max(), err.max())
    # the restarted QPs against the exact optimum (rho' is clipped to [rho/10, 5 rho] for exactly this)
    for b in np.where((ref["iters"] > 100) & (ref["status"] == orc.STATUS_SOLVED))[0][:12]:
        xs, _ = orc.solve_reference(p, orc.build_qp(p, x0[b], xr[b], ft[b], ct[b]))
        assert np.abs(out["u"][b].reshape(-1) - xs * p.force_scale).max() <= TOL_EXACT_N


@pytest.mark.parametrize("N,every,count,schedule", [(10, 0, 0, "single"), (10, 40, 4, "single"), (8, 0, 0, "single"), (4, 50, 2, "single"),
                                                    (4, 25, 3, "double")])     # (the last: 4 contacts per step, EVERY QP past the first mark)
def test_one_wave_kernel_restarts_in_place(torch_first, built_lib, N, every, count, schedule):
    """The one-wave kernel re-balances rho IN PLACE (srbdqp_setup1.hpp RST): every rho_restart_iter iterations, up to rho_restart_count times, each time
    from the rho of the pass that ended, inside the same cap on the total.  By default (0, 0 -> 55, 2) wherever that kernel runs the solve: 99.3 % -> 99.9 % of the
    configs[1] QPs solved.  Same rule in both oracles; the restarted QPs end within the exact-optimum tolerance."""
    import c_oracle
    from g1_locomotion_amd import BatchMPC
    B = 4096
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=1000, schedule=schedule)
    p = orc.params_for(N, rho_restart_iter=every or 55, rho_restart_count=min(count or 2, 3))      # (srbdqp_config.rho_restart_count: values above 3 mean 3)
    ref = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=8)
    plain = c_oracle.solve_batch(orc.params_for(N), x0, xr, ft, ct, nthreads=8)
    kw = {} if every == 0 else dict(rho_restart_iter=every, rho_restart_count=count)
    from g1_locomotion_amd import _lib
    if schedule != "single":   # (4 contacts per step: AUTO sends batches of this size to the general kernel)
        kw.update(kernel=_lib.KERNEL_WAVE, max_contacts_per_step=4)
    else:
        kw.update(max_contacts_per_step=2)
    with BatchMPC(horizon=N, **kw) as eng:
        out = eng.solve(x0, xr, ft, ct)
        assert eng.kernel_name().startswith("wave_"), eng.kernel_name()
    solved = (out["status"] == orc.STATUS_SOLVED).mean()
    assert solved >= 0.999 and solved >= (plain["status"] == orc.STATUS_SOLVED).mean()
    assert out["iters"].mean() <= plain["iters"].mean() + 0.05
    np.testing.assert_array_equal(out["status"], ref["status"])
    assert np.abs(out["iters"].astype(int) - ref["iters"].astype(int)).max() <= p.check_every
    same = out["iters"] == ref["iters"]
    assert same.mean() > 0.97
    err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
    assert err[same].max() <= 1e-3 and err.max() <= 2 * TOL_TWIN_N, (err[same].max(), err.max())
    mark = p.rho_restart_iter
    twice = np.where((ref["iters"] > 2 * mark) & (ref["status"] == orc.STATUS_SOLVED))[0]
    once = np.where((ref["iters"] > mark) & (ref["iters"] <= 2 * mark) & (ref["status"] == orc.STATUS_SOLVED))[0]
    if N == 10:
        assert len(twice) >= 4 and len(once) >= 12
    for b in list(twice[:8]) + list(once[:8]):
        xs, _ = orc.solve_reference(p, orc.build_qp(p, x0[b], xr[b], ft[b], ct[b]))
        # (a QP that re-balanced more than once stops further from the optimum on the same residual test: the C oracle's worst of 4096 is 0.087 N after three)
        tol = TOL_EXACT_N if ref["iters"][b] <= 2 * mark else 3 * TOL_EXACT_N
        assert np.abs(out["u"][b].reshape(-1) - xs * p.force_scale).max() <= tol, b
        o = orc.update(p, x0[b], xr[b], ft[b], ct[b])                  # the numpy oracle runs the same passes
        assert o["status"] == out["status"][b] and abs(o["iters"] - int(out["iters"][b])) <= p.check_every


def test_restart_in_place_from_a_warm_start(torch_first, built_lib):
    """The first pass of the restart kernel starts from the caller's (u, y), the continued ones from their own: every QP warm-started from the solution of its
    NEIGHBOUR in the batch (a poor guess: some stay past the marks), against the numpy oracle run the same way."""
    from g1_locomotion_amd import BatchMPC
    N, B = 10, 1024
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=77, schedule="single")
    r_iter, r_count = orc.default_restart(N, one_wave=True)
    p = orc.params_for(N, rho_restart_iter=r_iter, rho_restart_count=r_count)
    with BatchMPC(horizon=N, max_contacts_per_step=2, rho_restart_iter=r_iter, rho_restart_count=r_count) as eng:   # (explicit: automatic from 4096 QPs per call)
        first = eng.solve(x0, xr, ft, ct, want_y=True)
        wu, wy = np.roll(first["u"].reshape(B, -1), 1, axis=0), np.roll(first["y"], 1, axis=0)
        out = eng.solve(x0, xr, ft, ct, warm_u=wu, warm_y=wy)
        assert eng.kernel_name().startswith("wave_"), eng.kernel_name()
    assert (out["status"] == orc.STATUS_SOLVED).mean() > 0.995
    slow = np.where(out["iters"] > r_iter)[0]
    assert len(slow) >= 3
    for b in list(slow[:6]) + list(np.where(out["iters"] <= r_iter)[0][:4]):
        o = orc.update(p, x0[b], xr[b], ft[b], ct[b], warm=(wu[b] / p.force_scale, wy[b]))
        assert o["status"] == out["status"][b] and abs(o["iters"] - int(out["iters"][b])) <= p.check_every, (b, o["iters"], out["iters"][b])
        if o["iters"] == out["iters"][b]:
            assert np.abs(o["u"] - out["u"][b]).max() <= 1e-3, b


def test_rho_restart_on_the_staged_batch1_path(torch_first, built_lib):
    """MPC.update() (staged, fused kernel): the second pass is started by the host only when a status asks for it."""
    from g1_locomotion_amd import mpc
    N = 10
    x0, xr, ft, ct = orc.synthetic_batch(400, N, seed=1000, schedule="single")
    p = orc.SrbdParams(rho_restart_iter=100)
    refs = [orc.update(p, x0[b], xr[b], ft[b], ct[b]) for b in range(400)]
    hard = [b for b in range(400) if refs[b]["iters"] > 100][:4]
    easy = [b for b in range(400) if refs[b]["iters"] <= 40][:2]
    assert len(hard) >= 2
    MPC = mpc.MPC(dt=0.04, rho_restart_iter=100)
    MPC.init_matrices()
    for b in hard + easy + hard:
        MPC.x_ref_hor[:] = xr[b]
        u0, xo = MPC.update(list(ct[b]), list(ft[b]), xr[b][:, 3:6], x_current=x0[b].reshape(13, 1), one_rollout=True)
        assert MPC.status == refs[b]["status"] and abs(MPC.iters - refs[b]["iters"]) <= p.check_every, (b, MPC.iters, refs[b]["iters"])
        assert np.abs(MPC.u_opt - refs[b]["u"]).max() <= 2 * TOL_TWIN_N
    MPC.close()


def test_ragged_call_runs_the_automatic_rho_restart_of_its_long_buckets(torch_first, built_lib):
    """Default rho_restart_iter on a ragged object: the N > 10 buckets take the same two passes as a homogeneous batch of that
    horizon (the per-horizon automatic rule, later passes selected in-kernel; the N = 8 bucket its 55 x 2 too): statuses, iteration
    counts and forces equal the per-horizon engines' bit for bit, and some QPs of the case do restart."""
    from g1_locomotion_amd import RaggedMPC, BatchMPC, _lib
    rng = np.random.default_rng(23)
    hz = (8, 16, 24)
    Bq = 300
    Nq = rng.choice(hz, Bq).astype(np.int32)
    parts = [[a[0] for a in orc.synthetic_batch(1, int(N), seed=8000 + i, schedule="single" if i % 2 else "mixed")] for i, N in enumerate(Nq)]
    x0 = np.stack([p[0] for p in parts]); xr = np.concatenate([p[1] for p in parts]); ft = np.concatenate([p[2] for p in parts]); ct = np.concatenate([p[3] for p in parts])
    eng = RaggedMPC(horizons=hz)
    out = eng.solve_packed(Nq, x0, xr, ft, ct)
    eng.close()
    off = out["off"]
    restarted = 0
    for N in hz:
        idx = np.where(Nq == N)[0]
        with BatchMPC(horizon=int(N), kernel=_lib.KERNEL_WRENCH) as one:
            ref = one.solve(x0[idx], np.stack([xr[off[i]:off[i + 1]] for i in idx]), np.stack([ft[off[i]:off[i + 1]] for i in idx]),
                            np.stack([ct[off[i]:off[i + 1]] for i in idx]))
        np.testing.assert_array_equal(out["status"][idx], ref["status"])
        np.testing.assert_array_equal(out["iters"][idx], ref["iters"])
        for j, i in enumerate(idx):
            np.testing.assert_array_equal(out["u"][off[i]:off[i + 1]], ref["u"][j])
        if N > 10:
            restarted += int((ref["iters"] > orc.default_restart(int(N))[0]).sum())
    assert restarted >= 3, restarted


@pytest.mark.parametrize("N,schedule", [(10, "single"), (8, "single"), (4, "double")])
def test_two_phase_call_equals_the_one_shot_call(torch_first, built_lib, N, schedule):
    """srbdqp_prepare_staged_f64 + srbdqp_solve_prepared_f64: the set-up runs from a WRONG predicted state, the second phase
    patches the gradient (q is affine in x0: q_pred + dq/dx0 (x0 - x0_pred)) and rolls out from the measured state.  Against
    the one-shot call on the same inputs (split pipeline: same iterates): statuses and iteration counts equal, forces and
    predicted states to 1e-8 (the patched gradient is summed in another order); and against the oracle twin."""
    from g1_locomotion_amd import BatchMPC
    B = 8
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=600 + N, schedule=schedule)
    rng = np.random.default_rng(N)
    with BatchMPC(horizon=N, rho_restart_iter=-1) as eng:
        ref = eng.solve(x0, xr, ft, ct)
        st = eng.stage()
        assert st["capacity"] >= B
        st["x_ref"][:B] = xr; st["foot"][:B] = ft.reshape(B, N, 12); st["contact"][:B] = ct.reshape(B, N, 4)
        st["x0"][:B] = x0 + rng.normal(size=x0.shape) * np.array([0.2] * 3 + [0.05] * 3 + [0.5] * 6 + [0.0])     # the prediction: off
        eng.prepare_staged(B)
        assert eng.kernel_name().startswith("prepare_f64_n")
        st["x0"][:B] = x0                                                                                          # the measurement
        eng.solve_prepared(B, want_x=True)
        assert eng.kernel_name().startswith("prepared_f64_n")
        u, x, status, iters = st["u"][:B].copy(), st["x"][:B].copy(), st["status"][:B].copy(), st["iters"][:B].copy()
        with pytest.raises(Exception):
            eng.solve_prepared(B)                     # nothing pending any more
    np.testing.assert_array_equal(status, ref["status"])
    assert np.abs(iters - ref["iters"]).max() <= 5, (iters, ref["iters"])
    assert np.abs(u - ref["u"]).max() <= 1e-6 and np.abs(x - ref["x"]).max() <= 1e-8
    p = orc.params_for(N)
    for b in range(B):
        o = orc.update(p, x0[b], xr[b], ft[b], ct[b])
        assert status[b] == o["status"] and np.abs(u[b] - o["u"]).max() <= TOL_TWIN_N


@pytest.mark.parametrize("N,schedule,suffix", [(10, "single", "compact_f64_n10_s2_lat"), (8, "single", "compact_f64_n8_s2_lat"), (4, "single", "compact_f64_n4_s2_lat"),
                                               (10, "double", "wrench_f64_n10_lat"), (10, "mixed", "wrench_f64_n10_lat"), (8, "double", "wrench_f64_n8_lat")])
def test_staged_batch1_low_latency_instantiations(torch_first, built_lib, N, schedule, suffix):
    """The staged call (what MPC.update() uses) one QP at a time: <= 2 stance contacts per step run the 4-wave set-up + one-wave iteration kernel, anything
    else the low-latency instantiation of the general kernel (the reference's own call pattern is full double support, run_simulation.py:100-101).  Each QP
    against the oracle twin (status, iterations, forces, predicted states) and against the batch kernels on the same inputs; SRBDQP_FLAG_NO_LAT switches both
    instantiations off."""
    from g1_locomotion_amd import BatchMPC, _lib
    B = 12
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=4200 + N, schedule=schedule)
    p = orc.params_for(N)
    with BatchMPC(horizon=N, rho_restart_iter=-1) as eng, BatchMPC(horizon=N, rho_restart_iter=-1, flags=_lib.FLAG_NO_LAT) as plain:
        batch = eng.solve(x0, xr, ft, ct)
        st, st2 = eng.stage(), plain.stage()
        for b in range(B):
            for s_ in (st, st2):
                s_["x0"][0] = x0[b]; s_["x_ref"][0] = xr[b]; s_["foot"][0] = ft[b].reshape(N, 12); s_["contact"][0] = ct[b].reshape(N, 4)
            eng.solve_staged(1, want_x=True)
            plain.solve_staged(1, want_x=True)
            assert eng.kernel_name() == suffix, eng.kernel_name()
            assert not plain.kernel_name().endswith("_lat"), plain.kernel_name()
            o = orc.update(p, x0[b], xr[b], ft[b], ct[b])
            assert int(st["status"][0]) == o["status"] == int(st2["status"][0]) == int(batch["status"][b])
            assert abs(int(st["iters"][0]) - o["iters"]) <= p.check_every and abs(int(st2["iters"][0]) - o["iters"]) <= p.check_every
            assert np.abs(st["u"][0] - o["u"]).max() <= TOL_TWIN_N and np.abs(st["x"][0] - o["x"]).max() <= 1e-4
            assert np.abs(st["u"][0] - st2["u"][0]).max() <= TOL_TWIN_N and np.abs(st["u"][0] - batch["u"][b]).max() <= TOL_TWIN_N
            assert (st["u"][0].reshape(N, 4, 3)[ct[b].reshape(N, 4) == 0] == 0.0).all()           # swing contacts: exactly zero


def test_two_phase_call_limits_and_pcom(torch_first, built_lib):
    """Outside its instantiations (more than 64 presolved variables) the two-phase call refuses loudly; with a CoM horizon
    (use_pcom) it still equals the one-shot call."""
    from g1_locomotion_amd import BatchMPC, SrbdqpError
    with BatchMPC(horizon=12) as eng:
        st = eng.stage()
        x0, xr, ft, ct = orc.synthetic_batch(1, 12, seed=3, schedule="single")
        st["x0"][0] = x0[0]; st["x_ref"][0] = xr[0]; st["foot"][0] = ft[0].reshape(12, 12); st["contact"][0] = ct[0].reshape(12, 4)
        with pytest.raises(SrbdqpError):
            eng.prepare_staged(1)
    N, B = 10, 4
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=91, schedule="single")
    pc = xr[:, :, 3:6] + 0.01
    with BatchMPC(horizon=N, rho_restart_iter=-1) as eng:
        ref = eng.solve(x0, xr, ft, ct, pcom=pc)
        st = eng.stage()
        st["x_ref"][:B] = xr; st["foot"][:B] = ft.reshape(B, N, 12); st["contact"][:B] = ct.reshape(B, N, 4); st["pcom"][:B] = pc
        st["x0"][:B] = 0.5 * x0
        eng.prepare_staged(B, use_pcom=True)
        st["x0"][:B] = x0
        eng.solve_prepared(B)
        np.testing.assert_array_equal(st["status"][:B], ref["status"])
        assert np.abs(st["u"][:B] - ref["u"]).max() <= 1e-6


def test_mpc_prepare_then_update_prepared(torch_first, built_lib):
    """The drop-in object's two-phase form: prepare(...) from the previous state, update_prepared(x) = update(..., x)."""
    from g1_locomotion_amd import mpc
    N = 10
    x0, xr, ft, ct = (a[0] for a in orc.synthetic_batch(1, N, seed=77, schedule="single"))
    M = mpc.MPC(dt=0.04)
    M.init_matrices()
    M.x_ref_hor[:] = xr
    u_a, x_a = M.update(list(ct), list(ft), xr[:, 3:6], x_current=x0.reshape(13, 1))
    M.prepare(list(ct), list(ft), xr[:, 3:6], x_predicted=x0 * 0.9)
    u_b, x_b = M.update_prepared(x0.reshape(13, 1))
    assert M.status == orc.STATUS_SOLVED
    assert np.abs(u_a - u_b).max() <= 1e-6 and np.abs(x_a - x_b).max() <= 1e-8
    M.close()


def test_wave_kernel_with_ragged_contact_counts(torch_first, built_lib):
    """The one-wave kernel with fewer stance contacts than its template bound: single-support schedules with contacts
    dropped at random (0, 1 or 2 stance points per step, so n_eff varies from QP to QP and the tiles are padded)."""
    import c_oracle
    from g1_locomotion_amd import _lib
    N, B = 10, 1024
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=4300, schedule="single")
    rng = np.random.default_rng(23)
    ct = (ct.astype(bool) & (rng.random(ct.shape) < 0.8)).astype(np.uint8)
    ct[0] = 0                                                       # flight
    ct[1, 1:] = 0                                                   # contact only in the first step
    p = orc.SrbdParams()
    ref = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=8)
    ct_bad = ct.copy()
    ct_bad[2] = 1                                                   # double support under a promise of <= 2 contacts per step
    for kid, name in ((_lib.KERNEL_WAVE, "wave_"), (_lib.KERNEL_SPLIT, "split_")):
        with _engine(N, kernel=kid, max_contacts_per_step=2) as eng:
            out = eng.solve(x0, xr, ft, ct)
            assert eng.kernel_name().startswith(name)
            bad = eng.solve(x0, xr, ft, ct_bad)
        assert bad["status"][2] == _lib.CONTACT_BOUND and np.all(bad["u"][2] == 0.0) and bad["iters"][2] == 0
        keep = np.arange(B) != 2
        np.testing.assert_array_equal(bad["status"][keep], out["status"][keep])
        np.testing.assert_array_equal(bad["u"][keep], out["u"][keep])
        np.testing.assert_array_equal(out["status"], ref["status"])
        assert np.abs(out["iters"].astype(int) - ref["iters"].astype(int)).max() <= p.check_every
        same = out["iters"] == ref["iters"]
        assert same.mean() > 0.97
        err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
        assert err[same].max() <= 1e-4 and err.max() <= TOL_TWIN_N, (err[same].max(), err.max())
        assert np.abs(out["x"] - ref["x"]).max() <= 1e-5
        assert np.all(out["u"].reshape(B, N, 4, 3)[ct == 0] == 0.0)


def test_non_finite_input_is_reported_not_propagated(torch_first, built_lib):
    """A NaN in one QP's inputs (here a foot position) must come back as SRBDQP_NUMERICAL for that QP only -- on the
    one-wave batch kernel and on the 4-wave kernel."""
    from g1_locomotion_amd import _lib
    N, B = 10, 600
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=4400, schedule="single")
    ft_bad = ft.copy()
    ft_bad[7, 3, 3 * int(np.argmax(ct[7, 3])) + 1] = np.nan              # a STANCE contact's position (swing ones are not used)
    for kid in (_lib.KERNEL_AUTO, _lib.KERNEL_COMPACT):
        with _engine(N, kernel=kid, max_contacts_per_step=2) as eng:
            good = eng.solve(x0, xr, ft, ct)
            bad = eng.solve(x0, xr, ft_bad, ct)
        assert bad["status"][7] == _lib.NUMERICAL, bad["status"][7]
        keep = np.arange(B) != 7
        np.testing.assert_array_equal(bad["status"][keep], good["status"][keep])
        np.testing.assert_array_equal(bad["u"][keep], good["u"][keep])
        assert np.all(np.isfinite(bad["u"][keep])) and np.all(bad["u"][7] == 0.0)


def test_explicit_com_horizon_on_the_batch_kernel(torch_first, built_lib):
    """p_com_horizon given explicitly (run_simulation.py:103) instead of taken from x_ref: the lever arms change, on the
    one-wave kernel and on the 4-wave kernel alike."""
    import c_oracle
    from g1_locomotion_amd import _lib
    N, B = 10, 600
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=4500, schedule="single")
    pc = xr[:, :, 3:6] + np.random.default_rng(31).uniform(-0.03, 0.03, (B, N, 3))
    p = orc.SrbdParams()
    ref = c_oracle.solve_batch(p, x0, xr, ft, ct, pcom=pc, nthreads=8)
    ref0 = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=8)
    assert np.abs(ref["u"] - ref0["u"]).max() > 1.0                 # the explicit CoM horizon matters
    for kid in (_lib.KERNEL_AUTO, _lib.KERNEL_COMPACT):
        with _engine(N, kernel=kid, max_contacts_per_step=2) as eng:
            out = eng.solve(x0, xr, ft, ct, pcom=pc)
        np.testing.assert_array_equal(out["status"], ref["status"])
        assert np.abs(out["iters"].astype(int) - ref["iters"].astype(int)).max() <= p.check_every
        assert np.abs(out["u"] - ref["u"]).max() <= TOL_TWIN_N and np.abs(out["x"] - ref["x"]).max() <= 1e-5


def test_non_default_constants_reach_every_kernel(torch_first, built_lib):
    """No constant of the problem is baked into a kernel: a different dt, mass, inertia, friction, force bounds, weights,
    scaling and ADMM parameters -- against the oracle with the same values, on the one-wave and the 4-wave kernel."""
    import c_oracle
    from g1_locomotion_amd import _lib
    N, B = 10, 600
    kw = dict(dt=0.03, mass=41.0, inertia=(0.11, 0.09, 0.006), mu=0.55, fz_min=5.0, fz_max=420.0,
              q_diag=(250.0, 320.0, 120.0, 380.0, 410.0, 700.0, 2.0, 1.5, 1.0, 15.0, 25.0, 30.0, 0.0), r_diag=3.0e-4,
              force_scale=60.0, rho=0.8, alpha=1.5, sigma=2.0e-6, eps_abs=2.0e-6, eps_rel=2.0e-6, max_iter=180, check_every=4)
    p = orc.SrbdParams(**kw)
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=4600, schedule="single", dt=kw["dt"])
    ref = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=8)
    for kid in (_lib.KERNEL_AUTO, _lib.KERNEL_COMPACT):
        with _engine(N, kernel=kid, max_contacts_per_step=2, **kw) as eng:
            out = eng.solve(x0, xr, ft, ct)
        np.testing.assert_array_equal(out["status"], ref["status"])
        assert np.abs(out["iters"].astype(int) - ref["iters"].astype(int)).max() <= p.check_every
        same = out["iters"] == ref["iters"]
        assert same.mean() > 0.95
        err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
        assert err[same].max() <= 1e-3 and err.max() <= 5 * TOL_TWIN_N, (err[same].max(), err.max())
        assert np.abs(out["x"] - ref["x"]).max() <= 1e-4


def test_empty_batch_and_null_optional_outputs(torch_first, built_lib):
    """B = 0 is a no-op; status / iters / x / y are optional on the device API (null pointers), also with the rho
    restart, which needs statuses internally."""
    torch = torch_first
    N = 10
    with _engine(N) as eng:
        out = eng.solve(np.zeros((0, 13)), np.zeros((0, N, 13)), np.zeros((0, N, 12)), np.zeros((0, N, 4), np.uint8))
        assert out["u"].shape == (0, N, 12) and out["status"].shape == (0,)
    B = 700
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=4700, schedule="single")
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(v).to(dev) for v in (x0, xr, ft, ct)]
    us = []
    for kw in ({}, {"rho_restart_iter": 100}):
        with _engine(N, max_contacts_per_step=2, **kw) as eng:
            u = torch.full((B, N, 12), float("nan"), dtype=torch.float64, device=dev)
            eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr())   # u only
            eng.synchronize()
            full = eng.solve(x0, xr, ft, ct)
        assert torch.isfinite(u).all()
        np.testing.assert_array_equal(u.cpu().numpy(), full["u"])
        us.append(full)
    assert (us[1]["status"] == orc.STATUS_SOLVED).sum() >= (us[0]["status"] == orc.STATUS_SOLVED).sum()


def test_ragged_f32_and_warm_start_entry_points(torch_first, built_lib):
    """srbdqp_solve_ragged_f32 / _device_f32 and srbdqp_solve_ragged_warm_device_f64: a mixed-horizon fleet in fp32 equals the
    per-horizon fp32 engines bit for bit (same kernel, same fp64-tile factorisation), and a ragged solve warm-started from its own
    primal / dual solution stops at the first check with the same forces."""
    torch = torch_first
    from g1_locomotion_amd import RaggedMPC, BatchMPC, _lib
    rng = np.random.default_rng(31)
    hz = (8, 12, 20)
    Bq = 90
    Nq = rng.choice(hz, Bq).astype(np.int32)
    parts = [[a[0] for a in orc.synthetic_batch(1, int(N), seed=8100 + i, schedule=("single", "mixed", "double")[i % 3])] for i, N in enumerate(Nq)]
    x0 = np.stack([p[0] for p in parts]); xr = np.concatenate([p[1] for p in parts]); ft = np.concatenate([p[2] for p in parts]); ct = np.concatenate([p[3] for p in parts])
    eng = RaggedMPC(horizons=hz, rho_restart_iter=-1)
    out = eng.solve_packed(Nq, x0, xr, ft, ct, dtype=np.float32)
    off = out["off"]
    assert out["u"].dtype == np.float32 and set(np.unique(out["status"])) <= {orc.STATUS_SOLVED, orc.STATUS_MAX_ITER}
    for N in hz:
        idx = np.where(Nq == N)[0]
        with BatchMPC(horizon=int(N), kernel=_lib.KERNEL_WRENCH, rho_restart_iter=-1, flags=_lib.FLAG_F64_TILES) as one:
            ref = one.solve(x0[idx], np.stack([xr[off[i]:off[i + 1]] for i in idx]), np.stack([ft[off[i]:off[i + 1]] for i in idx]),
                            np.stack([ct[off[i]:off[i + 1]] for i in idx]), dtype=np.float32)
        np.testing.assert_array_equal(out["status"][idx], ref["status"])
        np.testing.assert_array_equal(out["iters"][idx], ref["iters"])
        for j, i in enumerate(idx):
            np.testing.assert_array_equal(out["u"][off[i]:off[i + 1]], ref["u"][j])
    # fp64, device buffers: cold solve with the duals out, then warm-started from its own solution
    dev = torch.device("cuda", 0)
    rows = int(Nq.sum())
    d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (x0, xr, ft, ct)]
    u = torch.zeros((rows, 12), dtype=torch.float64, device=dev); y = torch.zeros((rows, 20), dtype=torch.float64, device=dev)
    u2 = torch.zeros_like(u); y2 = torch.zeros_like(y)
    st = torch.zeros(Bq, dtype=torch.int32, device=dev); it = torch.zeros(Bq, dtype=torch.int32, device=dev)
    st2 = torch.zeros_like(st); it2 = torch.zeros_like(it)
    eng.solve_device(Bq, Nq, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), status=st.data_ptr(),
                     iters=it.data_ptr(), y_out=y.data_ptr())
    eng.solve_device(Bq, Nq, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u2.data_ptr(), status=st2.data_ptr(),
                     iters=it2.data_ptr(), warm_u=u.data_ptr(), warm_y=y.data_ptr(), y_out=y2.data_ptr())
    torch.cuda.synchronize()
    eng.close()
    ok = (st.cpu().numpy() == orc.STATUS_SOLVED)
    assert ok.mean() > 0.9
    assert (it2.cpu().numpy()[ok] == 5).all() and (st2.cpu().numpy()[ok] == orc.STATUS_SOLVED).all()
    du = (u2 - u).abs().cpu().numpy()
    rows_ok = np.concatenate([np.full(int(n), o) for n, o in zip(Nq, ok)])
    assert du[rows_ok].max() < 5e-3
    # the cold fp64 result is the ordinary ragged result
    ref64 = RaggedMPC(horizons=hz, rho_restart_iter=-1)
    o64 = ref64.solve_packed(Nq, x0, xr, ft, ct)
    ref64.close()
    np.testing.assert_array_equal(o64["u"], u.cpu().numpy())


GOLDEN_CASES = [("n10_single_a", 10), ("n10_single_b", 10), ("n10_double", 10), ("n10_mixed", 10), ("n8_mixed", 8), ("n4_single", 4)]


@pytest.mark.parametrize("path", ["staged", "batch", "wave", "wrench"])
@pytest.mark.parametrize("name,N", GOLDEN_CASES)
def test_committed_golden_fixtures_gate_the_kernels(torch_first, built_lib, name, N, path):
    """tests/golden/srbd_qp_golden.npz (inputs -> exact optimum u*, made by tests/golden/make_golden.py) through the HIP path itself: the
    staged batch-1 call (MPC.update), the host-buffer batch call, the one-wave batch kernel and the general kernel.  Forces against the
    frozen exact optimum and the frozen ADMM twin, KKT residuals of the returned primal / dual pair."""
    import os
    from g1_locomotion_amd import _lib, mpc
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "srbd_qp_golden.npz"))
    x0, xr, ft, ct = (gold[f"{name}/{k}"] for k in ("x0", "x_ref", "foot", "contact"))
    u_exact, u_admm, it_admm = gold[f"{name}/u_exact"], gold[f"{name}/u_admm"], int(gold[f"{name}/iters_admm"])
    p = orc.SrbdParams()
    capped = it_admm >= p.max_iter                                   # n10_mixed: the fixed-rho twin itself ends at the cap, 0.055 N from the optimum
    if path == "staged":
        # MPC() runs the engine's defaults, i.e. WITH the automatic rho restart (every 55 iterations, up to twice): the twin of that is the oracle with
        # default_params(); the case fixed-rho ADMM leaves at the cap (n10_mixed) is solved here
        tw = orc.update(orc.default_params(N), x0, xr, ft, ct, pcom_hor=xr[:, 3:6])
        u_admm, it_admm, capped = tw["u"], tw["iters"], tw["status"] == orc.STATUS_MAX_ITER
        assert not capped
        M = mpc.MPC(dt=0.04, horizon=N, strict=False)
        M.init_matrices()
        M.x_ref_hor[:] = xr
        u0, xo = M.update(list(ct), list(ft), xr[:, 3:6].copy(), x_current=x0.reshape(13, 1))
        u, x, status, iters, y = M.u_opt, M.x_opt, M.status, M.iters, None
        assert np.array_equal(u0.reshape(-1), u[0]) and np.array_equal(xo, x)
        M.close()
    else:
        if path == "wave" and not (name.startswith("n10_single") or N == 4):
            pytest.skip("the one-wave kernel holds at most 64 presolved variables")
        kid = {"batch": _lib.KERNEL_COMPACT, "wave": _lib.KERNEL_WAVE, "wrench": _lib.KERNEL_WRENCH}[path]
        with _engine(N, kernel=kid) as eng:
            out = eng.solve(x0[None], xr[None], ft[None], ct[None], want_y=True)
            assert eng.kernel_name().startswith({"batch": "compact_", "wave": "wave_", "wrench": "wrench_"}[path]), eng.kernel_name()
        u, x, status, iters, y = out["u"][0], out["x"][0], int(out["status"][0]), int(out["iters"][0]), out["y"][0]
    assert status == (orc.STATUS_MAX_ITER if capped else orc.STATUS_SOLVED)
    assert abs(iters - it_admm) <= p.check_every, (iters, it_admm)
    assert np.abs(u - u_admm).max() <= (TOL_TWIN_N if not capped else 2e-2)
    assert np.abs(u - u_exact).max() <= ((TOL_EXACT_N if iters <= 110 else 3 * TOL_EXACT_N) if not capped else 0.1)   # (re-balanced twice: stops further out)
    assert np.abs(x - gold[f"{name}/x_exact"]).max() <= (1e-4 if not capped else 1e-3)
    if y is not None:
        qp = orc.build_qp(p, x0, xr, ft, ct)
        red, vi, ri = orc.presolve(qp, ct)
        kr = orc.kkt_residuals(red["P"], red["q"], red["A"], red["l"], red["u"], u.reshape(-1)[vi] / p.force_scale, y[ri])
        assert kr["primal"] <= (1e-4 if not capped else 1e-2) and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(qp["q"]).max()), kr


def test_documented_ctypes_stub_solves_a_qp(torch_first, built_lib):
    """examples/ctypes_stub.py (verbatim) against the oracle: the reference's own call pattern, one QP."""
    import importlib.util, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ctypes_stub", os.path.join(root, "examples", "ctypes_stub.py"))
    stub = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stub)
    N = 10
    x0, xr, ft, ct = (a[0] for a in orc.synthetic_batch(1, N, seed=56, schedule="double"))
    M = stub.MPC(dt=0.04)
    M.init_matrices()
    ref = orc.update(orc.SrbdParams(), x0, xr, ft, ct, pcom_hor=xr[:, 3:6])
    MPC = M
    for pc in (xr[:, 3:6].copy(), None):
        # the caller's statements as the reference writes them (run_simulation.py:73-82,94-106)
        MPC.x0[:] = x0.reshape(13, 1)
        MPC.x_ref_hor[:] = xr
        contact_horizon, c_horizon, p_com_horizon = [np.array([1, 1, 1, 1])] * MPC.HORIZON_LENGTH, list(ft), pc
        u0, x1 = MPC.update(contact_horizon, c_horizon, p_com_horizon, x_current=MPC.x0, one_rollout=True)
        assert M.status == ref["status"] == orc.STATUS_SOLVED and abs(M.iters - ref["iters"]) <= 5
        assert u0.shape == (12, 1) and x1.shape == (N + 1, 13)
        assert np.abs(u0.reshape(-1) - ref["u"][0]).max() <= TOL_TWIN_N and np.abs(x1 - ref["x"]).max() <= 1e-5
    M.close()


def test_mpc_update_fast_path_equals_the_general_path(torch_first, built_lib):
    """MPC.update() binds srbdqp_update_f64 once and gathers straight into the staging arrays; lists of per-step arrays (the reference's
    call, run_simulation.py:94-101), whole arrays and irregular inputs (nested lists -> the general path) must all give the same QP."""
    from g1_locomotion_amd import mpc
    N = 10
    x0s, xrs, fts, cts = orc.synthetic_batch(6, N, seed=57, schedule="mixed")
    M = mpc.MPC(dt=0.04)
    M.init_matrices()
    for b in range(6):
        x0, xr, ft, ct = x0s[b], xrs[b], fts[b], cts[b]
        M.x_ref_hor[:] = xr
        M.x0[:] = x0.reshape(13, 1)
        ref = orc.update(orc.SrbdParams(), x0, xr, ft, ct, pcom_hor=xr[:, 3:6])
        got = []
        for contact_h, c_h, pc, xc in ((list(ct.astype(np.int64)), list(ft), xr[:, 3:6].copy(), M.x0),      # the reference's form
                                      (ct, ft, xr[:, 3:6], None),                                          # arrays, x_current defaulted
                                      (ct.tolist(), ft.tolist(), xr[:, 3:6].tolist(), x0.tolist()),        # nested lists: general path
                                      (list(ct), list(ft), None, x0.reshape(13, 1))):                      # no CoM horizon: x_ref[:, 3:6]
            u0, x1 = M.update(contact_h, c_h, pc, x_current=xc, one_rollout=True)
            assert u0.shape == (12, 1) and x1.shape == (N + 1, 13) and M.status == ref["status"]
            got.append((u0.copy(), x1.copy(), M.iters))
            assert np.array_equal(M.u_opt[0], u0.reshape(-1)) and np.array_equal(M.x_opt, x1)
            u0b, x1b = M.update(contact_h, c_h, pc, x_current=xc, one_rollout=False)
            assert x1b.shape == (2, 13) and np.array_equal(x1b, x1[:2]) and np.array_equal(u0b, u0)
        for u0, x1, it in got[1:]:
            assert np.array_equal(u0, got[0][0]) and np.array_equal(x1, got[0][1]) and it == got[0][2]
        assert np.abs(got[0][0].reshape(-1) - ref["u"][0]).max() <= TOL_TWIN_N
    M.close()


def test_staged_call_after_an_in_place_restart_does_not_replay_a_stale_second_pass(torch_first, built_lib):
    """Advisor finding (round 3): a staged NO_SPIN call of >= 512 QPs with an explicit rho_restart_iter lands on the one-wave kernel, which
    restarts in place; the host must not start a second pass from the arguments of an EARLIER lazy staged call on the same handle."""
    from g1_locomotion_amd import BatchMPC, _lib
    import c_oracle
    N = 10
    x0, xr, ft, ct = orc.synthetic_batch(600, N, seed=1000, schedule="single")
    p = orc.params_for(N, rho_restart_iter=60, rho_restart_count=1)
    ref = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=4)
    assert (ref["iters"] > 60).sum() >= 2                      # the restart really happens in this batch
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WAVE, flags=_lib.FLAG_NO_SPIN, rho_restart_iter=60, rho_restart_count=1, max_contacts_per_step=2) as eng:
        # staging capacity is small: raise it by going through the host-buffer API for the big batch, and use the staged call with
        # its capacity for the lazy two-pass solve that leaves last_args behind
        st = eng.stage()
        cap = st["capacity"]
        hard = np.argsort(-ref["iters"])[:cap]
        for k, b in enumerate(hard):
            st["x0"][k] = x0[b]; st["x_ref"][k] = xr[b]; st["foot"][k] = ft[b]; st["contact"][k] = ct[b]
        eng.solve_staged(cap, want_x=True)                      # wave kernel forced: restarts in place, nothing lazy may be pending
        assert eng.kernel_name().startswith("wave_")
        first = (st["u"][:cap].copy(), st["iters"][:cap].copy(), st["status"][:cap].copy())
        assert np.array_equal(first[2], ref["status"][hard]) and np.abs(first[1] - ref["iters"][hard]).max() <= 5
        assert first[1].max() <= p.max_iter
        assert np.abs(first[0] - ref["u"][hard]).max() <= 5e-3
    # the same through a handle that HAS a stale lazy first pass behind it (4-wave kernel, two-pass restart), then the wave kernel
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_COMPACT, flags=_lib.FLAG_NO_SPIN, rho_restart_iter=60, rho_restart_count=1) as eng:
        st = eng.stage()
        cap = st["capacity"]
        hard = np.argsort(-ref["iters"])[:cap]
        for k, b in enumerate(hard):
            st["x0"][k] = x0[b]; st["x_ref"][k] = xr[b]; st["foot"][k] = ft[b]; st["contact"][k] = ct[b]
        eng.solve_staged(cap, want_x=True)                      # compact kernel: lazy first pass + host-started second pass
        assert eng.kernel_name().startswith("compact_")
        a = (st["u"][:cap].copy(), st["iters"][:cap].copy(), st["status"][:cap].copy())
        eng.solve_staged(2, want_x=True)                        # again, fewer QPs: must not replay the 16-QP pass
        assert np.array_equal(st["iters"][:2], a[1][:2]) and np.array_equal(st["u"][:2], a[0][:2])
        assert np.array_equal(a[2], ref["status"][hard]) and np.abs(a[1] - ref["iters"][hard]).max() <= 5


@pytest.mark.parametrize("kernel", ["compact", "wave"])
def test_assembly_of_a_flight_phase_qp(torch_first, built_lib, kernel):
    """A QP without a stance contact leaves the dump kernels before they write the friction-row bounds: the host must still report the
    rows the oracle assembles (-inf <= friction rows <= 0, 0 <= fz <= 0), not the memset zeros (advisor finding, round 3)."""
    from g1_locomotion_amd import _lib
    N, B = 10, 3
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=101, schedule="single")
    ct[1] = 0
    with _engine(N, kernel=_lib.KERNEL_WAVE if kernel == "wave" else _lib.KERNEL_COMPACT) as eng:
        got = eng.assemble(x0, xr, ft, ct)
    p = orc.params_for(N)
    for b in range(B):
        qp = orc.build_qp(p, x0[b], xr[b], ft[b], ct[b])
        np.testing.assert_array_equal(got["l"][b], qp["l"])
        np.testing.assert_array_equal(got["u"][b], qp["u"])
    assert np.all(got["P"][1] == 0.0) and np.all(got["q"][1] == 0.0)


# (the last case: restart marks every 5 iterations, so nearly every QP of a 32,768-QP launch continues -- far more records than a list holds (a quarter of the
#  largest launch, round 5): the QPs that find their list full run their remaining passes in place, with the same results)
@pytest.mark.parametrize("N,every,count,schedule,B", [(10, 0, 0, "single", 4096), (10, 25, 3, "single", 1024), (8, 30, 2, "single", 1024), (4, 25, 3, "double", 512),
                                                      (4, 5, 3, "single", 32768)])
def test_deferred_tails_equal_the_restart_in_place(torch_first, built_lib, N, every, count, schedule, B):
    """SRBDQP_FLAG_DEFER_TAIL: a QP that reaches a restart mark unconverged rides in the next solve on the stream instead of holding its own launch up.  Same
    passes, same arithmetic: after srbdqp_flush() every status, iteration count, force and state equals the restart in place, batch by batch -- over a
    pipeline of different batches in different buffers, a batch of another size in between, a dispatch hint, and two launch streams through one handle."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    dev = torch.device("cuda", 0)
    kw = dict(max_contacts_per_step=2 if schedule == "single" else 4, kernel=_lib.KERNEL_WAVE)
    if every:
        kw.update(rho_restart_iter=every, rho_restart_count=count)
    sizes = [B // 2, B, B // 2, B, B]               # (the second solve outgrows the lists the first one allocated: flushed, re-allocated, carried on)
    batches = [orc.synthetic_batch(sizes[j], N, seed=1000 + 7 * j, schedule=schedule) for j in range(len(sizes))]
    d_in = [[torch.from_numpy(v).to(dev) for v in hb] for hb in batches]

    def outputs():
        return [dict(u=torch.zeros((sz, N, 12), dtype=torch.float64, device=dev), x=torch.zeros((sz, N + 1, 13), dtype=torch.float64, device=dev),
                     st=torch.full((sz,), -77, dtype=torch.int32, device=dev), it=torch.zeros(sz, dtype=torch.int32, device=dev)) for sz in sizes]

    def run(eng, outs, streams, hint):
        for j, (d, o) in enumerate(zip(d_in, outs)):
            s = streams[j % len(streams)]
            if hint and j > 1 and sizes[j] == sizes[1]:
                eng.set_schedule_hint(ref_outs[1]["it"].data_ptr(), sizes[1])
            else:
                eng.set_schedule_hint(0, 0)
            eng.solve_device(sizes[j], d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), o["u"].data_ptr(), x_out=o["x"].data_ptr(),
                             status=o["st"].data_ptr(), iters=o["it"].data_ptr(), stream=s.cuda_stream)

    s0, s1 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    ref_outs = outputs()
    with BatchMPC(horizon=N, **kw) as eng:                          # the restart in place
        if B < 4096 and not every:
            pytest.skip("automatic restart needs 4096 QPs")
        run(eng, ref_outs, [s0], False)
        torch.cuda.synchronize(dev)
        assert eng.kernel_name().startswith("wave_f64"), eng.kernel_name()
    restarted = sum(int((o["it"] > (every or 55)).sum()) for o in ref_outs)
    assert restarted >= 8, restarted                               # the marks are really passed
    for streams, hint in (([s0], False), ([s0], True), ([s0, s1], False)):
        outs = outputs()
        with BatchMPC(horizon=N, flags=_lib.FLAG_DEFER_TAIL, **kw) as eng:
            run(eng, outs, streams, hint)
            assert eng.kernel_name().startswith("wave_defer_f64"), eng.kernel_name()
            torch.cuda.synchronize(dev)
            pending = sum(int((o["st"] == _lib.PENDING).sum()) for o in outs)
            assert pending >= 1                                    # the last launches' continuations are still waiting
            assert all(int((o["st"] == -77).sum()) == 0 for o in outs)
            eng.flush()
            torch.cuda.synchronize(dev)
            eng.flush()                                            # nothing left: a no-op
            torch.cuda.synchronize(dev)
        for j, (o, r) in enumerate(zip(outs, ref_outs)):
            assert torch.equal(o["st"], r["st"]) and torch.equal(o["it"], r["it"]), (j, streams, hint)
            assert float((o["u"] - r["u"]).abs().max()) <= 1e-9 and float((o["x"] - r["x"]).abs().max()) <= 1e-11, (j, float((o["u"] - r["u"]).abs().max()))


def test_deferred_tails_at_n4_without_a_contact_bound(torch_first, built_lib):
    """Advisor, round 4: with max_contacts_per_step = 0 (the default) the device API runs N = 4 on <4, 4>, and srbdqp_flush / srbdqp_synchronize / the
    host-buffer auto-flush used to continue its records on <4, 2> -- a QP with more than two stance contacts in a step then came back
    SRBDQP_CONTACT_BOUND with zero forces.  One instantiation for every defer launch and flush at N = 4 now: double-support QPs left pending by the LAST
    launch (only the flush can finish them) equal the restart in place, through the device API and through host-buffer calls whose contact scans
    alternate between 2 and 4."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    dev = torch.device("cuda", 0)
    N, B = 4, 512
    kw = dict(kernel=_lib.KERNEL_WAVE, rho_restart_iter=25, rho_restart_count=3)          # max_contacts_per_step left at 0
    dbl = orc.synthetic_batch(B, N, seed=4401, schedule="double")
    sgl = orc.synthetic_batch(B, N, seed=4402, schedule="single")
    with BatchMPC(horizon=N, **kw) as eng:
        ref_d, ref_s = eng.solve(*dbl), eng.solve(*sgl)
    assert (ref_d["iters"] > 25).sum() >= 4 and (ref_d["status"] > 0).all()
    with BatchMPC(horizon=N, flags=_lib.FLAG_DEFER_TAIL, **kw) as eng:
        d = [torch.from_numpy(v).to(dev) for v in dbl]
        u = torch.zeros((B, N, 12), dtype=torch.float64, device=dev)
        st = torch.full((B,), -77, dtype=torch.int32, device=dev); it = torch.zeros(B, dtype=torch.int32, device=dev)
        eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), status=st.data_ptr(), iters=it.data_ptr())
        assert eng.kernel_name() == "wave_defer_f64_n4_s4", eng.kernel_name()
        eng.synchronize()                                   # flushes the handle's own stream
        np.testing.assert_array_equal(st.cpu().numpy(), ref_d["status"])
        np.testing.assert_array_equal(it.cpu().numpy(), ref_d["iters"])
        assert np.abs(u.cpu().numpy() - ref_d["u"]).max() <= 1e-9
        for batch, ref in ((sgl, ref_s), (dbl, ref_d), (sgl, ref_s), (dbl, ref_d)):      # host-buffer calls: the scan says 2, 4, 2, 4
            out = eng.solve(*batch)
            np.testing.assert_array_equal(out["status"], ref["status"])
            np.testing.assert_array_equal(out["iters"], ref["iters"])
            assert np.abs(out["u"] - ref["u"]).max() <= 1e-9


def test_status_does_not_depend_on_the_batch_size(torch_first, built_lib):
    """One restart rule for every kernel and batch size (round 4): the same 4096 single-support QPs through the staged batch-1 call (compact_*_lat, passes
    started by the host when a status asks for them), in calls of 512 and in one call of 4096 (one-wave kernel, restart in place) end with identical
    status[]; and the same for 1024 mixed-gait QPs through the staged call (wrench_*_lat), calls of 256 (4-wave kernel) and one call of 1024 (general
    kernel, one launch per pass)."""
    from g1_locomotion_amd import BatchMPC, _lib
    import c_oracle
    N = 10
    for schedule, B, mid, names in (("single", 4096, 512, ("compact_f64_n10_s2_lat", "wave_f64_n10_s2", "wave_f64_n10_s2")),
                                    ("mixed", 1024, 256, ("wrench_f64_n10_lat", "compact_f64_n10_s4", "wrench_f64_n10"))):
        x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=1000, schedule=schedule)
        ref = c_oracle.solve_batch(orc.default_params(N), x0, xr, ft, ct, nthreads=8)
        with BatchMPC(horizon=N) as eng:                        # nothing configured: the defaults
            big = eng.solve(x0, xr, ft, ct)
            assert eng.kernel_name() == names[2], eng.kernel_name()
            st_mid, it_mid, u_mid = [], [], []
            for k in range(0, B, mid):
                o = eng.solve(x0[k:k + mid], xr[k:k + mid], ft[k:k + mid], ct[k:k + mid])
                st_mid.append(o["status"]); it_mid.append(o["iters"]); u_mid.append(o["u"])
            assert eng.kernel_name() == names[1], eng.kernel_name()
            st = eng.stage()
            st_one, it_one, u_one = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros((B, N, 12))
            for b in range(B):
                st["x0"][0] = x0[b]; st["x_ref"][0] = xr[b]; st["foot"][0] = ft[b]; st["contact"][0] = ct[b]
                eng.solve_staged(1, want_x=False)
                st_one[b], it_one[b], u_one[b] = st["status"][0], st["iters"][0], st["u"][0]
                if b == 0:
                    assert eng.kernel_name() == names[0], eng.kernel_name()
        st_mid, it_mid, u_mid = np.concatenate(st_mid), np.concatenate(it_mid), np.concatenate(u_mid)
        np.testing.assert_array_equal(big["status"], ref["status"])
        np.testing.assert_array_equal(st_mid, big["status"])
        np.testing.assert_array_equal(st_one, big["status"])
        assert (big["status"] == orc.STATUS_SOLVED).mean() >= (0.999 if schedule == "single" else 0.998)
        for it, u in ((it_mid, u_mid), (it_one, u_one)):
            assert np.abs(it.astype(int) - big["iters"].astype(int)).max() <= 5
            same = it == big["iters"]
            assert same.mean() >= 0.97 and np.abs(u - big["u"])[same].max() <= 1e-3 and np.abs(u - big["u"]).max() <= 2 * TOL_TWIN_N


def test_mpc_update_rarely_ends_at_the_iteration_cap(torch_first, built_lib):
    """The reference's consumer has no status handling (ros_run_simulation.py:188-218): what MPC.update() returns goes straight to the WBID step.  10,000
    consecutive control steps through MPC.update(): 400 segments of 25 steps, each starting from a synthetic state of the mixed gait (a large disturbance) and
    then receding -- every state the previous plan's prediction, the contact schedule shifted by one step.  With the staged call's automatic rho restart
    (every 55 iterations, up to twice, a further launch only when a status asks for it) fewer than 0.1 % of the solves end at the cap, and fewer than with
    the restart switched off."""
    from g1_locomotion_amd import MPC
    N, SEG, L = 10, 400, 25
    X0, XR, FT, CT = orc.synthetic_batch(SEG, N, seed=77, schedule="mixed")

    def loop(**kw):
        M = MPC(dt=0.04, horizon=N, strict=False, **kw)
        M.init_matrices()
        capped = failed = restarted = 0
        for s in range(SEG):
            x = X0[s].copy()
            M.x_ref_hor[:] = XR[s]
            c_h = list(FT[s])
            for j in range(L):
                u0, xo = M.update(list(np.roll(CT[s], -j, axis=0)), c_h, None, x_current=x.reshape(13, 1))
                capped += M.status == orc.STATUS_MAX_ITER
                failed += M.status < 0
                restarted += M.iters > 55
                x = xo[1].copy()
        M.close()
        return capped, failed, restarted

    capped, failed, restarted = loop()
    capped_off, failed_off, _ = loop(rho_restart_iter=-1)
    assert failed == 0 and failed_off == 0
    assert restarted >= 20                                      # the restart really runs in this loop
    assert capped < 10 and capped < capped_off, (capped, capped_off)


@pytest.mark.parametrize("N,schedule,B,f32,kname", [(10, "mixed", 1024, False, "wrench_f64_n10"), (10, "mixed", 256, False, "compact_f64_n10_s4"),
                                                    (20, "double", 512, False, "wrench_f64_n20"), (20, "double", 512, True, "wrench_f32_n20"),
                                                    (16, "single", 256, False, "compact_f64_n16_s2")])
def test_deferred_restart_passes_on_the_tail_stream(torch_first, built_lib, N, schedule, B, f32, kname):
    """SRBDQP_FLAG_DEFER_TAIL on the kernels that restart by further launches: the restart passes of a solve run on the library's tail stream beside the caller's
    next solves (lists of capped QPs as their dispatch order, three buffer sets in rotation); after srbdqp_flush() every output equals the same solves with the
    passes on the caller's stream, over a pipeline of five batches."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    dev = torch.device("cuda", 0)
    tdt = torch.float32 if f32 else torch.float64
    kw = dict(rho_restart_iter=30, rho_restart_count=2) if N <= 10 else dict(rho_restart_iter=40, rho_restart_count=1)     # (early marks: many QPs pass them)
    batches = [orc.synthetic_batch(B, N, seed=2000 + 7 * j, schedule=schedule) for j in range(5)]
    d_in = [[torch.from_numpy(v).to(dev).to(tdt) if v.dtype == np.float64 else torch.from_numpy(v).to(dev) for v in hb] for hb in batches]

    def run(flags):
        outs = [dict(u=torch.zeros((B, N, 12), dtype=tdt, device=dev), x=torch.zeros((B, N + 1, 13), dtype=tdt, device=dev),
                     st=torch.full((B,), -77, dtype=torch.int32, device=dev), it=torch.zeros(B, dtype=torch.int32, device=dev)) for _ in batches]
        s0 = torch.cuda.Stream(device=dev)
        with BatchMPC(horizon=N, flags=flags, max_contacts_per_step=2 if schedule == "single" else 4, **kw) as eng:
            for d, o in zip(d_in, outs):
                eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), o["u"].data_ptr(), x_out=o["x"].data_ptr(),
                                 status=o["st"].data_ptr(), iters=o["it"].data_ptr(), stream=s0.cuda_stream, f32=f32)
            assert eng.kernel_name() == kname, eng.kernel_name()
            eng.flush()
            s0.synchronize()
        return outs
    ref, got = run(0), run(_lib.FLAG_DEFER_TAIL)
    assert sum(int((o["it"] > kw["rho_restart_iter"]).sum()) for o in ref) >= 8
    for j, (o, r) in enumerate(zip(got, ref)):
        assert torch.equal(o["st"], r["st"]) and torch.equal(o["it"], r["it"]), j
        assert torch.equal(o["u"], r["u"]) and torch.equal(o["x"], r["x"]), j


def _ragged_fleet(dev, HZ, B, j):
    """B QPs with horizons drawn from HZ, packed row by row in the caller's order, on the device (draw j)."""
    import torch
    rng = np.random.default_rng(50 + j)
    Nq = rng.choice(HZ, size=B).astype(np.int32)
    rows = int(Nq.sum()); off = np.concatenate([[0], np.cumsum(Nq)])
    x0 = np.empty((B, 13)); xr = np.empty((rows, 13)); ft = np.empty((rows, 12)); ct = np.empty((rows, 4), np.uint8)
    for N in HZ:
        idx = np.where(Nq == N)[0]
        a, b_, c, d = orc.synthetic_batch(len(idx), N, seed=60 + N + j, schedule="mixed")
        x0[idx] = a
        dst = (off[idx][:, None] + np.arange(N)[None, :]).reshape(-1)
        xr[dst] = b_.reshape(-1, 13); ft[dst] = c.reshape(-1, 12); ct[dst] = d.reshape(-1, 4)
    return dict(B=B, Nq=Nq, rows=rows, d=[torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (x0, xr, ft, ct)])


def test_ragged_restart_passes_on_the_tail_streams(torch_first, built_lib):
    """srbdqp_ragged_create with SRBDQP_FLAG_DEFER_TAIL: the restart passes of every bucket run on the bucket's tail stream beside the next calls (three sets of the
    shared arrays in rotation); after srbdqp_ragged_flush() a pipeline of six calls (two fleets alternating, each with its own outputs) equals the same calls with
    the passes on the buckets' own streams."""
    torch = torch_first
    from g1_locomotion_amd import RaggedMPC, _lib
    dev = torch.device("cuda", 0)
    HZ = (8, 12, 16, 24)
    fleets = [_ragged_fleet(dev, HZ, 600 + 100 * j, j) for j in range(2)]

    def run(flags):
        outs = []
        s0 = torch.cuda.Stream(device=dev)
        eng = RaggedMPC(horizons=HZ, rho_restart_iter=40, rho_restart_count=2, **({"flags": flags} if flags else {}))
        for k in range(6):
            f = fleets[k % 2]
            o = dict(u=torch.zeros((f["rows"], 12), dtype=torch.float64, device=dev), x=torch.zeros((f["rows"] + f["B"], 13), dtype=torch.float64, device=dev),
                     st=torch.zeros(f["B"], dtype=torch.int32, device=dev), it=torch.zeros(f["B"], dtype=torch.int32, device=dev))
            d = f["d"]
            eng.solve_device(f["B"], f["Nq"], d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), o["u"].data_ptr(), x_out=o["x"].data_ptr(),
                             status=o["st"].data_ptr(), iters=o["it"].data_ptr(), stream=s0.cuda_stream)
            outs.append(o)
        eng.flush(s0.cuda_stream)
        s0.synchronize()
        eng.close()
        return outs
    ref, got = run(0), run(_lib.FLAG_DEFER_TAIL)
    assert sum(int((o["it"] > 40).sum()) for o in ref) >= 20
    for k, (o, r) in enumerate(zip(got, ref)):
        assert torch.equal(o["st"], r["st"]) and torch.equal(o["it"], r["it"]) and torch.equal(o["u"], r["u"]) and torch.equal(o["x"], r["x"]), k


def _assert_deferred_equals_in_stream(torch, ref, got, mark):
    """every call of a DEFER_TAIL pipeline equals the same call with flags = 0, and the case is honest: at least a quarter of each reference call's QPs pass the mark"""
    for j, (o, r) in enumerate(zip(got, ref)):
        assert 4 * int((r["it"] > mark).sum()) >= r["it"].numel(), (j, int((r["it"] > mark).sum()), r["it"].numel())
        assert torch.equal(o["st"], r["st"]) and torch.equal(o["it"], r["it"]), j
        assert torch.equal(o["u"], r["u"]) and torch.equal(o["x"], r["x"]), j


def test_deferred_restart_passes_survive_growing_buffers(torch_first, built_lib):
    """SRBDQP_FLAG_DEFER_TAIL, calls of 48, 160 and 48 QPs on one stream without a wait in between: the second call outgrows the restart buffers of the first
    while the first call's passes may still be pending on the tail stream, the third reuses the grown buffers.  After one flush every output equals the same
    pipeline with the passes on the caller's stream."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    dev = torch.device("cuda", 0)
    N, sizes = 10, (48, 160, 48)
    batches = [orc.synthetic_batch(B, N, seed=2000 + 7 * j, schedule="mixed") for j, B in enumerate(sizes)]
    d_in = [[torch.from_numpy(v).to(dev) for v in hb] for hb in batches]

    def run(flags):
        outs = [dict(u=torch.zeros((B, N, 12), dtype=torch.float64, device=dev), x=torch.zeros((B, N + 1, 13), dtype=torch.float64, device=dev),
                     st=torch.full((B,), -77, dtype=torch.int32, device=dev), it=torch.zeros(B, dtype=torch.int32, device=dev)) for B in sizes]
        s0 = torch.cuda.Stream(device=dev)
        with BatchMPC(horizon=N, flags=flags, max_contacts_per_step=4, rho_restart_iter=25, rho_restart_count=2) as eng:
            for B, d, o in zip(sizes, d_in, outs):
                eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), o["u"].data_ptr(), x_out=o["x"].data_ptr(),
                                 status=o["st"].data_ptr(), iters=o["it"].data_ptr(), stream=s0.cuda_stream)
            eng.flush()
            s0.synchronize()
        return outs
    _assert_deferred_equals_in_stream(torch, run(0), run(_lib.FLAG_DEFER_TAIL), 25)


def test_ragged_restart_passes_survive_growing_buffers(torch_first, built_lib):
    """The ragged twin: calls of 48, 160 and 48 QPs over the horizons (8, 12).  The first call reserves 48 + 12 + 64 = 124 QPs, so the second re-allocates the
    index arrays, the restart buffers and the dual buffer while the first call's passes may still be pending on the buckets' tail streams."""
    torch = torch_first
    from g1_locomotion_amd import RaggedMPC, _lib
    dev = torch.device("cuda", 0)
    HZ = (8, 12)
    fleets = [_ragged_fleet(dev, HZ, B, j) for j, B in enumerate((48, 160, 48))]

    def run(flags):
        outs = []
        s0 = torch.cuda.Stream(device=dev)
        eng = RaggedMPC(horizons=HZ, rho_restart_iter=25, rho_restart_count=2, **({"flags": flags} if flags else {}))
        for f in fleets:
            o = dict(u=torch.zeros((f["rows"], 12), dtype=torch.float64, device=dev), x=torch.zeros((f["rows"] + f["B"], 13), dtype=torch.float64, device=dev),
                     st=torch.zeros(f["B"], dtype=torch.int32, device=dev), it=torch.zeros(f["B"], dtype=torch.int32, device=dev))
            d = f["d"]
            eng.solve_device(f["B"], f["Nq"], d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), o["u"].data_ptr(), x_out=o["x"].data_ptr(),
                             status=o["st"].data_ptr(), iters=o["it"].data_ptr(), stream=s0.cuda_stream)
            outs.append(o)
        eng.flush(s0.cuda_stream)
        s0.synchronize()
        eng.close()
        return outs
    _assert_deferred_equals_in_stream(torch, run(0), run(_lib.FLAG_DEFER_TAIL), 25)


@pytest.mark.parametrize("schedule,B,mcs", [("single", 1024, 2), ("mixed", 1024, 4), ("single", 64, 2)])
def test_host_buffer_calls_flush_deferred_work_themselves(torch_first, built_lib, schedule, B, mcs):
    """An engine created with SRBDQP_FLAG_DEFER_TAIL and used through the HOST-buffer call: the call returns finished results (it flushes before it copies back)."""
    from g1_locomotion_amd import BatchMPC, _lib
    N = 10
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=3100, schedule=schedule)
    kw = dict(rho_restart_iter=25, rho_restart_count=3, max_contacts_per_step=mcs)
    with BatchMPC(horizon=N, **kw) as eng:
        ref = eng.solve(x0, xr, ft, ct, want_y=True)
    with BatchMPC(horizon=N, flags=_lib.FLAG_DEFER_TAIL, **kw) as eng:
        got = eng.solve(x0, xr, ft, ct, want_y=True)
        again = eng.solve(x0, xr, ft, ct, want_y=True)             # (the lists are empty again: the second call equals the first)
    assert (ref["iters"] > 25).sum() >= 8 and (ref["status"] != _lib.PENDING).all()
    for o in (got, again):
        np.testing.assert_array_equal(o["status"], ref["status"]); np.testing.assert_array_equal(o["iters"], ref["iters"])
        assert np.abs(o["u"] - ref["u"]).max() <= 1e-9 and np.abs(o["x"] - ref["x"]).max() <= 1e-11 and np.abs(o["y"] - ref["y"]).max() <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 3])
def test_deferred_tails_survive_a_host_far_ahead_of_the_device(seed):
    """tools/defer_fuzz.py: 150 solves of random size on random streams with random hints and flushes, restart marks low enough that most of every batch
    continues (seeds 1 and 3 draw restart 20 x 1: ~95 % continue) and no synchronisation in between, so the host is a hundred launches ahead of the device.
    Every status, iteration count and force must equal the restart in place (a first version of the tail-workgroup sizing lost records here)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "defer_fuzz.py"), "150", str(seed)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 mismatching solves" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
