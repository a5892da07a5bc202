"""GPU tests of SRBDQP_FLAG_ANY_HORIZON (include/srbdqp.h): a horizon n without instantiations of its own runs the general kernel instantiated for the next
tabulated horizon N* in its live-horizon mode (srbdqp_wrench.hpp, MODE = 3) on arrays of the caller's shape for n.

Tolerances: the ones tests/test_gpu_wrench.py states for the fp64 general kernel, and no other --
    forces vs the oracle's ADMM twin (orc.update)   <= 2e-3 N, iteration counts within one check interval, x within 1e-5
    forces vs the independent exact QP optimum      <= 5e-2 N, KKT: primal <= 1e-4, stationarity <= 1e-3 |q|_inf
The oracle runs with the engine's automatic rho restart (orc.default_params(n)), as the engine does when nothing is configured.  A QP the oracle itself ends at
the iteration cap is held to its twin only (as in tests/test_gpu_wrench.py); at most one QP in eight of a case may be left out that way.  On the CPU the
oracle leaves out at most 1 of 12 QPs in every case below, and its forces on the solved QPs stay within 6.0e-3 N of the active-set optimum ("three" schedule;
2.6e-2 N over single / double / mixed, the capped QPs included).
"""
import numpy as np
import pytest

import srbd_oracle as orc
from test_gpu_wrench import TOL_EXACT_N, TOL_TWIN_N, _batch
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TABULATED = (4, 8, 10, 12, 16, 20, 24)
LIVE = (1, 2, 3, 5, 7, 9, 11, 13, 15, 18, 19, 21, 23)       # at least one below each N*, both neighbours of a tabulated value at least once
SCHEDULES = ("single", "double", "mixed", "three")


def nstar(n):
    return min(N for N in TABULATED if N >= n)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("n", LIVE)
def test_live_horizon_matches_oracle_and_exact_optimum(torch_first, built_lib, n, schedule):
    from g1_locomotion_amd import BatchMPC
    B = 12
    x0, xr, ft, ct = _batch(B, n, 7, schedule)
    with BatchMPC(horizon=n) as eng:                                  # nothing configured: AUTO, the automatic restart on, the flag set by the wrapper
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{nstar(n)}_h{n}", eng.kernel_name()
    assert out["u"].shape == (B, n, 12) and out["x"].shape == (B, n + 1, 13) and out["y"].shape == (B, 20 * n)
    p = orc.default_params(n)
    left_out = 0
    for b in range(B):
        ref = orc.update(p, x0[b], xr[b], ft[b], ct[b])
        du, dx = np.abs(out["u"][b] - ref["u"]).max(), np.abs(out["x"][b] - ref["x"]).max()
        print(f"n={n} {schedule} qp {b}: status {out['status'][b]}/{ref['status']} iters {out['iters'][b]}/{ref['iters']} |du| {du:.2e} N |dx| {dx:.2e}")
        assert out["status"][b] == ref["status"] and ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER), (b, out["status"][b], ref["status"])
        solved = ref["status"] == orc.STATUS_SOLVED
        assert abs(int(out["iters"][b]) - ref["iters"]) <= p.check_every, (b, out["iters"][b], ref["iters"])
        assert du <= TOL_TWIN_N, (b, du)
        assert dx <= 1e-5
        assert np.array_equal(out["x"][b][0], x0[b])                   # row 0 of the roll-out is the caller's state
        kq, vi, ri = orc.presolve(ref["qp"], ct[b])
        if solved:   # a QP that ends at the iteration cap (status MAX_ITER, on the oracle too) is only held to its twin
            xs, ys = orc.solve_reference(p, ref["qp"])
            de = np.abs(out["u"][b].reshape(-1) - xs * p.force_scale).max()
            print(f"    vs the exact optimum {de:.2e} N")
            assert de <= TOL_EXACT_N
            kr = orc.kkt_residuals(kq["P"], kq["q"], kq["A"], kq["l"], kq["u"], out["u"][b].reshape(-1)[vi] / p.force_scale, out["y"][b][ri])
            assert kr["primal"] <= 1e-4 and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(ref["qp"]["q"]).max()), kr
        else:
            left_out += 1
        off = np.setdiff1d(np.arange(12 * n), vi)
        assert np.all(out["u"][b].reshape(-1)[off] == 0.0)              # swing contacts carry exactly zero force
        offr = np.setdiff1d(np.arange(20 * n), ri)
        assert np.all(out["y"][b][offr] == 0.0)
    assert left_out <= B // 8, left_out


def test_no_write_outside_a_qps_rows(torch_first, built_lib):
    """A device-buffer solve of 64 QPs at n = 15 (kernel for N* = 16) into output tensors one QP longer at each end, pre-filled with a sentinel: the guard QPs
    stay bit-identical, every value of the 64 is written, and each QP equals the same QP solved alone."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC
    n, B = 15, 64
    x0, xr, ft, ct = orc.synthetic_batch(B, n, seed=7, schedule="mixed")
    ct[5] = 0                                                          # a QP with nothing to solve takes the early path: its rows too
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(v).to(dev) for v in (x0, xr, ft, ct)]
    SENT, ISENT = -7.25e33, -77
    u = torch.full((B + 2, n, 12), SENT, dtype=torch.float64, device=dev)
    x = torch.full((B + 2, n + 1, 13), SENT, dtype=torch.float64, device=dev)
    y = torch.full((B + 2, 20 * n), SENT, dtype=torch.float64, device=dev)
    st = torch.full((B + 2,), ISENT, dtype=torch.int32, device=dev)
    it = torch.full((B + 2,), ISENT, dtype=torch.int32, device=dev)
    with BatchMPC(horizon=n) as eng:
        eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u[1:].data_ptr(), x_out=x[1:].data_ptr(), y_out=y[1:].data_ptr(),
                         status=st[1:].data_ptr(), iters=it[1:].data_ptr())
        eng.synchronize()
        assert eng.kernel_name() == "wrench_f64_n16_h15"
        u, x, y, st, it = (t.cpu().numpy() for t in (u, x, y, st, it))
        for a in (u, x, y):
            assert np.all(a[0] == SENT) and np.all(a[-1] == SENT)
            assert not np.any(a[1:-1] == SENT)
        for a in (st, it):
            assert a[0] == ISENT and a[-1] == ISENT and not np.any(a[1:-1] == ISENT)
        assert st[1 + 5] == orc.STATUS_SOLVED and it[1 + 5] == 0 and np.all(u[1 + 5] == 0.0) and np.all(y[1 + 5] == 0.0)
        for b in range(B):
            one = eng.solve(x0[b:b + 1], xr[b:b + 1], ft[b:b + 1], ct[b:b + 1], want_y=True)
            assert one["status"][0] == st[1 + b] and one["iters"][0] == it[1 + b], b
            assert np.array_equal(one["u"][0], u[1 + b]) and np.array_equal(one["x"][0], x[1 + b]) and np.array_equal(one["y"][0], y[1 + b]), b


def test_ragged_fleet_at_live_horizons(torch_first, built_lib):
    """RaggedMPC(horizons=(6, 9, 15, 22)) on a shuffled fleet of 200 QPs: every QP bit-equal to the per-horizon BatchMPC result (as
    test_ragged_device_call_does_not_block_and_buckets_overlap does for the tabulated horizons), statuses equal to the oracle's and iteration counts within one
    check interval of it."""
    torch = torch_first
    from g1_locomotion_amd import RaggedMPC, BatchMPC, SrbdqpError
    rng = np.random.default_rng(11)
    hz = (6, 9, 15, 22)
    Bq = 200
    Nq = rng.choice(hz, Bq).astype(np.int32)
    parts = [[a[0] for a in orc.synthetic_batch(1, int(N), seed=7000 + i, schedule="mixed")] for i, N in enumerate(Nq)]
    x0 = np.stack([p[0] for p in parts]); xr = np.concatenate([p[1] for p in parts]); ft = np.concatenate([p[2] for p in parts]); ct = np.concatenate([p[3] for p in parts])
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(v).to(dev) for v in (x0, xr, ft, ct)]
    rows = int(Nq.sum())
    u = torch.zeros((rows, 12), dtype=torch.float64, device=dev); xo = torch.zeros((rows + Bq, 13), dtype=torch.float64, device=dev)
    st = torch.zeros(Bq, dtype=torch.int32, device=dev); it = torch.zeros(Bq, dtype=torch.int32, device=dev)
    eng = RaggedMPC(horizons=hz)
    try:
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            eng.solve_device(Bq, Nq, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), x_out=xo.data_ptr(), status=st.data_ptr(),
                             iters=it.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        bad = Nq.copy()
        bad[3] = 7                                                     # a horizon this object was not created for: still refused
        with pytest.raises(SrbdqpError, match="not created for"):
            eng.solve_device(Bq, bad, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), status=st.data_ptr(), iters=it.data_ptr())
    finally:
        eng.close()
    u, xo, st, it = u.cpu().numpy(), xo.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(Nq)])
    for N in hz:
        idx = np.where(Nq == N)[0]
        assert idx.size > 0
        with BatchMPC(horizon=int(N)) as one:
            ref = one.solve(x0[idx], np.stack([xr[off[i]:off[i + 1]] for i in idx]), np.stack([ft[off[i]:off[i + 1]] for i in idx]),
                            np.stack([ct[off[i]:off[i + 1]] for i in idx]))
            assert one.kernel_name() == f"wrench_f64_n{nstar(N)}_h{N}"
        np.testing.assert_array_equal(st[idx], ref["status"])
        np.testing.assert_array_equal(it[idx], ref["iters"])
        for j, i in enumerate(idx):
            np.testing.assert_array_equal(u[off[i]:off[i + 1]], ref["u"][j])
            np.testing.assert_array_equal(xo[off[i] + i:off[i + 1] + i + 1], ref["x"][j])
    for i in range(Bq):
        p = orc.default_params(int(Nq[i]))
        r = orc.update(p, x0[i], xr[off[i]:off[i + 1]], ft[off[i]:off[i + 1]], ct[off[i]:off[i + 1]])
        assert st[i] == r["status"], (i, Nq[i], st[i], r["status"], it[i], r["iters"])
        assert abs(int(it[i]) - r["iters"]) <= p.check_every, (i, Nq[i], it[i], r["iters"])


def test_mpc_drop_in_at_horizon_15(torch_first, built_lib):
    """MPC(horizon=15): update() (srbdqp_update_f64) and solve() (srbdqp_solve_staged_f64) on one QP against the oracle, the whole roll-out and its first two
    rows; the staged calls take the HIP launch of the batch instantiation; prepare() has no live-horizon form."""
    from g1_locomotion_amd import mpc, SrbdqpError
    n = 15
    x0, xr, ft, ct = (a[0] for a in orc.synthetic_batch(1, n, seed=55, schedule="double"))
    M = mpc.MPC(dt=0.04, horizon=n)
    M.init_matrices()
    assert M._engine.batch1_launch_path().startswith("hip: ") and "SRBDQP_FLAG_ANY_HORIZON" in M._engine.batch1_launch_path()
    M.x0[:] = x0.reshape(13, 1)
    M.x_ref_hor[:] = xr
    c_horizon = [ft[k].copy() for k in range(n)]
    contact_horizon = [ct[k].copy() for k in range(n)]
    p_com_horizon = M.x_ref_hor[:, 3:6].copy()
    ref = orc.update(orc.default_params(n), x0, xr, ft, ct, pcom_hor=p_com_horizon)
    assert ref["status"] == orc.STATUS_SOLVED
    u_opt0, x_opt1 = M.update(contact_horizon, c_horizon, p_com_horizon, x_current=M.x0, one_rollout=True)
    assert M._engine.kernel_name() == "wrench_f64_n16_h15"
    assert u_opt0.shape == (12, 1) and x_opt1.shape == (n + 1, 13)
    assert M.status == ref["status"] and abs(M.iters - ref["iters"]) <= orc.default_params(n).check_every
    assert np.abs(u_opt0.flatten() - ref["u"][0]).max() <= TOL_TWIN_N
    assert np.abs(M.u_opt - ref["u"]).max() <= TOL_TWIN_N
    assert np.abs(x_opt1 - ref["x"]).max() <= 1e-5
    u2, x2 = M.update(contact_horizon, c_horizon, p_com_horizon, x_current=M.x0, one_rollout=False)
    assert x2.shape == (2, 13) and np.array_equal(x2, x_opt1[:2]) and np.array_equal(u2, u_opt0)
    us, xs = M.solve(M.x0, M.x_ref_hor, c_horizon, contact_horizon, p_com_horizon)
    assert us.shape == (n, 12) and xs.shape == (n + 1, 13)
    assert np.array_equal(us[0].reshape(12, 1), u_opt0) and np.array_equal(xs, x_opt1)
    # without pcom (the CoM horizon from x_ref), arrays instead of lists
    ref3 = orc.update(orc.default_params(n), x0, xr, ft, ct)
    u3, x3 = M.update(ct, ft, None, x_current=M.x0, one_rollout=True)
    assert np.abs(u3.flatten() - ref3["u"][0]).max() <= TOL_TWIN_N and np.abs(x3 - ref3["x"]).max() <= 1e-5
    with pytest.raises(SrbdqpError, match="SRBDQP_FLAG_ANY_HORIZON"):
        M.prepare(contact_horizon, c_horizon, p_com_horizon)
    M.close()


def test_deferred_passes_equal_the_restart_in_place(torch_first, built_lib):
    """SRBDQP_FLAG_DEFER_TAIL at n = 9 (kernel for N* = 10; restart 55 x 2): the restart passes run on the library's tail stream beside the next solves; after
    flush() every status, iteration count, force and state equals the restart in place (bounds of test_deferred_tails_equal_the_restart_in_place) -- over a
    pipeline of batches in their own buffers and two launch streams through one handle."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    dev = torch.device("cuda", 0)
    n, B = 9, 4096
    sizes = [B // 2, B, B]
    batches = [orc.synthetic_batch(sizes[j], n, seed=1000 + 7 * j, schedule="single") for j in range(len(sizes))]
    d_in = [[torch.from_numpy(v).to(dev) for v in hb] for hb in batches]

    def outputs():
        return [dict(u=torch.zeros((sz, n, 12), dtype=torch.float64, device=dev), x=torch.zeros((sz, n + 1, 13), dtype=torch.float64, device=dev),
                     st=torch.full((sz,), -77, dtype=torch.int32, device=dev), it=torch.zeros(sz, dtype=torch.int32, device=dev)) for sz in sizes]

    def run(eng, outs, streams):
        for j, (d, o) in enumerate(zip(d_in, outs)):
            s = streams[j % len(streams)]
            eng.solve_device(sizes[j], d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), o["u"].data_ptr(), x_out=o["x"].data_ptr(),
                             status=o["st"].data_ptr(), iters=o["it"].data_ptr(), stream=s.cuda_stream)

    s0, s1 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    ref_outs = outputs()
    with BatchMPC(horizon=n) as eng:                                    # the restart in place (one more launch per pass on the same stream)
        run(eng, ref_outs, [s0])
        torch.cuda.synchronize(dev)
        assert eng.kernel_name() == "wrench_f64_n10_h9", eng.kernel_name()
    restarted = sum(int((o["it"] > 55).sum()) for o in ref_outs)
    print("QPs past the first restart mark:", restarted)
    assert restarted >= 8, restarted                                   # the marks are really passed
    for streams in ([s0], [s0, s1]):
        outs = outputs()
        with BatchMPC(horizon=n, flags=_lib.FLAG_DEFER_TAIL) as eng:
            run(eng, outs, streams)
            assert eng.kernel_name() == "wrench_f64_n10_h9", eng.kernel_name()
            eng.flush()
            torch.cuda.synchronize(dev)
            eng.flush()                                                # nothing left: a no-op
            torch.cuda.synchronize(dev)
        for j, (o, r) in enumerate(zip(outs, ref_outs)):
            assert torch.equal(o["st"], r["st"]) and torch.equal(o["it"], r["it"]), (j, len(streams))
            assert float((o["u"] - r["u"]).abs().max()) <= 1e-9 and float((o["x"] - r["x"]).abs().max()) <= 1e-11, (j, float((o["u"] - r["u"]).abs().max()))


def test_refusals_name_the_flag(torch_first, built_lib):
    """The calls without a live-horizon form return SRBDQP_E_INVALID with a message that names the flag; the handle keeps working."""
    torch = torch_first
    import ctypes as C
    from g1_locomotion_amd import BatchMPC, RaggedMPC, SrbdqpError, _lib
    from g1_locomotion_amd.mpc import robots_array
    n, B = 7, 4
    x0, xr, ft, ct = orc.synthetic_batch(B, n, seed=51, schedule="double")
    flag = "SRBDQP_FLAG_ANY_HORIZON"
    with BatchMPC(horizon=n) as eng:
        ref = eng.solve(x0, xr, ft, ct)
        with pytest.raises(SrbdqpError, match=flag):
            eng.solve(x0, xr, ft, ct, dtype=np.float32)
        f32 = [torch.from_numpy(np.asarray(v, np.float32) if v.dtype == np.float64 else v).cuda() for v in (x0, xr, ft, ct)]
        u32 = torch.zeros((B, n, 12), dtype=torch.float32, device="cuda")
        with pytest.raises(SrbdqpError, match=flag):
            eng.solve_device(B, f32[0].data_ptr(), f32[1].data_ptr(), f32[2].data_ptr(), f32[3].data_ptr(), u32.data_ptr(), f32=True)
        eng.stage()
        with pytest.raises(SrbdqpError, match=flag):
            eng.prepare_staged(1)
        with pytest.raises(SrbdqpError, match=flag):
            eng.solve_prepared(1)
        with pytest.raises(SrbdqpError, match=flag):
            eng.assemble(x0, xr, ft, ct)
        with pytest.raises(SrbdqpError, match=flag):
            eng.assemble_wrench(x0, xr, ft, ct)
        with pytest.raises(SrbdqpError, match=flag):
            eng.set_robots(robots_array(B))
        with pytest.raises(SrbdqpError, match=flag):
            eng.set_robots(torch.from_numpy(robots_array(B)).cuda())
        eng.set_robots(None)                                           # clearing what was never set is not an error
        raw = _lib.load()
        for fn, args in (("srbdqp_solve_batch_f32", (eng._h, 1) + (None,) * 12), ("srbdqp_prepare_staged_f64", (eng._h, 1, 0)),
                         ("srbdqp_solve_prepared_f64", (eng._h, 1, 1, 0)), ("srbdqp_assemble_wrench_f64", (eng._h, 1) + (None,) * 9)):
            assert getattr(raw, fn)(*args) == _lib.E_INVALID, fn
            assert flag.encode() in raw.srbdqp_last_error(eng._h), fn
        again = eng.solve(x0, xr, ft, ct)
        assert eng.kernel_name() == "wrench_f64_n8_h7"
        for k in ("u", "x", "status", "iters"):
            assert np.array_equal(again[k], ref[k]), k
    for kern in (_lib.KERNEL_COMPACT, _lib.KERNEL_SPLIT, _lib.KERNEL_WAVE):
        with pytest.raises(SrbdqpError, match=flag):
            BatchMPC(horizon=n, kernel=kern)
    for bad in (0, 25, -3):
        with pytest.raises(SrbdqpError, match="unsupported horizon"):
            BatchMPC(horizon=bad)
    cfg = _lib.default_config()
    cfg.horizon = n
    h = C.c_void_p()
    assert raw.srbdqp_create(C.byref(cfg), C.byref(h)) == _lib.E_INVALID and not h.value          # without the flag: as ever
    rg = RaggedMPC(horizons=(6, 8))
    try:
        Nq = np.array([6, 8, 6], np.int32)
        parts = [[a[0] for a in orc.synthetic_batch(1, int(N), seed=60 + i, schedule="mixed")] for i, N in enumerate(Nq)]
        rx0 = np.stack([p[0] for p in parts]); rxr = np.concatenate([p[1] for p in parts]); rft = np.concatenate([p[2] for p in parts]); rct = np.concatenate([p[3] for p in parts])
        rg.solve_packed(Nq, rx0, rxr, rft, rct)
        with pytest.raises(SrbdqpError, match=flag):
            rg.solve_packed(Nq, rx0, rxr, rft, rct, dtype=np.float32)
        with pytest.raises(SrbdqpError, match=flag):
            rg.set_robots(robots_array(3))
    finally:
        rg.close()


def test_the_flag_on_a_tabulated_horizon_changes_nothing(torch_first, built_lib):
    from g1_locomotion_amd import BatchMPC, _lib
    N, B = 10, 600
    for schedule in ("single", "double"):
        x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=31, schedule=schedule)
        with BatchMPC(horizon=N) as eng:
            ref = eng.solve(x0, xr, ft, ct, want_y=True)
            ref_name = eng.kernel_name()
            ref_one = eng.solve(x0[:1], xr[:1], ft[:1], ct[:1])
            ref_name_one = eng.kernel_name()
        with BatchMPC(horizon=N, flags=_lib.FLAG_ANY_HORIZON) as eng:
            out = eng.solve(x0, xr, ft, ct, want_y=True)
            assert eng.kernel_name() == ref_name
            one = eng.solve(x0[:1], xr[:1], ft[:1], ct[:1])
            assert eng.kernel_name() == ref_name_one
            out32 = eng.solve(x0[:8], xr[:8], ft[:8], ct[:8], dtype=np.float32)     # nothing is refused on such a handle
            assert eng.kernel_name() == "wrench_f32_n10" and (out32["status"] == orc.STATUS_SOLVED).all()
        for k in ("u", "x", "y", "status", "iters"):
            assert np.array_equal(out[k], ref[k]), (schedule, k)
            if k != "y":
                assert np.array_equal(one[k], ref_one[k]), (schedule, k)


def test_cascade_calls_take_a_live_horizon(torch_first, built_lib):
    """srbdqp_mpc_inputs_* at n = 15 against the same call's rows at N = 16 (the inputs of step k do not depend on the horizon), feeding a solve; wbid_reference
    on its result."""
    from g1_locomotion_amd import BatchMPC
    B, n = 40, 15
    rng = np.random.default_rng(3)
    x0 = np.zeros((B, 13)); x0[:, 3:6] = rng.normal(size=(B, 3)) * 0.05 + [0.0, 0.0, 0.55]; x0[:, 9:11] = rng.normal(size=(B, 2)) * 0.1; x0[:, 12] = -9.80665
    feet = np.tile(np.array([0.08, 0.1, 0.0, -0.08, 0.1, 0.0, 0.08, -0.1, 0.0, -0.08, -0.1, 0.0]), (B, 1)) + np.tile(x0[:, 3:6] * [1, 1, 0], (1, 4))
    stamp = rng.uniform(0, 3, B); v_ref = rng.normal(size=(B, 2)) * 0.2
    with BatchMPC(horizon=16) as e16:
        full = e16.mpc_inputs(x0, feet, stamp, v_ref, (0.0, 0.0, 0.55))
    with BatchMPC(horizon=n) as eng:
        got = eng.mpc_inputs(x0, feet, stamp, v_ref, (0.0, 0.0, 0.55))
        for k in ("x_ref", "foot", "contact", "pcom"):
            assert got[k].shape[1] == n and np.array_equal(got[k], full[k][:, :n]), k
        assert np.array_equal(got["landing"], full["landing"])
        out = eng.solve(x0, got["x_ref"], got["foot"], got["contact"], pcom=got["pcom"])
        assert eng.kernel_name() == "wrench_f64_n16_h15"
        p = orc.default_params(n)
        for b in range(0, B, 8):
            ref = orc.update(p, x0[b], got["x_ref"][b], got["foot"][b], got["contact"][b], pcom_hor=got["pcom"][b])
            assert out["status"][b] == ref["status"] and np.abs(out["u"][b] - ref["u"]).max() <= TOL_TWIN_N
        w = eng.wbid_reference(out["x"][:, 1], out["u"][:, 0], got["foot"][:, 0])
        assert np.isfinite(w["base_acc"]).all() and w["R"].shape == (B, 3, 3)
