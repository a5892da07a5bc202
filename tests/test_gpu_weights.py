"""GPU tests of the per-QP cost weights (include/srbdqp.h srbdqp_weights, srbdqp_set_weights / _device, srbdqp_ragged_set_weights / _device): every QP of a
batch with its own q_diag and r_diag, on the general kernel's MODE = 6 instantiation (srbdqp_wrench_wt_kernel), alone or beside per-QP robot records.

The bars are those of tests/test_gpu_robots.py (tests/weights_twin.py check_qp), per QP against the oracle run with THAT QP's weights; the draw
and the seeds are described in tests/weights_twin.py.  B = 16 unless a test says otherwise."""
import numpy as np
import pytest

import srbd_oracle as orc
import weights_twin as wt
from gpu_helpers import device_solve as _device_solve, refusal as _refusal, to_dev as _to_dev

pytestmark = pytest.mark.gpu

B16 = 16


@pytest.fixture(scope="module")
def torch_first():
    import torch  # load torch's HIP runtime before libsrbdqp.so so both share one
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("schedule", wt.SCHEDULES)
@pytest.mark.parametrize("N", wt.HORIZONS)
def test_per_qp_weights_match_the_oracle(torch_first, built_lib, N, schedule):
    from g1_locomotion_amd import BatchMPC
    B = B16
    x0, xr, ft, ct = wt.batch(B, N, wt.batch_seed(N, schedule), schedule)
    rec = wt.draw(B, wt.weights_seed(N))
    with BatchMPC(horizon=N) as eng:
        out0 = eng.solve(x0, xr, ft, ct)                             # the config's weights for every QP
        eng.set_weights(rec)
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}_wt", eng.kernel_name()
    moved, solved, most = 0, 0, 0
    for b in range(B):
        ref = wt.check_qp(out, b, N, wt.params(N, rec[b]), x0, xr, ft, ct)
        moved += int(np.abs(out["u"][b] - out0["u"][b]).max() > 1.0)
        solved += int(ref["status"] == orc.STATUS_SOLVED)
        most = max(most, int(ref["iters"]))
    print(f"N={N} {schedule}: {solved} of {B} SOLVED, {moved} moved by > 1 N, most iterations {most}")
    assert solved >= 14, solved
    assert moved >= B // 2, f"only {moved} of {B} QPs moved by > 1 N from the solution with the config's weights"
    if N == 10:   # the restart passes ran with the record: a QP that needed them agrees with the oracle
        assert most > orc.default_restart(N)[0], most


@pytest.mark.parametrize("N,schedule", [(4, "double"), (10, "mixed"), (10, "single"), (16, "double"), (20, "three")])
def test_uniform_weights_equal_the_config(torch_first, built_lib, N, schedule):
    """Every record = the handle's config: the same QPs as a KERNEL_WRENCH solve without weights (statuses and iteration counts identical, forces and
    roll-out within 1e-9).  The record path forms sqrt(q_diag) and (r_diag s) s by the operations of the host's fill_args() -- a correctly rounded fp64
    square root and two IEEE multiplications in the host's order --, so the results are bit-identical too: printed, then asserted."""
    from g1_locomotion_amd import BatchMPC, _lib
    from g1_locomotion_amd.mpc import weights_array
    B = 48
    x0, xr, ft, ct = wt.batch(B, N, 700 + N, schedule)
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH) as eng:
        ref = eng.solve(x0, xr, ft, ct, want_y=True)
        eng.set_weights(weights_array(B, cfg=eng.cfg))
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}_wt"
    du, dx = np.abs(out["u"] - ref["u"]).max(), np.abs(out["x"] - ref["x"]).max()
    same = np.array_equal(out["u"], ref["u"]) and np.array_equal(out["x"], ref["x"]) and np.array_equal(out["y"], ref["y"])
    print(f"N={N} {schedule}: max |du| {du:.3e} N, max |dx| {dx:.3e}, bit-identical: {same}")
    assert np.array_equal(out["status"], ref["status"]) and np.array_equal(out["iters"], ref["iters"])
    assert du <= 1e-9 and dx <= 1e-9
    assert same, "weights = config: not bit-identical to the solve without weights"


@pytest.mark.parametrize("N", [10, 16])
def test_weights_and_robot_records_combine(torch_first, built_lib, N):
    """Both records on one handle, the setters in either order: per QP against the oracle with both; clearing one leaves the other."""
    from g1_locomotion_amd import BatchMPC
    from test_gpu_robots import _draw as robots_draw
    B = B16
    x0, xr, ft, ct = wt.batch(B, N, wt.batch_seed(N, "mixed"), "mixed")
    rec, rob = wt.draw(B, wt.weights_seed(N)), robots_draw(B, 3900 + N)     # (3900 + N: no QP of the oracle at the 250 cap with both records)
    with BatchMPC(horizon=N) as eng:
        eng.set_robots(rob)
        rb_only = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}_rb"
        eng.set_weights(rec)                                         # records first, then weights
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}_wt"
        eng.set_weights(None)
        back = eng.solve(x0, xr, ft, ct, want_y=True)                # weights cleared: the records stay in force
        assert eng.kernel_name() == f"wrench_f64_n{N}_rb"
    with BatchMPC(horizon=N) as eng:
        eng.set_weights(rec)                                         # weights first, then records
        eng.set_robots(rob)
        out2 = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}_wt"
        eng.set_robots(None)
        wt_only = eng.solve(x0, xr, ft, ct, want_y=True)             # records cleared: the weights stay in force
        assert eng.kernel_name() == f"wrench_f64_n{N}_wt"
    for k in ("u", "x", "y", "status", "iters"):
        assert np.array_equal(out[k], out2[k]), k
        assert np.array_equal(back[k], rb_only[k]), k
    for b in range(B):
        wt.check_qp(out, b, N, wt.params(N, rec[b], rob[b]), x0, xr, ft, ct)
        wt.check_qp(wt_only, b, N, wt.params(N, rec[b]), x0, xr, ft, ct)


def test_schedule_hint_keeps_weights_by_qp_index(torch_first, built_lib):
    torch = torch_first
    from g1_locomotion_amd import BatchMPC
    B, N = 256, 10
    x0, xr, ft, ct = wt.batch(B, N, 31, "mixed")
    rec = wt.draw(B, 33)
    t = _to_dev(torch, x0, xr, ft, ct)
    with BatchMPC(horizon=N) as eng:
        eng.set_weights(rec)
        plain = _device_solve(torch, eng, t, B)
        torch.cuda.synchronize()
        hint = torch.from_numpy(np.random.default_rng(5).integers(0, 250, B).astype(np.int32)).cuda()   # a hint that reorders
        eng.set_schedule_hint(hint.data_ptr(), B)
        hinted = _device_solve(torch, eng, t, B)
        torch.cuda.synchronize()
        eng.set_schedule_hint(0, 0)
    for k in ("u", "x", "status", "iters"):
        assert torch.equal(plain[k], hinted[k]), k


RAGGED_HORIZONS = (8, 12, 16)
RAGGED_B = 48
RAGGED_SEED = 87


@pytest.fixture(scope="module")
def ragged_case():
    """The ragged QPs, their records and the oracle's solution of each with record b (computed once, shared by both cases below)."""
    Nq, x0, xr, ft, ct = wt.ragged_inputs(RAGGED_B, RAGGED_HORIZONS, RAGGED_SEED)
    rec = wt.draw(RAGGED_B, RAGGED_SEED + 1)
    off = np.concatenate([[0], np.cumsum(Nq)])
    refs = [orc.update(wt.params(int(Nq[b]), rec[b]), x0[b], xr[off[b]:off[b + 1]], ft[off[b]:off[b + 1]], ct[off[b]:off[b + 1]]) for b in range(RAGGED_B)]
    return Nq, x0, xr, ft, ct, rec, off, refs


@pytest.mark.parametrize("defer", [False, True])
def test_ragged_weights_follow_the_callers_order(torch_first, built_lib, ragged_case, defer):
    """Horizons {8, 12, 16}, the QPs shuffled across the buckets: QP b of the caller's order solves with record b (against the oracle per QP), without and
    with SRBDQP_FLAG_DEFER_TAIL (the device setter: read in place, beside the deferred passes too), after the flush."""
    torch = torch_first
    from g1_locomotion_amd import RaggedMPC, _lib
    Nq, x0, xr, ft, ct, rec, off, refs = ragged_case
    B, rows = RAGGED_B, int(off[-1])
    t = _to_dev(torch, x0, xr, ft, ct)
    rg = RaggedMPC(horizons=RAGGED_HORIZONS, flags=_lib.FLAG_DEFER_TAIL if defer else 0)
    try:
        keep = torch.from_numpy(rec).cuda() if defer else rec
        rg.set_weights(keep)
        u = torch.empty((rows, 12), dtype=torch.float64, device="cuda"); x = torch.empty((rows + B, 13), dtype=torch.float64, device="cuda")
        st = torch.empty(B, dtype=torch.int32, device="cuda"); it = torch.empty(B, dtype=torch.int32, device="cuda")
        rg.solve_device(B, Nq, t["x0"].data_ptr(), t["xr"].data_ptr(), t["ft"].data_ptr(), t["ct"].data_ptr(), u.data_ptr(), x.data_ptr(), st.data_ptr(),
                        it.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        rg.flush(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        rg.close()
    out = dict(u=u.cpu().numpy(), x=x.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy())
    for b in range(B):
        N, ref = int(Nq[b]), refs[b]
        assert out["status"][b] == ref["status"], (b, N, out["status"][b], ref["status"])
        assert abs(int(out["iters"][b]) - ref["iters"]) <= 5, (b, N, out["iters"][b], ref["iters"])
        assert np.abs(out["u"][off[b]:off[b + 1]] - ref["u"]).max() <= wt.TOL_TWIN_N, (b, N)
        assert np.abs(out["x"][off[b] + b:off[b + 1] + b + 1] - ref["x"]).max() <= 1e-5, (b, N)


def test_ragged_objects_that_refuse_weights(torch_first, built_lib):
    from g1_locomotion_amd import RaggedMPC, SrbdqpError
    from g1_locomotion_amd.mpc import weights_array
    rec = weights_array(4)
    for horizons, text in (((8, 24), "bucket N=24: per-QP cost weights: not at N = 24"), ((3, 4), "SRBDQP_FLAG_ANY_HORIZON")):
        rg = RaggedMPC(horizons=horizons)
        try:
            for arg in (rec, torch_first.from_numpy(rec).cuda()):
                with pytest.raises(SrbdqpError, match=text):
                    rg.set_weights(arg)
            rg.set_weights(None)
        finally:
            rg.close()


def test_ragged_solves_that_weights_refuse(torch_first, built_lib, ragged_case):
    """While weights are set on a ragged object: the fp32 solves and a solve of B > length QPs return SRBDQP_E_INVALID with a message (nothing is launched);
    a solve of B <= length and, after clearing, the fp32 solve are accepted."""
    from g1_locomotion_amd import RaggedMPC, _lib
    Nq, x0, xr, ft, ct, rec, off, refs = ragged_case
    B, E = 6, f"srbdqp error {_lib.E_INVALID}: "
    rows = int(off[B])
    q = (Nq[:B], x0[:B], xr[:rows], ft[:rows], ct[:rows])
    rg = RaggedMPC(horizons=RAGGED_HORIZONS)
    try:
        rg.set_weights(rec[:B])
        f32 = E + "fp32 ragged solve: refused while per-QP cost weights are set (srbdqp_ragged_set_weights): only the fp64 solves read them"
        assert _refusal(lambda: rg.solve_packed(*q, dtype=np.float32)) == f32
        rg.set_weights(rec[:B - 1])
        assert _refusal(lambda: rg.solve_packed(*q)) == E + f"ragged solve of {B} QPs with {B - 1} weight records set: every QP needs its record"
        assert _refusal(lambda: rg.solve_packed(*q, dtype=np.float32)) == f32
        short = rg.solve_packed(Nq[:B - 1], x0[:B - 1], xr[:off[B - 1]], ft[:off[B - 1]], ct[:off[B - 1]])       # B <= length
        assert np.array_equal(short["status"], [refs[b]["status"] for b in range(B - 1)])
        rg.set_weights(None)
        assert _refusal(lambda: rg.solve_packed(*q, dtype=np.float32)) is None
    finally:
        rg.close()


def test_a_bad_device_record_stays_local_and_the_host_setter_names_it(torch_first, built_lib):
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, SrbdqpError, _lib
    B, N = B16, 12
    x0, xr, ft, ct = wt.batch(B, N, 41, "mixed")
    rec = wt.draw(B, 43)
    bad = rec.copy()
    bad[3, 4] = np.nan              # a NaN q
    bad[7, 0] = -1.0                # a negative q
    bad[10, 13] = 0.0               # r_diag = 0
    bad[13, 15] = 1.0               # reserved not 0
    with BatchMPC(horizon=N) as eng:
        eng.set_weights(torch.from_numpy(rec).cuda())
        good = eng.solve(x0, xr, ft, ct, want_y=True)
        dev_bad = torch.from_numpy(bad).cuda()
        eng.set_weights(dev_bad)
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        with pytest.raises(SrbdqpError, match="srbdqp_set_weights: record 3 is invalid"):
            eng.set_weights(bad)
        again = eng.solve(x0, xr, ft, ct, want_y=True)               # the previous setting (the device records) was kept
    for b in range(B):
        if b in (3, 7, 10, 13):
            assert out["status"][b] == _lib.NUMERICAL and out["iters"][b] == 0, (b, out["status"][b])
            assert np.all(out["u"][b] == 0.0) and np.all(out["y"][b] == 0.0) and np.all(np.isfinite(out["x"][b]))
        else:
            for k in ("u", "x", "y", "status", "iters"):
                assert np.array_equal(out[k][b], good[k][b]), (b, k)
    for k in ("u", "x", "y", "status", "iters"):
        assert np.array_equal(again[k], out[k]), k


def test_the_host_setter_and_the_kernel_share_one_bound(torch_first, built_lib):
    """"Finite" is < SRBDQP_WEIGHT_MAX = 1e300 on both sides: a record the kernel would end as SRBDQP_NUMERICAL is one the host setter refuses."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, SrbdqpError, _lib
    B, N = 4, 4
    x0, xr, ft, ct = wt.batch(B, N, 51, "double")
    bad = wt.draw(B, 53)
    bad[2, 5] = 1e300                       # q at the bound
    bad[3, 13] = np.finfo(np.float64).max   # r finite, above it
    with BatchMPC(horizon=N) as eng:
        with pytest.raises(SrbdqpError, match="srbdqp_set_weights: record 2 is invalid"):
            eng.set_weights(bad)
        with pytest.raises(SrbdqpError, match="srbdqp_set_weights: record 3 is invalid"):
            eng.set_weights(np.concatenate([wt.draw(3, 54), bad[3:]]))
        eng.set_weights(torch.from_numpy(bad).cuda())
        out = eng.solve(x0, xr, ft, ct)
    assert out["status"].tolist()[2:] == [_lib.NUMERICAL, _lib.NUMERICAL] and np.all(out["u"][2:] == 0.0)
    assert all(s in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER) for s in out["status"][:2])


def test_what_the_refusal_table_does_not_say_about_weights(torch_first, built_lib):
    """The weights column and rows of the table are in tests/test_gpu_variant_refusals.py; here, with its calls (B = 2, N = 4, full double support), what a
    table of (call, variant) cannot express."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    from g1_locomotion_amd.mpc import weights_array
    from test_gpu_variant_refusals import TAIL as VT, _calls
    B, N = 2, 4
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=610 + N, schedule="double")
    wr = weights_array(B, r_diag=[1e-4, 3e-4])
    wr_dev = torch.from_numpy(wr).cuda()
    E = f"srbdqp error {_lib.E_INVALID}: "
    with BatchMPC(horizon=N) as eng:
        calls = _calls(torch, eng, N)
        eng.set_weights(wr)
        assert _refusal(calls["srbdqp_solve_batch_f64"]) is None and eng.kernel_name() == "wrench_f64_n4_wt"
        # B > length
        eng.set_weights(wr[:1])
        msg = _refusal(calls["srbdqp_solve_batch_f64"])
        assert msg == E + "solve of 2 QPs with 1 weight records set (srbdqp_set_weights): every QP needs its record", msg
        assert _refusal(calls["srbdqp_solve_batch_device_f64"]) == msg
        # the clearing calls, host and device form: a plain handle again
        eng.set_weights(wr_dev)
        eng.set_weights(None)
        eng.set_weights(wr)
        eng.set_weights(torch.empty((0, 16), dtype=torch.float64, device="cuda"))
        for name in ("srbdqp_solve_staged_f64", "srbdqp_solve_batch_f32", "srbdqp_assemble_wrench_f64", "srbdqp_set_contact_normals"):
            assert _refusal(calls[name]) is None, name
        # with normals set (the line above), the weight setters are refused in the normals' words
        for fn, arg in (("srbdqp_set_weights", wr), ("srbdqp_set_weights_device", wr_dev)):
            assert _refusal(lambda: eng.set_weights(arg)) == E + f"{fn}: {VT['normals']}"
        eng.set_weights(None)                                        # (clearing is accepted in every state)
    # an explicit presolved kernel
    for kern in (_lib.KERNEL_COMPACT, _lib.KERNEL_SPLIT, _lib.KERNEL_WAVE):
        with BatchMPC(horizon=N, kernel=kern) as eng:
            eng.set_weights(wr)
            msg = _refusal(lambda: eng.solve(x0, xr, ft, ct))
            assert msg is not None and "per-QP cost weights (srbdqp_set_weights) are read by the general kernel only" in msg, msg
    # a live horizon, rank-aware steps, N = 24
    with BatchMPC(horizon=3) as eng:
        for fn, arg in (("srbdqp_set_weights", wr), ("srbdqp_set_weights_device", wr_dev)):
            assert _refusal(lambda: eng.set_weights(arg)) == E + f"{fn}: {VT['live']}"
    with BatchMPC(horizon=N, rank_aware=True) as eng:
        for fn, arg in (("srbdqp_set_weights", wr), ("srbdqp_set_weights_device", wr_dev)):
            assert _refusal(lambda: eng.set_weights(arg)) == E + f"{fn}: {VT['rank_aware']}"
    with BatchMPC(horizon=24) as eng:
        for arg in (wr, wr_dev):
            msg = _refusal(lambda: eng.set_weights(arg))
            assert msg is not None and msg.startswith(E + "per-QP cost weights: not at N = 24"), msg
        eng.set_weights(None)
