"""GPU tests of the external wrench (include/srbdqp.h srbdqp_set_external_wrench / _device, srbdqp_ragged_set_external_wrench / _device): a known
world-frame torque and force on the body per horizon step of every QP, on the general kernel's MODE = 7 instantiation (srbdqp_wrench_ew_kernel), alone or
beside per-QP robot records and cost weights.

The bars are those of tests/weights_twin.py, per QP against the twin of tests/ext_wrench_twin.py run with THAT QP's wrench; the draw and the seeds are
described there.  B = 16 unless a test says otherwise."""
import numpy as np
import pytest

import srbd_oracle as orc
import weights_twin as wt
import ext_wrench_twin as ew
from gpu_helpers import device_solve as _device_solve, refusal as _refusal, to_dev as _to_dev

pytestmark = pytest.mark.gpu

B16 = ew.B16
KEYS = ("u", "x", "y", "status", "iters")
EW_TAIL = ("refused while an external wrench is set (srbdqp_set_external_wrench): only the fp64 batch and ragged solves on the general kernel read it "
           "-- srbdqp_set_external_wrench(h, NULL, 0) goes back to no wrench")


@pytest.fixture(scope="module")
def torch_first():
    import torch  # load torch's HIP runtime before libsrbdqp.so so both share one
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("schedule", ew.SCHEDULES)
@pytest.mark.parametrize("N", ew.HORIZONS)
def test_per_qp_wrenches_match_the_twin(torch_first, built_lib, N, schedule):
    """Per QP against the twin, by the bars of weights_twin.check_qp.

    Measured on an MI355X: statuses and iteration counts equal the twin's in all 24 cases; worst |u - twin| 6e-9 N (N = 4), 1.2e-7 (8), 3.3e-7 (10), 3.0e-6 (12),
    5.8e-6 (16), 2.7e-5 N (20) against the bar of 2e-3 N, worst |x - twin| 5.6e-9, 9.1e-8, 3.2e-7, 9.1e-7, 3.0e-6 and 8.0e-6 against the bar of 1e-5.  The bar
    on x is what the refinement of x_q in MODE = 7 is for: without it the drawn torque's |q| of 1e6 - 1e7 left x up to 1.3e-4 from the
    twin at N >= 10, carried by the yaw rate."""
    from g1_locomotion_amd import BatchMPC
    B = B16
    x0, xr, ft, ct = wt.batch(B, N, ew.batch_seed(N, schedule), schedule)
    w = ew.draw(B, N, ew.wrench_seed(N))
    with BatchMPC(horizon=N) as eng:
        out0 = eng.solve(x0, xr, ft, ct)                             # no wrench
        eng.set_external_wrench(w)
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}_ew", eng.kernel_name()
    moved, solved, most = 0, 0, 0
    p = ew.params(N)
    refs = [ew.update(p, x0[b], xr[b], ft[b], ct[b], w[b]) for b in range(B)]
    print(f"N={N} {schedule}: max |u - twin| {max(np.abs(out['u'][b] - refs[b]['u']).max() for b in range(B)):.3e} N, "
          f"max |x - twin| {max(np.abs(out['x'][b] - refs[b]['x']).max() for b in range(B)):.3e}, "
          f"max |iters - twin| {max(abs(int(out['iters'][b]) - refs[b]['iters']) for b in range(B))}")
    for b in range(B):
        ref = ew.check_qp(out, b, N, p, x0, xr, ft, ct, w[b], refs[b])
        moved += int(np.abs(out["u"][b] - out0["u"][b]).max() > 1.0)
        solved += int(ref["status"] == orc.STATUS_SOLVED)
        most = max(most, int(ref["iters"]))
    print(f"N={N} {schedule}: {solved} of {B} SOLVED, {moved} moved by > 1 N, most iterations {most}")
    assert solved >= 14, solved
    assert moved >= B // 2, f"only {moved} of {B} QPs moved by > 1 N from the solution without the wrench"
    if N == 10:   # the restart passes ran under the wrench: a QP that needed them agrees with the twin
        assert most > orc.default_restart(N)[0], most


ZERO_CASES = [(4, "double"), (10, "mixed"), (10, "single"), (16, "double"), (20, "three")]


@pytest.fixture(scope="module")
def zero_runs(torch_first, built_lib):
    """Per case: (a KERNEL_WRENCH solve without a wrench, the same QPs under a zero wrench, the kernel's name).  Computed once: the last case asserts what
    all five showed."""
    from g1_locomotion_amd import BatchMPC, _lib
    runs = {}
    for N, schedule in ZERO_CASES:
        B = 48
        x0, xr, ft, ct = wt.batch(B, N, 700 + N, schedule)
        with BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH) as eng:
            ref = eng.solve(x0, xr, ft, ct, want_y=True)
            eng.set_external_wrench(np.zeros((B, N, 6)))
            out = eng.solve(x0, xr, ft, ct, want_y=True)
            runs[(N, schedule)] = (ref, out, eng.kernel_name())
    return runs


@pytest.mark.parametrize("N,schedule", ZERO_CASES)
def test_a_zero_wrench_equals_no_wrench(zero_runs, N, schedule):
    """A zero wrench: the same QPs as a KERNEL_WRENCH solve without one -- statuses and iteration counts identical, forces and roll-out within 1e-9.
    x_ref - 0.0 and s + 0.0 are exact, so the results should be bit-identical: printed per case, and asserted where all five cases showed it."""
    ref, out, name = zero_runs[(N, schedule)]
    assert name == f"wrench_f64_n{N}_ew"
    du, dx = np.abs(out["u"] - ref["u"]).max(), np.abs(out["x"] - ref["x"]).max()
    same = {c: all(np.array_equal(o[k], r[k]) for k in ("u", "x", "y")) for c, (r, o, _) in zero_runs.items()}
    print(f"N={N} {schedule}: max |du| {du:.3e} N, max |dx| {dx:.3e}, bit-identical: {same[(N, schedule)]} (all five cases: {all(same.values())})")
    assert np.array_equal(out["status"], ref["status"]) and np.array_equal(out["iters"], ref["iters"])
    assert du <= 1e-9 and dx <= 1e-9
    if all(same.values()):
        assert same[(N, schedule)]


@pytest.mark.parametrize("N,schedule", [(10, "mixed"), (16, "double")])
def test_the_two_identities_on_the_gpu(torch_first, built_lib, N, schedule):
    """Against plain solves of the equivalent QPs (tests/test_ext_wrench_cpu.py has both on the twin): a constant vertical force is x0[12] + F / m, and a
    wrench without a yaw torque is the reference x_ref - D with pcom = x_ref[:, 3:6] passed.  2e-3 N and one check interval."""
    from g1_locomotion_amd import BatchMPC, _lib
    B = B16
    x0, xr, ft, ct = wt.batch(B, N, ew.batch_seed(N, schedule), schedule)
    p = ew.params(N)
    F = 25.0 * (np.arange(B) % 4 + 1) * (-1.0) ** np.arange(B)
    wg = np.zeros((B, N, 6)); wg[:, :, 5] = F[:, None]
    xg = x0.copy(); xg[:, 12] += F / p.mass
    ws = ew.draw(B, N, ew.wrench_seed(N)); ws[:, :, 2] = 0.0
    D = np.stack([ew.response(p, xr[b], ws[b]) for b in range(B)])
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH) as eng:
        ref_g = eng.solve(xg, xr, ft, ct)
        ref_s = eng.solve(x0, xr - D, ft, ct, pcom=np.ascontiguousarray(xr[:, :, 3:6]))
        eng.set_external_wrench(wg)
        out_g = eng.solve(x0, xr, ft, ct)
        eng.set_external_wrench(ws)
        out_s = eng.solve(x0, xr, ft, ct)
        assert eng.kernel_name() == f"wrench_f64_n{N}_ew"
    for what, out, ref, xshift in (("gravity", out_g, ref_g, None), ("reference shift", out_s, ref_s, D)):
        du = np.abs(out["u"] - ref["u"]).max()
        di = np.abs(out["iters"].astype(int) - ref["iters"].astype(int)).max()
        xr_ = ref["x"].copy()
        if xshift is not None:
            xr_[:, 1:] += xshift
        dx = np.abs(out["x"][:, :, :12] - xr_[:, :, :12]).max()
        print(f"N={N} {schedule} {what}: max |du| {du:.3e} N, max |d iters| {di}, max |dx| {dx:.3e}")
        assert np.array_equal(out["status"], ref["status"])
        assert du <= wt.TOL_TWIN_N and di <= p.check_every and dx <= 1e-5


@pytest.mark.parametrize("N", [10, 16])
def test_wrench_records_and_weights_combine(torch_first, built_lib, N):
    """All three on one handle, the setters in two orders: per QP against the twin with all three; clearing each leaves the others, and the kernel names follow."""
    from g1_locomotion_amd import BatchMPC
    from test_gpu_robots import _draw as robots_draw
    B = B16
    x0, xr, ft, ct = wt.batch(B, N, wt.batch_seed(N, "mixed"), "mixed")
    rec, rob, w = wt.draw(B, wt.weights_seed(N)), robots_draw(B, 3900 + N), ew.draw(B, N, ew.wrench_seed(N))
    with BatchMPC(horizon=N) as eng:
        eng.set_robots(rob); eng.set_weights(rec); eng.set_external_wrench(w)
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}_ew"
        eng.set_weights(None)
        no_wt = eng.solve(x0, xr, ft, ct, want_y=True)               # weights cleared: records and wrench stay
        assert eng.kernel_name() == f"wrench_f64_n{N}_ew"
        eng.set_external_wrench(None)
        rb_only = eng.solve(x0, xr, ft, ct, want_y=True)             # wrench cleared too: the records stay
        assert eng.kernel_name() == f"wrench_f64_n{N}_rb"
    with BatchMPC(horizon=N) as eng:
        eng.set_external_wrench(w); eng.set_weights(rec); eng.set_robots(rob)
        out2 = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}_ew"
        eng.set_robots(None)
        no_rb = eng.solve(x0, xr, ft, ct, want_y=True)               # records cleared: weights and wrench stay
        assert eng.kernel_name() == f"wrench_f64_n{N}_ew"
        eng.set_external_wrench(None)
        wt_only = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}_wt"
        eng.set_weights(None)
        eng.set_robots(rob)
        ref_rb = eng.solve(x0, xr, ft, ct, want_y=True)
    for k in KEYS:
        assert np.array_equal(out[k], out2[k]), k
        assert np.array_equal(rb_only[k], ref_rb[k]), k
    for b in range(B):
        ew.check_qp(out, b, N, ew.params(N, rob[b], rec[b]), x0, xr, ft, ct, w[b])
        ew.check_qp(no_wt, b, N, ew.params(N, rob[b]), x0, xr, ft, ct, w[b])
        ew.check_qp(no_rb, b, N, ew.params(N, None, rec[b]), x0, xr, ft, ct, w[b])
        wt.check_qp(wt_only, b, N, wt.params(N, rec[b]), x0, xr, ft, ct)


def test_a_qp_in_flight_is_pushed(torch_first, built_lib):
    """A QP without any stance contact: zero forces, SOLVED in 0 iterations, and x_out the ballistic roll-out under the wrench."""
    from g1_locomotion_amd import BatchMPC
    B, N = 4, 12
    x0, xr, ft, ct = wt.batch(B, N, 61, "mixed")
    ct[2] = 0
    w = ew.draw(B, N, 63)
    with BatchMPC(horizon=N) as eng:
        eng.set_external_wrench(w)
        out = eng.solve(x0, xr, ft, ct, want_y=True)
    p = ew.params(N)
    ref = ew.update(p, x0[2], xr[2], ft[2], ct[2], w[2])
    assert out["status"][2] == orc.STATUS_SOLVED and out["iters"][2] == 0 and np.all(out["u"][2] == 0.0) and np.all(out["y"][2] == 0.0)
    assert np.all(ref["u"] == 0.0)
    assert np.abs(out["x"][2] - ref["x"]).max() <= 1e-9, np.abs(out["x"][2] - ref["x"]).max()
    assert np.abs(ref["x"][1:] - orc.update(p, x0[2], xr[2], ft[2], ct[2])["x"][1:]).max() > 1e-3      # (the push shows)
    for b in (0, 1, 3):
        ew.check_qp(out, b, N, p, x0, xr, ft, ct, w[b])


def test_a_bad_device_wrench_stays_local_and_the_host_setter_names_it(torch_first, built_lib):
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, SrbdqpError, _lib
    B, N = B16, 12
    x0, xr, ft, ct = wt.batch(B, N, 41, "mixed")
    w = ew.draw(B, N, 43)
    bad = w.copy()
    bad[3, 7, 4] = np.nan
    bad[9, 11, 0] = np.inf
    with BatchMPC(horizon=N) as eng:
        plain = eng.solve(x0, xr, ft, ct)
        eng.set_external_wrench(torch.from_numpy(w).cuda())
        good = eng.solve(x0, xr, ft, ct, want_y=True)
        dev_bad = torch.from_numpy(bad).cuda()
        eng.set_external_wrench(dev_bad)
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        msg = _refusal(lambda: eng.set_external_wrench(bad))
        assert msg == (f"srbdqp error {_lib.E_INVALID}: srbdqp_set_external_wrench: the wrench at (qp 3, step 7, component 4) is invalid "
                       "(every value must be finite with |value| <= 1e6); the previous setting is kept"), msg
        again = eng.solve(x0, xr, ft, ct, want_y=True)               # the previous setting (the device array) was kept
    for b in range(B):
        if b in (3, 9):
            assert out["status"][b] == _lib.NUMERICAL and out["iters"][b] == 0, (b, out["status"][b])
            assert np.all(out["u"][b] == 0.0) and np.all(out["y"][b] == 0.0) and np.all(np.isfinite(out["x"][b]))
            zero = ew.update(ew.params(N), x0[b], xr[b], ft[b], np.zeros_like(ct[b]), np.zeros((N, 6)))   # the roll-out of zero forces and no wrench
            assert np.abs(out["x"][b] - zero["x"]).max() <= 1e-9
        else:
            for k in KEYS:
                assert np.array_equal(out[k][b], good[k][b]), (b, k)
    for k in KEYS:
        assert np.array_equal(again[k], out[k]), k
    assert plain["status"][3] != _lib.NUMERICAL


def test_the_host_setter_and_the_kernel_share_one_bound(torch_first, built_lib):
    """|value| <= SRBDQP_EXT_WRENCH_MAX = 1e6 on both sides: the bound itself passes both, the next double above it is refused by the host setter and ends
    the QP as SRBDQP_NUMERICAL in the kernel."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    B, N = 4, 4
    x0, xr, ft, ct = wt.batch(B, N, 51, "double")
    w = ew.draw(B, N, 53)
    w[1, 2, 3] = -1.0e6                      # at the bound: valid
    with BatchMPC(horizon=N) as eng:
        eng.set_external_wrench(w)
        bad = w.copy()
        bad[2, 1, 5] = np.nextafter(1.0e6, np.inf)
        bad[3, 3, 1] = -np.finfo(np.float64).max
        msg = _refusal(lambda: eng.set_external_wrench(bad))
        assert msg is not None and "the wrench at (qp 2, step 1, component 5) is invalid" in msg, msg
        msg = _refusal(lambda: eng.set_external_wrench(bad[3:]))
        assert msg is not None and "the wrench at (qp 0, step 3, component 1) is invalid" in msg, msg
        eng.set_external_wrench(torch.from_numpy(bad).cuda())
        out = eng.solve(x0, xr, ft, ct)
    assert out["status"].tolist()[2:] == [_lib.NUMERICAL, _lib.NUMERICAL] and np.all(out["u"][2:] == 0.0)
    assert all(s in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER) for s in out["status"][:2])


def test_schedule_hint_keeps_wrenches_by_qp_index(torch_first, built_lib):
    torch = torch_first
    from g1_locomotion_amd import BatchMPC
    B, N = 256, 10
    x0, xr, ft, ct = wt.batch(B, N, 31, "mixed")
    w = ew.draw(B, N, 33)
    t = _to_dev(torch, x0, xr, ft, ct)
    with BatchMPC(horizon=N) as eng:
        eng.set_external_wrench(w)
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
    """The ragged QPs, their wrench rows and the twin's solution of each (computed once, shared by the cases below)."""
    Nq, x0, xr, ft, ct = wt.ragged_inputs(RAGGED_B, RAGGED_HORIZONS, RAGGED_SEED)
    off = np.concatenate([[0], np.cumsum(Nq)])
    w = np.concatenate([ew.draw(1, int(Nq[b]), 5000 + b)[0] for b in range(RAGGED_B)])
    refs = [ew.update(ew.params(int(Nq[b])), x0[b], xr[off[b]:off[b + 1]], ft[off[b]:off[b + 1]], ct[off[b]:off[b + 1]], w[off[b]:off[b + 1]]) for b in range(RAGGED_B)]
    return Nq, x0, xr, ft, ct, w, off, refs


@pytest.mark.parametrize("defer", [False, True])
def test_ragged_wrenches_follow_the_callers_rows(torch_first, built_lib, ragged_case, defer):
    """Horizons {8, 12, 16}, the QPs shuffled across the buckets: QP b of the caller's order solves under the rows at its row offset (against the twin per QP),
    without and with SRBDQP_FLAG_DEFER_TAIL (the device setter: read in place, beside the deferred passes too), after the flush."""
    torch = torch_first
    from g1_locomotion_amd import RaggedMPC, _lib
    Nq, x0, xr, ft, ct, w, off, refs = ragged_case
    B, rows = RAGGED_B, int(off[-1])
    t = _to_dev(torch, x0, xr, ft, ct)
    rg = RaggedMPC(horizons=RAGGED_HORIZONS, flags=_lib.FLAG_DEFER_TAIL if defer else 0)
    try:
        keep = torch.from_numpy(w).cuda() if defer else w
        rg.set_external_wrench(keep)
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


def test_ragged_refusals(torch_first, built_lib, ragged_case):
    """While a wrench is set on a ragged object: the fp32 solves and a solve of more rows than set return SRBDQP_E_INVALID with a message (nothing is
    launched); a solve that fits and, after clearing, the fp32 solve are accepted.  Objects with an N = 24 or a live bucket refuse the setters, and the host
    setter names the first bad (row, component)."""
    from g1_locomotion_amd import RaggedMPC, _lib
    Nq, x0, xr, ft, ct, w, off, refs = ragged_case
    B, E = 6, f"srbdqp error {_lib.E_INVALID}: "
    rows = int(off[B])
    q = (Nq[:B], x0[:B], xr[:rows], ft[:rows], ct[:rows])
    rg = RaggedMPC(horizons=RAGGED_HORIZONS)
    try:
        rg.set_external_wrench(w[:rows])
        f32 = E + "fp32 ragged solve: refused while external wrenches are set (srbdqp_ragged_set_external_wrench): only the fp64 solves read them"
        assert _refusal(lambda: rg.solve_packed(*q, dtype=np.float32)) == f32
        rg.set_external_wrench(w[:rows - 1])
        assert _refusal(lambda: rg.solve_packed(*q)) == E + f"ragged solve of {rows} horizon rows with an external wrench for {rows - 1} set: every row needs its wrench"
        short = rg.solve_packed(Nq[:B - 1], x0[:B - 1], xr[:off[B - 1]], ft[:off[B - 1]], ct[:off[B - 1]])       # fits
        assert np.array_equal(short["status"], [refs[b]["status"] for b in range(B - 1)])
        bad = w[:rows].copy(); bad[5, 2] = np.nan
        msg = _refusal(lambda: rg.set_external_wrench(bad))
        assert msg == E + ("srbdqp_ragged_set_external_wrench: the wrench at (row 5, component 2) is invalid (every value must be finite with |value| <= 1e6); "
                           "the previous setting is kept"), msg
        rg.set_external_wrench(None)
        assert _refusal(lambda: rg.solve_packed(*q, dtype=np.float32)) is None
    finally:
        rg.close()
    for horizons, text in (((8, 24), "bucket N=24: an external wrench: not at N = 24"), ((3, 4), "SRBDQP_FLAG_ANY_HORIZON")):
        rg = RaggedMPC(horizons=horizons)
        try:
            for arg in (w[:8], torch_first.from_numpy(w[:8]).cuda()):
                msg = _refusal(lambda: rg.set_external_wrench(arg))
                assert msg is not None and text in msg, msg
            rg.set_external_wrench(None)
        finally:
            rg.close()


def test_refusals(torch_first, built_lib):
    """With the calls of tests/test_gpu_variant_refusals.py (B = 2, N = 4, full double support): every call without a form for a wrench handle carries the
    fixed text, and the handle solves again after clearing."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    from test_gpu_variant_refusals import TAIL as VT, _calls
    B, N = 2, 4
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=610 + N, schedule="double")
    w = ew.draw(B, N, 71)
    w_dev = torch.from_numpy(w).cuda()
    E = f"srbdqp error {_lib.E_INVALID}: "
    refused = ("srbdqp_solve_staged_f64", "srbdqp_update_f64", "srbdqp_prepare_staged_f64", "srbdqp_solve_prepared_f64", "srbdqp_solve_batch_f32",
               "srbdqp_solve_batch_device_f32", "srbdqp_assemble_f64", "srbdqp_assemble_wrench_f64", "srbdqp_set_contact_normals", "srbdqp_set_contact_normals_device")
    with BatchMPC(horizon=N) as eng:
        calls = _calls(torch, eng, N, ("srbdqp_set_robots", "srbdqp_set_robots_device", "srbdqp_set_weights", "srbdqp_set_weights_device"))
        eng.set_external_wrench(w)
        for name in ("srbdqp_solve_batch_f64", "srbdqp_solve_batch_device_f64"):
            assert _refusal(calls[name]) is None and eng.kernel_name() == "wrench_f64_n4_ew", name
        for name in refused:
            assert _refusal(calls[name]) == E + f"{name}: {EW_TAIL}", name
        for name in ("srbdqp_set_robots", "srbdqp_set_robots_device", "srbdqp_set_weights", "srbdqp_set_weights_device"):   # (set, then cleared again)
            assert _refusal(calls[name]) is None, name
        # B > length
        eng.set_external_wrench(w[:1])
        msg = _refusal(calls["srbdqp_solve_batch_f64"])
        assert msg == E + "solve of 2 QPs with an external wrench for 1 set (srbdqp_set_external_wrench): every QP needs its block", msg
        assert _refusal(calls["srbdqp_solve_batch_device_f64"]) == msg
        # the clearing calls, host and device form: a plain handle again
        eng.set_external_wrench(w_dev)
        eng.set_external_wrench(None)
        eng.set_external_wrench(w)
        eng.set_external_wrench(torch.empty((0, N, 6), dtype=torch.float64, device="cuda"))
        for name in ("srbdqp_solve_staged_f64", "srbdqp_solve_batch_f32", "srbdqp_assemble_wrench_f64", "srbdqp_set_contact_normals"):
            assert _refusal(calls[name]) is None, name
        # with normals set (the line above), the wrench setters are refused in the normals' words
        for fn, arg in (("srbdqp_set_external_wrench", w), ("srbdqp_set_external_wrench_device", w_dev)):
            assert _refusal(lambda: eng.set_external_wrench(arg)) == E + f"{fn}: {VT['normals']}"
        eng.set_external_wrench(None)                                # (clearing is accepted in every state)
    # an explicit presolved kernel
    for kern in (_lib.KERNEL_COMPACT, _lib.KERNEL_SPLIT, _lib.KERNEL_WAVE):
        with BatchMPC(horizon=N, kernel=kern) as eng:
            eng.set_external_wrench(w)
            msg = _refusal(lambda: eng.solve(x0, xr, ft, ct))
            assert msg is not None and "an external wrench (srbdqp_set_external_wrench) are read by the general kernel only" in msg, msg
            eng.set_external_wrench(None)
            assert _refusal(lambda: eng.solve(x0, xr, ft, ct)) is None
    # a live horizon, rank-aware steps, N = 24
    with BatchMPC(horizon=3) as eng:
        for fn, arg in (("srbdqp_set_external_wrench", w[:, :3]), ("srbdqp_set_external_wrench_device", torch.from_numpy(np.ascontiguousarray(w[:, :3])).cuda())):
            assert _refusal(lambda: eng.set_external_wrench(arg)) == E + f"{fn}: {VT['live']}"
    with BatchMPC(horizon=N, rank_aware=True) as eng:
        for fn, arg in (("srbdqp_set_external_wrench", w), ("srbdqp_set_external_wrench_device", w_dev)):
            assert _refusal(lambda: eng.set_external_wrench(arg)) == E + f"{fn}: {VT['rank_aware']}"
    with BatchMPC(horizon=24) as eng:
        w24 = ew.draw(B, 24, 72)
        for arg in (w24, torch.from_numpy(w24).cuda()):
            msg = _refusal(lambda: eng.set_external_wrench(arg))
            assert msg is not None and msg.startswith(E + "an external wrench: not at N = 24"), msg
        eng.set_external_wrench(None)


def test_mpc_update_with_an_external_wrench_is_the_batch_solve(torch_first, built_lib):
    from g1_locomotion_amd import MPC, BatchMPC
    N = 10
    x0, xr, ft, ct = wt.batch(1, N, ew.batch_seed(N, "mixed"), "mixed")
    w = ew.draw(1, N, ew.wrench_seed(N))
    with BatchMPC(horizon=N) as eng:
        eng.set_external_wrench(w)
        ref = eng.solve(x0, xr, ft, ct)
    assert ref["status"][0] == orc.STATUS_SOLVED
    mpc = MPC(horizon=N)
    try:
        mpc.init_matrices()
        mpc.x0 = x0[0].reshape(13, 1).copy()
        mpc.x_ref_hor = xr[0].copy()
        u0, x1 = mpc.update(ct[0], ft[0], None, external_wrench=w[0])
        with pytest.raises(ValueError, match="contact_normals and external_wrench together"):
            mpc.update(ct[0], ft[0], None, external_wrench=w[0], contact_normals=np.tile([0.0, 0.0, 1.0], (N, 4)))
        u0p, _ = mpc.update(ct[0], ft[0], None)                      # the wrench was for that call alone
    finally:
        mpc.close()
    assert np.array_equal(u0.reshape(-1), ref["u"][0, 0]) and np.array_equal(x1, ref["x"][0])
    assert np.abs(u0p - u0).max() > 1.0
