"""GPU tests of what is particular to the external wrench (include/srbdqp.h srbdqp_set_external_wrench / _device, srbdqp_ragged_set_external_wrench /
_device): a known world-frame torque and force on the body per horizon step of every QP, on the general kernel's MODE = 7 instantiation
(srbdqp_wrench_ew_kernel).  What the wrench shares with the other per-QP side inputs -- parity per QP, the zero wrench, the combination with robot records and
cost weights, the schedule hint, the ragged rows, bad device values, the shared bound -- is in tests/test_gpu_side_inputs.py; the bars, the twin, the draw and
the seeds are described in tests/side_inputs.py.  B = 16 unless a test says otherwise."""
import numpy as np
import pytest

import side_inputs as si
import srbd_oracle as orc
from gpu_helpers import refusal as _refusal, torch_first  # noqa: F401  (torch_first: the fixture)
from test_gpu_side_inputs import NEUTRAL_CASES, check_neutral, check_parity

pytestmark = pytest.mark.gpu

B16 = si.B16


@pytest.mark.parametrize("schedule", si.SCHEDULES)
@pytest.mark.parametrize("N", si.HORIZONS)
def test_per_qp_wrenches_match_the_twin(torch_first, built_lib, N, schedule):
    """Measured on an MI355X: statuses and iteration counts equal the twin's in all 24 cases; worst |u - twin| 6e-9 N (N = 4), 1.2e-7 (8), 3.3e-7 (10), 3.0e-6 (12),
    5.8e-6 (16), 2.7e-5 N (20) against the bar of 2e-3 N, worst |x - twin| 5.6e-9, 9.1e-8, 3.2e-7, 9.1e-7, 3.0e-6 and 8.0e-6 against the bar of 1e-5.  The bar
    on x is what the refinement of x_q in MODE = 7 is for: without it the drawn torque's |q| of 1e6 - 1e7 left x up to 1.3e-4 from the
    twin at N >= 10, carried by the yaw rate."""
    check_parity(si.EXT_WRENCH, N, schedule)


@pytest.mark.parametrize("N,schedule", NEUTRAL_CASES)
def test_a_zero_wrench_equals_no_wrench(torch_first, built_lib, N, schedule):
    """x_ref - 0.0 and s + 0.0 are exact, so the results should be bit-identical: printed per case, and asserted where all five cases showed it."""
    check_neutral(si.EXT_WRENCH, N, schedule)


@pytest.mark.parametrize("N,schedule", [(10, "mixed"), (16, "double")])
def test_the_two_identities_on_the_gpu(torch_first, built_lib, N, schedule):
    """Against plain solves of the equivalent QPs (tests/test_ext_wrench_cpu.py has both on the twin): a constant vertical force is x0[12] + F / m, and a
    wrench without a yaw torque is the reference x_ref - D with pcom = x_ref[:, 3:6] passed.  2e-3 N and one check interval."""
    from g1_locomotion_amd import BatchMPC, _lib
    B = B16
    x0, xr, ft, ct = si.batch(B, N, si.wrench_batch_seed(N, schedule), schedule)
    p = si.params(N)
    F = 25.0 * (np.arange(B) % 4 + 1) * (-1.0) ** np.arange(B)
    wg = np.zeros((B, N, 6)); wg[:, :, 5] = F[:, None]
    xg = x0.copy(); xg[:, 12] += F / p.mass
    ws = si.draw_wrench(B, N, si.wrench_seed(N)); ws[:, :, 2] = 0.0
    D = np.stack([si.response(p, xr[b], ws[b]) for b in range(B)])
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
        assert du <= si.TOL_TWIN_N and di <= p.check_every and dx <= 1e-5


def test_a_qp_in_flight_is_pushed(torch_first, built_lib):
    """A QP without any stance contact: zero forces, SOLVED in 0 iterations, and x_out the ballistic roll-out under the wrench."""
    from g1_locomotion_amd import BatchMPC
    B, N = 4, 12
    x0, xr, ft, ct = si.batch(B, N, 61, "mixed")
    ct[2] = 0
    w = si.draw_wrench(B, N, 63)
    with BatchMPC(horizon=N) as eng:
        eng.set_external_wrench(w)
        out = eng.solve(x0, xr, ft, ct, want_y=True)
    p = si.params(N)
    ref = si.twin(p, x0[2], xr[2], ft[2], ct[2], ext_wrench=w[2])
    assert out["status"][2] == orc.STATUS_SOLVED and out["iters"][2] == 0 and np.all(out["u"][2] == 0.0) and np.all(out["y"][2] == 0.0)
    assert np.all(ref["u"] == 0.0)
    assert np.abs(out["x"][2] - ref["x"]).max() <= 1e-9, np.abs(out["x"][2] - ref["x"]).max()
    assert np.abs(ref["x"][1:] - orc.update(p, x0[2], xr[2], ft[2], ct[2])["x"][1:]).max() > 1e-3      # (the push shows)
    for b in (0, 1, 3):
        si.check_qp(out, b, N, p, si.twin(p, x0[b], xr[b], ft[b], ct[b], ext_wrench=w[b]), ct[b])


def test_ragged_refusals(torch_first, built_lib):
    """While a wrench is set on a ragged object: the fp32 solves and a solve of more rows than set return SRBDQP_E_INVALID with a message (nothing is
    launched); a solve that fits and, after clearing, the fp32 solve are accepted.  Objects with an N = 24 or a live bucket refuse the setters, and the host
    setter names the first bad (row, component)."""
    from g1_locomotion_amd import RaggedMPC, _lib
    Nq, x0, xr, ft, ct, w, off, refs, _ = si.ragged_case(si.EXT_WRENCH)
    B, E = 6, f"srbdqp error {_lib.E_INVALID}: "
    rows = int(off[B])
    q = (Nq[:B], x0[:B], xr[:rows], ft[:rows], ct[:rows])
    rg = RaggedMPC(horizons=si.RAGGED_HORIZONS)
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
    """What the table of tests/test_gpu_variant_refusals.py (its ext_wrench column and rows) cannot say, with its calls (B = 2, N = 4, full double support)."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    from test_gpu_variant_refusals import TAIL as VT, _calls
    B, N = 2, 4
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=610 + N, schedule="double")
    w = si.draw_wrench(B, N, 71)
    w_dev = torch.from_numpy(w).cuda()
    E = f"srbdqp error {_lib.E_INVALID}: "
    with BatchMPC(horizon=N) as eng:
        calls = _calls(torch, eng, N)
        # B > length
        eng.set_external_wrench(w[:1])
        msg = _refusal(calls["srbdqp_solve_batch_f64"])
        assert msg == E + "solve of 2 QPs with an external wrench for 1 set (srbdqp_set_external_wrench): every QP needs its block", msg
        assert _refusal(calls["srbdqp_solve_batch_device_f64"]) == msg
        # with normals set, the wrench setters are refused in the normals' words
        eng.set_external_wrench(None)
        assert _refusal(calls["srbdqp_set_contact_normals"]) is None
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
    # N = 24
    with BatchMPC(horizon=24) as eng:
        w24 = si.draw_wrench(B, 24, 72)
        for arg in (w24, torch.from_numpy(w24).cuda()):
            msg = _refusal(lambda: eng.set_external_wrench(arg))
            assert msg is not None and msg.startswith(E + "an external wrench: not at N = 24"), msg
        eng.set_external_wrench(None)


def test_mpc_update_with_an_external_wrench_is_the_batch_solve(torch_first, built_lib):
    from g1_locomotion_amd import MPC, BatchMPC
    N = 10
    x0, xr, ft, ct = si.batch(1, N, si.wrench_batch_seed(N, "mixed"), "mixed")
    w = si.draw_wrench(1, N, si.wrench_seed(N))
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
