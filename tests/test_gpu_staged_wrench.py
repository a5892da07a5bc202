"""GPU tests of the external wrench of ONE CALL on the staged path (include/srbdqp.h srbdqp_stage_ext_wrench, srbdqp_solve_staged_wrench_f64,
srbdqp_update_wrench_f64): the general kernel's low-latency MODE 7 instantiation (wrench_f64_n<N>_lat_ew: N <= 10, B <= 8) and its batch instantiation over the
staging arrays (wrench_f64_n<N>_ew: N in {12, 16, 20}, or 8 < B <= 16).  What this suite shares with the normals' (tests/test_gpu_staged_normals.py) -- the
helpers and the body of every shared test -- is tests/staged_side.py, called here with the wrench's row; the twin, the bars (check_qp), the batches, the draw and
the seeds are those of tests/side_inputs.py; the engine keeps its default rho restart and the twin runs the same one."""
import numpy as np
import pytest

import side_inputs as si
import srbd_oracle as orc
import staged_side as ss
from gpu_helpers import torch_first  # noqa: F401  (the fixture)
from staged_side import WRENCH

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("schedule", si.SCHEDULES)
@pytest.mark.parametrize("N", ss.LOW_LATENCY_HORIZONS)
def test_the_low_latency_form_matches_the_twin(torch_first, built_lib, N, schedule):
    ss.low_latency_form_matches_the_twin(WRENCH, N, schedule)


@pytest.mark.parametrize("N,schedule", ss.WARM_CASES)
def test_a_warm_start_under_the_wrench(torch_first, built_lib, N, schedule):
    ss.warm_start_under_the_input(WRENCH, N, schedule)


@pytest.mark.parametrize("N,schedule,B", ss.BATCH_FORM_CASES)
def test_the_batch_form_over_the_staging_arrays(torch_first, built_lib, N, schedule, B):
    ss.batch_form_over_the_staging_arrays(WRENCH, N, schedule, B)


@pytest.mark.parametrize("N,schedule", ss.NEUTRAL_CASES)
def test_a_zero_wrench_is_the_plain_staged_call(torch_first, built_lib, N, schedule):
    ss.neutral_input_is_the_plain_staged_call(WRENCH, N, schedule)


def test_the_wrench_is_the_calls(torch_first, built_lib):
    ss.input_is_the_calls(WRENCH)


def test_refusals(torch_first, built_lib):
    ss.refusals(WRENCH)


def test_a_restart_pass_carries_the_wrench(torch_first, built_lib):
    """N = 4, full double support, QP 2 of the suite's batch: the twin runs past the restart mark of 55 iterations, so the staged call's host-driven loop
    starts a second pass -- which must solve under the same wrench.  Alone in a B = 1 call."""
    from g1_locomotion_amd import BatchMPC
    N = 4
    x0, xr, ft, ct, w = (v[2:3] for v in WRENCH.case(N, "double", 8))
    p = si.params(N)
    ref = si.twin(p, x0[0], xr[0], ft[0], ct[0], ext_wrench=w[0])
    assert ref["iters"] > 55 and ref["status"] == orc.STATUS_SOLVED, ref["iters"]
    with BatchMPC(horizon=N) as eng:
        out = ss.staged(WRENCH, eng, x0, xr, ft, ct, w)
        assert eng.kernel_name() == f"wrench_f64_n{N}_lat_ew"
    print(f"iters {int(out['iters'][0])} twin {ref['iters']}, |u - twin| {np.abs(out['u'][0] - ref['u']).max():.3e} N")
    si.check_qp(out, 0, N, p, ref, ct[0])


@pytest.mark.parametrize("value,qp,step,comp", [(np.nan, 0, 3, 1), (np.inf, 2, 0, 5), (2e6, 1, 9, 0)])
def test_a_bad_wrench_value_is_named_and_nothing_is_launched(torch_first, built_lib, value, qp, step, comp):
    N, B = 10, 3
    x0, xr, ft, ct, w = WRENCH.case(N, "mixed", B)
    w = w.copy()
    w[qp, step, comp] = value
    if qp < B - 1:
        w[B - 1, 0, 0] = -np.inf                                    # (a later bad value: the FIRST one is named)
    ss.bad_value_is_named(WRENCH, N, B, x0, xr, ft, ct, w, si.draw_wrench(B, N, 5), qp, f"the wrench at (qp {{qp}}, step {step}, component {comp})",
                        "every value must be finite with |value| <= 1e6", (orc.STATUS_SOLVED,))


@pytest.mark.parametrize("N,B", [(10, 4), (12, 2)])
def test_main_inputs_that_are_not_finite(torch_first, built_lib, N, B):
    """The contract of include/srbdqp.h under the wrench of the call, on both forms.  NaN in the foot position of a stance contact: status -1, u = y = 0,
    iters 0, and x_out FINITE, the roll-out of zero forces plus the wrench's response D, to 1e-9.  NaN in x0: status -1, u = y = 0, iters 0 or check_every; row 0
    of x_out is the caller's x0 and the other rows carry no meaning (the header: x_out is finite only where x0 is).  The clean QPs beside them meet the twin."""
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct, w = WRENCH.case(N, "mixed", B)
    p = si.params(N)
    x0, ft = x0.copy(), ft.copy()
    k0 = int(np.flatnonzero(ct[0].any(1))[0]); c0 = int(np.flatnonzero(ct[0, k0])[0])
    ft[0, k0, 3 * c0 + 1] = np.nan
    x0[1, 4] = np.nan
    with BatchMPC(horizon=N) as eng:
        out = ss.staged(WRENCH, eng, x0, xr, ft, ct, w)
    for b in (0, 1):
        assert out["status"][b] == orc.STATUS_NUMERICAL and np.all(out["u"][b] == 0.0) and np.all(out["y"][b] == 0.0), b
    assert out["iters"][0] == 0 and out["iters"][1] in (0, p.check_every), out["iters"]
    clean = si.batch(16, N, si.wrench_batch_seed(N, "mixed"), "mixed")
    free = si.twin(p, clean[0][0], xr[0], clean[2][0], np.zeros_like(ct[0]), ext_wrench=w[0])["x"]      # no stance contact: zero forces, the roll-out under the wrench
    assert np.all(np.isfinite(out["x"][0])) and np.abs(out["x"][0] - free).max() <= 1e-9, np.abs(out["x"][0] - free).max()
    assert np.array_equal(out["x"][1][0], x0[1], equal_nan=True)
    for b in range(2, B):
        si.check_qp(out, b, N, p, si.twin(p, x0[b], xr[b], ft[b], ct[b], ext_wrench=w[b]), ct[b])


def test_a_qp_in_flight_is_pushed(torch_first, built_lib):
    """A QP without any stance contact in a B = 4 call at N = 10: SOLVED, 0 iterations, u = y = 0, and x_out the ballistic roll-out under the wrench."""
    from g1_locomotion_amd import BatchMPC
    N, B = 10, 4
    x0, xr, ft, ct, w = WRENCH.case(N, "mixed", B)
    ct = ct.copy()
    ct[2] = 0
    p = si.params(N)
    with BatchMPC(horizon=N) as eng:
        out = ss.staged(WRENCH, eng, x0, xr, ft, ct, w)
        assert eng.kernel_name() == f"wrench_f64_n{N}_lat_ew"
    ref = si.twin(p, x0[2], xr[2], ft[2], ct[2], ext_wrench=w[2])
    assert out["status"][2] == orc.STATUS_SOLVED and out["iters"][2] == 0 and np.all(out["u"][2] == 0.0) and np.all(out["y"][2] == 0.0)
    assert np.abs(out["x"][2] - ref["x"]).max() <= 1e-9, np.abs(out["x"][2] - ref["x"]).max()
    assert np.abs(ref["x"][1:] - orc.update(p, x0[2], xr[2], ft[2], ct[2])["x"][1:]).max() > 1e-3      # (the push shows)
    for b in (0, 1, 3):
        si.check_qp(out, b, N, p, si.twin(p, x0[b], xr[b], ft[b], ct[b], ext_wrench=w[b]), ct[b])


def test_mpc_with_staged_wrench(torch_first, built_lib):
    """MPC(staged_wrench=True): update(external_wrench=) meets the twin's bars on u0 and x1, the update() behind it equals a fresh plain update, and contact
    normals beside the wrench still raise."""
    from g1_locomotion_amd import MPC
    N = 10
    x0, xr, ft, ct, w = WRENCH.case(N, "mixed", 1)
    p = si.params(N)
    ref = si.twin(p, x0[0], xr[0], ft[0], ct[0], ext_wrench=w[0])
    assert ref["status"] == orc.STATUS_SOLVED

    def fresh():
        m = MPC(horizon=N, staged_wrench=False)
        try:
            m.x0, m.x_ref_hor = x0[0].reshape(13, 1).copy(), xr[0].copy()
            return m.update(ct[0], ft[0], None)
        finally:
            m.close()
    u0f, x1f = fresh()
    mpc = MPC(horizon=N, staged_wrench=True)
    try:
        mpc.x0, mpc.x_ref_hor = x0[0].reshape(13, 1).copy(), xr[0].copy()
        u0, x1 = mpc.update(ct[0], ft[0], None, external_wrench=w[0])
        assert mpc._engine.kernel_name() == f"wrench_f64_n{N}_lat_ew" and mpc.status == orc.STATUS_SOLVED and abs(mpc.iters - ref["iters"]) <= p.check_every
        assert u0.shape == (12, 1) and x1.shape == (N + 1, 13)
        ss.check_primal(dict(u=mpc.u_opt[None], x=mpc.x_opt[None], status=[mpc.status], iters=[mpc.iters]), N, p, ref, ct[0])
        assert np.abs(u0.reshape(-1) - ref["u"][0]).max() <= si.TOL_TWIN_N and np.abs(x1 - ref["x"]).max() <= 1e-5
        with pytest.raises(ValueError, match="contact_normals and external_wrench together"):
            mpc.update(ct[0], ft[0], None, external_wrench=w[0], contact_normals=np.tile([0.0, 0.0, 1.0], (N, 4)))
        u0p, x1p = mpc.update(ct[0], ft[0], None)
    finally:
        mpc.close()
    assert np.array_equal(u0p, u0f) and np.array_equal(x1p, x1f)
    assert np.abs(u0p - u0).max() > 1.0
