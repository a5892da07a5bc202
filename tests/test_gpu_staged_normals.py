"""GPU tests of the contact normals of ONE CALL on the staged path (include/srbdqp.h srbdqp_stage_contact_normals, srbdqp_solve_staged_normals_f64,
srbdqp_update_normals_f64): the general kernel's low-latency MODE 4 instantiation (wrench_f64_n<N>_lat_cn: N <= 10, B <= 8) and its batch instantiation over the
staging arrays (wrench_f64_n<N>_cn: N in {12, 16, 20}, or 8 < B <= 16).  What this suite shares with the wrench's (tests/test_gpu_staged_wrench.py) -- the
helpers and the body of every shared test -- is tests/staged_side.py, called here with the normals' row; the twin, the bars (check_qp), the batches, the draw
and the seeds are those of tests/side_inputs.py; the engine keeps its default rho restart and the twin runs the same one.

Observed on an MI355X (flat normals against the plain staged call, B = 4): see DESIGN.md section 13."""
import numpy as np
import pytest

import non_finite as nf
import side_inputs as si
import srbd_oracle as orc
import staged_side as ss
from gpu_helpers import torch_first  # noqa: F401  (the fixture)
from staged_side import NORMALS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("schedule", si.SCHEDULES)
@pytest.mark.parametrize("N", ss.LOW_LATENCY_HORIZONS)
def test_the_low_latency_form_matches_the_twin(torch_first, built_lib, N, schedule):
    ss.low_latency_form_matches_the_twin(NORMALS, N, schedule)


@pytest.mark.parametrize("N,schedule", ss.WARM_CASES)
def test_a_warm_start_under_the_normals(torch_first, built_lib, N, schedule):
    ss.warm_start_under_the_input(NORMALS, N, schedule)


@pytest.mark.parametrize("N,schedule,B", ss.BATCH_FORM_CASES)
def test_the_batch_form_over_the_staging_arrays(torch_first, built_lib, N, schedule, B):
    ss.batch_form_over_the_staging_arrays(NORMALS, N, schedule, B)


@pytest.mark.parametrize("N,schedule", ss.NEUTRAL_CASES)
def test_flat_normals_are_the_plain_staged_call_to_rounding(torch_first, built_lib, N, schedule):
    ss.neutral_input_is_the_plain_staged_call(NORMALS, N, schedule)


def test_the_normals_are_the_calls(torch_first, built_lib):
    ss.input_is_the_calls(NORMALS)


def test_refusals(torch_first, built_lib):
    ss.refusals(NORMALS)


@pytest.mark.parametrize("N,schedule,b", [(10, "double", 0), (10, "double", 1), (8, "three", 5)])
def test_one_qp_in_the_argument_segment(torch_first, built_lib, N, schedule, b):
    """srbdqp_update_normals_f64 of one QP, inputs and normals in the kernel-argument segment: twin iterations 70, 55 and 170 -- the restart passes, which
    run the grid form on the same normals, included."""
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct, nr, p, refs = ss.suite8(NORMALS, N, schedule)
    with BatchMPC(horizon=N) as eng:
        rc, one = ss.update_side(NORMALS, eng, x0[b], xr[b], ft[b], ct[b], nr[b])
        assert rc == 0 and eng.kernel_name() == f"wrench_f64_n{N}_lat_cn"
    print(f"N={N} {schedule} QP {b}: |u - twin| {np.abs(one['u'][0] - refs[b]['u']).max():.3e} N, iters {int(one['iters'][0])} twin {refs[b]['iters']}")
    ss.check_primal(one, N, p, refs[b], ct[b])


def test_the_cone_reaches_the_kernel(torch_first, built_lib):
    """The feet either side of a 0.6 rad ridge, N = 10, full double support, B = 8: the staged solution stays inside the true friction pyramids to 1e-3 N, the
    plain staged solve of the same QPs leaves them by more than 1 N in every QP (the twin: 2.2 - 10.7 N)."""
    from g1_locomotion_amd import BatchMPC
    N, B = 10, 8
    x0, xr, ft, ct = si.batch(B, N, 4210, "double")
    nr = si.ridge_normals(B, N)
    p = si.params(N)
    with BatchMPC(horizon=N) as eng:
        out = ss.staged(NORMALS, eng, x0, xr, ft, ct, nr)
        assert eng.kernel_name() == f"wrench_f64_n{N}_lat_cn"
        flat = ss.staged_plain(eng, x0, xr, ft, ct)
    T = si.frames_matrix(nr[0])                                       # (one ridge for every QP)
    for b in range(B):
        qp = orc.build_qp(p, x0[b], xr[b], ft[b], ct[b], None)
        inside, outside = si.cone_violation(p, qp, T, out["u"][b]) * p.force_scale, si.cone_violation(p, qp, T, flat["u"][b]) * p.force_scale
        print(f"QP {b}: status {out['status'][b]}, leaves the pyramids by {inside:.2e} N; the flat plan by {outside:.2f} N")
        assert out["status"][b] == orc.STATUS_SOLVED and inside < 1e-3, (b, inside)
        assert outside > 1.0, (b, outside)


def _bad_nan(n):
    n[0] = np.nan


def _bad_zero(n):
    n[:] = 0.0


def _bad_steep(n):
    n[:] = (np.sqrt(1.0 - 0.09), 0.0, 0.3)


@pytest.mark.parametrize("spoil,why,qp,step,contact,swing", [(_bad_nan, "every entry must be finite", 0, 3, 1, False), (_bad_zero, "need 0.5 <= |n| <= 2", 2, 0, 3, True),
                                                             (_bad_steep, "need n_z >= 0.5 |n| (slopes to 60 degrees)", 1, 9, 0, True)])
def test_a_bad_normal_is_named_and_nothing_is_launched(torch_first, built_lib, spoil, why, qp, step, contact, swing):
    N, B = 10, 3
    x0, xr, ft, ct, nr = si._normals_case(B, N, "mixed")
    ct = ct.copy()
    ct[qp, step, contact] = 0 if swing else 1                       # (a swing contact's normal is held to the rules too)
    ct[qp, step, (contact + 1) % 4] = 1
    nr = nr.copy().reshape(B, N, 4, 3)
    spoil(nr[qp, step, contact])
    if qp < B - 1:
        nr[B - 1, 0, 0] = np.inf                                    # (a later bad normal: the FIRST one is named)
    nr = nr.reshape(B, N, 12)
    ss.bad_value_is_named(NORMALS, N, B, x0, xr, ft, ct, nr, si._normals_case(B, N, "mixed")[4], qp, f"the normal of (qp {{qp}}, step {step}, contact {contact})", why,
                        (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER))


@pytest.mark.parametrize("N,B", [(10, 4), (12, 2)])
def test_main_inputs_that_are_not_finite(torch_first, built_lib, N, B):
    """The contract of include/srbdqp.h (tests/non_finite.py check_contract) under the normals of the call, on both forms: NaN in x0 (QP 0), in the position of
    a stance foot (QP 1), and -- harmless -- of a swing foot (the last QP): the rejected QPs read status -1, u = y = 0, iters 0 or check_every, x the
    zero-force roll-out or, with a poisoned x0, that x0 in row 0; every other QP is the clean solve bit for bit."""
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct, nr = si._normals_case(B, N, "mixed")
    ft = ft.reshape(B, N, 12)
    p = si.params(N)
    stance = nf.ROW["foot_stance_ge3"] if nf.ROW["foot_stance_ge3"].index(N, ct[1]) is not None else nf.ROW["foot_stance_le2"]
    bad = {0: nf.ROW["x0_pos"], 1: stance}
    if nf.ROW["foot_swing"].index(N, ct[B - 1]) is not None and B - 1 not in bad:
        bad[B - 1] = nf.ROW["foot_swing"]
    d = dict(x0=x0.copy(), foot=ft.copy())
    for b, row in bad.items():
        d[row.array][(b,) + tuple(row.index(N, ct[b]))] = np.nan
    with BatchMPC(horizon=N) as eng:
        clean = ss.staged(NORMALS, eng, x0, xr, ft, ct, nr)
        ss.mark_outputs(eng.stage())
        out = ss.staged(NORMALS, eng, d["x0"], xr, d["foot"], ct, nr)
        assert eng.kernel_name() == (f"wrench_f64_n{N}_lat_cn" if N <= 10 else f"wrench_f64_n{N}_cn")
    zero_x = lambda b: orc.update(orc.params_for(N), x0[b], xr[b], ft[b], np.zeros_like(ct[b]))["x"]      # (no forces: the frames do not enter)
    seen = nf.check_contract(out, clean, bad, p, x0=d["x0"], zero_x=zero_x, tag=f"staged normals N={N}")
    print(f"N={N} B={B}: iters of the rejected QPs {seen}")
    assert set(seen) == {0, 1}


def test_mpc_with_staged_normals(torch_first, built_lib):
    """MPC(staged_normals=True).update(contact_normals=) equals solve_staged_normals on the same QP bit for bit, and the default-route MPC within 2e-3 N; the
    update() behind it equals a fresh plain update, and a wrench beside the normals still raises."""
    from g1_locomotion_amd import MPC, BatchMPC
    N = 10
    x0, xr, ft, ct, nr, p, refs = ss.suite8(NORMALS, N, "mixed")
    ref = refs[0]
    assert ref["status"] == orc.STATUS_SOLVED
    with BatchMPC(horizon=N) as eng:
        direct = ss.staged(NORMALS, eng, x0[:1], xr[:1], ft[:1], ct[:1], nr[:1])

    def run(update_kw, **mpc_kw):
        m = MPC(horizon=N, **mpc_kw)
        try:
            m.x0, m.x_ref_hor = x0[0].reshape(13, 1).copy(), xr[0].copy()
            u0, x1 = m.update(ct[0], ft[0].reshape(N, 12), None, **update_kw)
            return u0, x1, m.u_opt.copy(), m.x_opt.copy(), m.status, m.iters, m._engine.kernel_name()
        finally:
            m.close()
    u0f, x1f = run({})[:2]
    u0d, x1d, ud, xd, std, itd, kd = run(dict(contact_normals=nr[0]))
    assert kd == f"wrench_f64_n{N}_cn"
    mpc = MPC(horizon=N, staged_normals=True)
    try:
        mpc.x0, mpc.x_ref_hor = x0[0].reshape(13, 1).copy(), xr[0].copy()
        for form in (nr[0], nr[0].reshape(N, 4, 3), [r.reshape(4, 3) for r in nr[0]]):
            u0, x1 = mpc.update(ct[0], ft[0].reshape(N, 12), None, contact_normals=form)
            assert mpc._engine.kernel_name() == f"wrench_f64_n{N}_lat_cn" and mpc.status == orc.STATUS_SOLVED
            assert u0.shape == (12, 1) and x1.shape == (N + 1, 13)
            assert np.array_equal(mpc.u_opt.reshape(N, 12), direct["u"][0]) and np.array_equal(x1, direct["x"][0]) and mpc.iters == direct["iters"][0]
            assert np.array_equal(u0.reshape(-1), direct["u"][0][0])
        ss.check_primal(dict(u=mpc.u_opt.reshape(1, N, 12), x=mpc.x_opt[None], status=[mpc.status], iters=[mpc.iters]), N, p, ref, ct[0])
        assert np.abs(mpc.u_opt.reshape(N, 12) - ud.reshape(N, 12)).max() <= si.TOL_TWIN_N and std == mpc.status
        with pytest.raises(ValueError, match="contact_normals and external_wrench together"):
            mpc.update(ct[0], ft[0].reshape(N, 12), None, external_wrench=np.zeros((N, 6)), contact_normals=nr[0])
        u0p, x1p = mpc.update(ct[0], ft[0].reshape(N, 12), None)
    finally:
        mpc.close()
    assert np.array_equal(u0p, u0f) and np.array_equal(x1p, x1f)
