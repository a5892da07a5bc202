"""GPU tests of the contact normals of ONE CALL on the staged path (include/srbdqp.h srbdqp_stage_contact_normals, srbdqp_solve_staged_normals_f64,
srbdqp_update_normals_f64): the general kernel's low-latency MODE 4 instantiation (wrench_f64_n<N>_lat_cn: N <= 10, B <= 8) and its batch instantiation over the
staging arrays (wrench_f64_n<N>_cn: N in {12, 16, 20}, or 8 < B <= 16).  The twin, the bars (check_qp), the batches, the draw and the seeds are those of
tests/side_inputs.py; the engine keeps its default rho restart and the twin runs the same one.

Observed on an MI355X (flat normals against the plain staged call, B = 4): see DESIGN.md section 13."""
import ctypes as C
import functools

import numpy as np
import pytest

import non_finite as nf
import side_inputs as si
import srbd_oracle as orc
from gpu_helpers import refusal as _refusal, torch_first  # noqa: F401  (torch_first: the fixture)

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = 12345.678, 777


def _fill(eng, x0, xr, ft, ct, nr=None):
    """B QPs (and their normals) into the first rows of the staging arrays -> (the arrays, B)."""
    st, B = eng.stage(), len(x0)
    st["x0"][:B], st["x_ref"][:B], st["foot"][:B], st["contact"][:B] = x0, xr, np.asarray(ft).reshape(B, eng.N, 12), np.asarray(ct) != 0
    if nr is not None:
        eng.stage_contact_normals()[:B] = nr
    return st, B


def _out(st, B):
    return {k: st[k][:B].copy() for k in si.KEYS}


def staged_normals(eng, x0, xr, ft, ct, nr, want_y=True):
    """srbdqp_solve_staged_normals_f64 of the B QPs on their normals -> dict(u, x, y, status, iters), copies."""
    st, B = _fill(eng, x0, xr, ft, ct, nr)
    eng.solve_staged_normals(B, want_x=True, want_y=want_y)
    return _out(st, B)


def staged_plain(eng, x0, xr, ft, ct, want_y=True):
    st, B = _fill(eng, x0, xr, ft, ct)
    eng.solve_staged(B, want_x=True, want_y=want_y)
    return _out(st, B)


def update_normals(eng, x0, xr, ft, ct, nr):
    """srbdqp_update_normals_f64 of ONE QP from the caller's own arrays into the caller's own outputs -> (rc, dict(u, x, status, iters) with a leading axis of 1)."""
    N = eng.N
    a = [np.ascontiguousarray(v, np.float64) for v in (x0, xr, ft)] + [np.ascontiguousarray(np.asarray(ct) != 0, np.uint8), np.ascontiguousarray(nr, np.float64)]
    u0, u, x = np.full(12, SENTINEL), np.full((N, 12), SENTINEL), np.full((N + 1, 13), SENTINEL)
    status, iters = np.full(1, ISENTINEL, np.int32), np.full(1, ISENTINEL, np.int32)
    P = lambda v: v.ctypes.data_as(C.c_void_p)
    rc = eng._lib.srbdqp_update_normals_f64(eng._h, P(a[0]), P(a[1]), P(a[2]), P(a[3]), None, P(a[4]), P(u0), P(u), P(x), P(status), P(iters))
    if rc == 0:
        assert np.array_equal(u0, u[0])
    return rc, dict(u=u[None], x=x[None], status=status, iters=iters)


def update_plain(eng, x0, xr, ft, ct):
    N = eng.N
    a = [np.ascontiguousarray(v, np.float64) for v in (x0, xr, ft)] + [np.ascontiguousarray(np.asarray(ct) != 0, np.uint8)]
    u0, u, x = np.empty(12), np.empty((N, 12)), np.empty((N + 1, 13))
    status, iters = np.zeros(1, np.int32), np.zeros(1, np.int32)
    P = lambda v: v.ctypes.data_as(C.c_void_p)
    eng._check(eng._lib.srbdqp_update_f64(eng._h, P(a[0]), P(a[1]), P(a[2]), P(a[3]), None, P(u0), P(u), P(x), P(status), P(iters)))
    return dict(u=u[None], x=x[None], status=status, iters=iters)


def check_primal(out, N, p, ref, contact):
    """check_qp's bars on what srbdqp_update_normals_f64 returns -- it has no y_out, so the bars on the duals (the KKT residuals, the zero rows) are the staged
    call's alone: same status, iterations within one check interval, 2e-3 N from the twin, 1e-5 on x, the distance from the exact optimum, swing forces 0."""
    assert out["status"][0] == ref["status"] and ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER), (out["status"][0], ref["status"])
    assert abs(int(out["iters"][0]) - ref["iters"]) <= p.check_every, (out["iters"][0], ref["iters"])
    assert np.abs(out["u"][0] - ref["u"]).max() <= si.TOL_TWIN_N, np.abs(out["u"][0] - ref["u"]).max()
    assert np.abs(out["x"][0] - ref["x"]).max() <= 1e-5, np.abs(out["x"][0] - ref["x"]).max()
    _, vi, _ = orc.presolve(ref["qp_loc"], contact)
    s = p.force_scale
    if ref["status"] == orc.STATUS_SOLVED:
        xs, _ = orc.solve_reference(p, ref["qp_loc"])
        twin_gap = np.abs(ref["u_loc"] - xs).max() * s
        assert np.abs(si._local(ref["T"], out["u"][0]) / s - xs).max() * s <= max(si.TOL_EXACT_N, twin_gap + si.TOL_TWIN_N)
    assert np.all(out["u"][0].reshape(-1)[np.setdiff1d(np.arange(12 * N), vi)] == 0.0)


@functools.lru_cache(maxsize=None)
def _case(N, schedule):
    """The first 8 QPs of the normals suite's batch with their drawn normals, and the twin of each on its normals (computed once, shared, left unchanged)."""
    x0, xr, ft, ct, nr = si._normals_case(8, N, schedule)
    p = si.params(N)
    refs = tuple(si.twin(p, x0[b], xr[b], ft[b], ct[b], normals=nr[b]) for b in range(8))
    return x0, xr, ft, ct, nr, p, refs


# the one QP of the 96 that the twin solves at exactly iteration 250 = max_iter: its status may legitimately read MAX_ITER on the hardware, so it alone is held to
# the forces and the roll-out
AT_THE_CAP = (10, "single", 3)


@pytest.mark.parametrize("schedule", si.SCHEDULES)
@pytest.mark.parametrize("N", (4, 8, 10))
def test_the_low_latency_form_matches_the_twin(torch_first, built_lib, N, schedule):
    """8 QPs of the normals suite's batch in ONE staged call of B = 8, each against the twin run on its normals.  Several pass the restart mark of 55 (N = 8
    double QP 1: 90; N = 8 three QP 5: 170; N = 10 double QP 0: 70), so the host-driven restart pass runs under the normals too."""
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct, nr, p, refs = _case(N, schedule)
    with BatchMPC(horizon=N) as eng:
        out = staged_normals(eng, x0, xr, ft, ct, nr)
        assert eng.kernel_name() == f"wrench_f64_n{N}_lat_cn"
    du = max(np.abs(out["u"][b] - refs[b]["u"]).max() for b in range(8))
    dx = max(np.abs(out["x"][b] - refs[b]["x"]).max() for b in range(8))
    print(f"N={N} {schedule}: max |u - twin| {du:.3e} N, max |x - twin| {dx:.3e}, iters {out['iters'].tolist()} twin {[r['iters'] for r in refs]}")
    assert all(r["status"] == orc.STATUS_SOLVED for r in refs)
    for b in range(8):
        if (N, schedule, b) == AT_THE_CAP:
            assert refs[b]["iters"] == p.max_iter
            assert np.abs(out["u"][b] - refs[b]["u"]).max() <= si.TOL_TWIN_N and np.abs(out["x"][b] - refs[b]["x"]).max() <= 1e-5
            continue
        si.check_qp(out, b, N, p, refs[b], ct[b])


@pytest.mark.parametrize("N,schedule,b", [(10, "double", 0), (10, "double", 1), (8, "three", 5)])
def test_one_qp_in_the_argument_segment(torch_first, built_lib, N, schedule, b):
    """srbdqp_update_normals_f64 of one QP, inputs and normals in the kernel-argument segment: twin iterations 70, 55 and 170 -- the restart passes, which
    run the grid form on the same normals, included."""
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct, nr, p, refs = _case(N, schedule)
    with BatchMPC(horizon=N) as eng:
        rc, one = update_normals(eng, x0[b], xr[b], ft[b], ct[b], nr[b])
        assert rc == 0 and eng.kernel_name() == f"wrench_f64_n{N}_lat_cn"
    print(f"N={N} {schedule} QP {b}: |u - twin| {np.abs(one['u'][0] - refs[b]['u']).max():.3e} N, iters {int(one['iters'][0])} twin {refs[b]['iters']}")
    check_primal(one, N, p, refs[b], ct[b])


@pytest.mark.parametrize("N,schedule", [(4, "double"), (8, "mixed"), (10, "mixed")])
def test_a_warm_start_under_the_normals(torch_first, built_lib, N, schedule):
    """use_warm = 1 with the twin's own solution as warm_u (world frame, newtons) and warm_y, against the twin started from the same point: the world -> local
    conversion of the start.  B = 4, the bars of check_qp."""
    from g1_locomotion_amd import BatchMPC
    B = 4
    x0, xr, ft, ct, nr, p, refs = _case(N, schedule)
    wu = np.stack([refs[b]["u"].reshape(-1) for b in range(B)])
    wy = np.stack([refs[b]["y"] for b in range(B)])
    with BatchMPC(horizon=N) as eng:
        st, _ = _fill(eng, x0[:B], xr[:B], ft[:B], ct[:B], nr[:B])
        st["warm_u"][:B], st["warm_y"][:B] = wu, wy
        eng.solve_staged_normals(B, use_warm=True, want_x=True, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}_lat_cn"
        out = _out(st, B)
    warm = [si.twin(p, x0[b], xr[b], ft[b], ct[b], normals=nr[b], warm=(wu[b] / p.force_scale, wy[b])) for b in range(B)]
    print(f"N={N} {schedule}: iters warm {out['iters'].tolist()} twin warm {[r['iters'] for r in warm]} twin cold {[refs[b]['iters'] for b in range(B)]}")
    for b in range(B):
        si.check_qp(out, b, N, p, warm[b], ct[b])


@pytest.mark.parametrize("N,schedule,B", [(12, "mixed", 4), (16, "mixed", 4), (20, "mixed", 4), (10, "double", 16)])
def test_the_batch_form_over_the_staging_arrays(torch_first, built_lib, N, schedule, B):
    """The long horizons, and more QPs than the low-latency form takes: the batch instantiation _cn reads the staged normals array, with the completion word.
    (N = 20 QPs 1 and 2 pass that horizon's restart mark of 125.)"""
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct, nr = si._normals_case(B, N, schedule)
    p = si.params(N)
    with BatchMPC(horizon=N) as eng:
        out = staged_normals(eng, x0, xr, ft, ct, nr)
        assert eng.kernel_name() == f"wrench_f64_n{N}_cn"
    for b in range(B):
        si.check_qp(out, b, N, p, si.twin(p, x0[b], xr[b], ft[b], ct[b], normals=nr[b]), ct[b])


def test_the_cone_reaches_the_kernel(torch_first, built_lib):
    """The feet either side of a 0.6 rad ridge, N = 10, full double support, B = 8: the staged solution stays inside the true friction pyramids to 1e-3 N, the
    plain staged solve of the same QPs leaves them by more than 1 N in every QP (the twin: 2.2 - 10.7 N)."""
    from g1_locomotion_amd import BatchMPC
    N, B = 10, 8
    x0, xr, ft, ct = si.batch(B, N, 4210, "double")
    nr = si.ridge_normals(B, N)
    p = si.params(N)
    with BatchMPC(horizon=N) as eng:
        out = staged_normals(eng, x0, xr, ft, ct, nr)
        assert eng.kernel_name() == f"wrench_f64_n{N}_lat_cn"
        flat = staged_plain(eng, x0, xr, ft, ct)
    T = si.frames_matrix(nr[0])                                       # (one ridge for every QP)
    for b in range(B):
        qp = orc.build_qp(p, x0[b], xr[b], ft[b], ct[b], None)
        inside, outside = si.cone_violation(p, qp, T, out["u"][b]) * p.force_scale, si.cone_violation(p, qp, T, flat["u"][b]) * p.force_scale
        print(f"QP {b}: status {out['status'][b]}, leaves the pyramids by {inside:.2e} N; the flat plan by {outside:.2f} N")
        assert out["status"][b] == orc.STATUS_SOLVED and inside < 1e-3, (b, inside)
        assert outside > 1.0, (b, outside)


@pytest.mark.parametrize("N,schedule", [(10, "mixed"), (10, "double"), (4, "single")])
def test_flat_normals_are_the_plain_staged_call_to_rounding(torch_first, built_lib, N, schedule):
    """(0, 0, 1) everywhere against srbdqp_solve_staged_f64 on the same handle and inputs, B = 4, by the project's bars for the batch form (si.NORMALS); the
    largest differences are printed."""
    from g1_locomotion_amd import BatchMPC
    B = 4
    x0, xr, ft, ct, _ = si._normals_case(B, N, schedule)
    with BatchMPC(horizon=N) as eng:
        ref = staged_plain(eng, x0, xr, ft, ct)
        plain_kernel = eng.kernel_name()
        out = staged_normals(eng, x0, xr, ft, ct, si.flat_normals(B, N))
        assert eng.kernel_name() == f"wrench_f64_n{N}_lat_cn"
    d = {k: np.abs(out[k].astype(float) - ref[k].astype(float)).max() for k in si.KEYS}
    print(f"N={N} {schedule}: plain call on {plain_kernel}; max |du| {d['u']:.3e} N, |dx| {d['x']:.3e}, |dy| {d['y']:.3e}, |d iters| {int(d['iters'])}")
    assert np.array_equal(out["status"], ref["status"])
    assert d["iters"] <= si.NORMALS.neutral_iters and d["u"] <= si.NORMALS.neutral_tol, d


def test_the_normals_are_the_calls(torch_first, built_lib):
    """Plain update, normals update, plain update, three rounds on one handle: the two plain results of a round are bit-equal -- nothing was set and nothing had
    to be cleared -- and the ridge moved the forces by more than 1 N.  A block of the staging array nobody wrote acts as flat ground."""
    from g1_locomotion_amd import BatchMPC
    N = 10
    x0, xr, ft, ct = si.batch(3, N, 4210, "double")
    nr = si.ridge_normals(3, N)
    with BatchMPC(horizon=N) as eng:
        assert np.array_equal(eng.stage_contact_normals(), si.flat_normals(eng.stage()["capacity"], N))
        for r in range(3):
            a = update_plain(eng, x0[r], xr[r], ft[r], ct[r])
            ka = eng.kernel_name()
            rc, m = update_normals(eng, x0[r], xr[r], ft[r], ct[r], nr[r])
            assert rc == 0 and eng.kernel_name() == f"wrench_f64_n{N}_lat_cn"
            b = update_plain(eng, x0[r], xr[r], ft[r], ct[r])
            assert eng.kernel_name() == ka
            assert all(np.array_equal(a[k], b[k]) for k in ("u", "x", "status", "iters")), r
            assert np.abs(m["u"] - a["u"]).max() > 1.0, r
        # blocks 1 and 2 were never written (update writes block 0): a B = 3 call solves QPs 1 and 2 on flat ground
        assert np.array_equal(eng.stage_contact_normals()[1:3], si.flat_normals(2, N))
        mixed = staged_normals(eng, x0, xr, ft, ct, None)
        eng.stage_contact_normals()[0] = si.flat_normals(1, N)[0]
        flat = staged_normals(eng, x0, xr, ft, ct, None)
        assert all(np.array_equal(mixed[k][1:], flat[k][1:]) for k in si.KEYS)
        assert np.abs(mixed["u"][0] - flat["u"][0]).max() > 1.0
        plain = staged_plain(eng, x0, xr, ft, ct)
        assert np.array_equal(flat["status"], plain["status"]) and np.abs(flat["u"] - plain["u"]).max() <= si.NORMALS.neutral_tol


def test_refusals(torch_first, built_lib):
    """Every handle of the header's list refuses the two solve calls with SRBDQP_E_INVALID and a message that names the reason, and leaves the outputs alone;
    the staging array itself is handed out on any handle."""
    from g1_locomotion_amd import BatchMPC, _lib
    from g1_locomotion_amd.mpc import robots_array, weights_array
    from test_gpu_variant_refusals import TAIL
    N, E = 4, f"srbdqp error {_lib.E_INVALID}: "
    x0, xr, ft, ct, nr = si._normals_case(1, N, "double")
    outs = []

    def upd(eng, q, n):
        rc, one = update_normals(eng, q[0][0], q[1][0], q[2][0], q[3][0], n[0])
        outs.append(one)
        eng._check(rc)
    calls = {"srbdqp_solve_staged_normals_f64": lambda eng: eng.solve_staged_normals(1),
             "srbdqp_update_normals_f64": lambda eng: upd(eng, (x0, xr, ft, ct), nr)}

    def refused(eng, call):
        st = eng.stage()
        for k in ("u", "x", "y"):
            st[k][:] = SENTINEL
        st["status"][:], st["iters"][:] = ISENTINEL, ISENTINEL
        del outs[:]
        msg = _refusal(lambda: call(eng))
        assert all(np.all(st[k] == SENTINEL) for k in ("u", "x", "y")) and np.all(st["status"] == ISENTINEL) and np.all(st["iters"] == ISENTINEL)
        assert all(np.all(o["u"] == SENTINEL) and np.all(o["x"] == SENTINEL) and o["status"][0] == ISENTINEL for o in outs)
        return msg
    sides = dict(robots=lambda e: e.set_robots(robots_array(1)), weights=lambda e: e.set_weights(weights_array(1)),
                 normals=lambda e: e.set_contact_normals(si.flat_normals(1, N)), ext_wrench=lambda e: e.set_external_wrench(si.draw_wrench(1, N, 3)))
    for name, setit in sides.items():
        with BatchMPC(horizon=N) as eng:
            _fill(eng, x0, xr, ft, ct, nr)
            setit(eng)
            for fn, call in calls.items():
                assert refused(eng, call) == E + f"{fn}: {TAIL[name]}", (name, fn)
    with BatchMPC(horizon=N, rank_aware=True) as eng:
        for fn, call in calls.items():
            assert refused(eng, call) == E + f"{fn}: {TAIL['rank_aware']}", fn

    def other(Nh, seed):                                             # the same two calls on a QP of another horizon
        q = orc.synthetic_batch(1, Nh, seed=seed, schedule="double")
        nq = si.flat_normals(1, Nh)
        return {"srbdqp_solve_staged_normals_f64": lambda eng: eng.solve_staged_normals(1),
                "srbdqp_update_normals_f64": lambda eng: upd(eng, q, nq)}
    with BatchMPC(horizon=3) as eng:                               # a live horizon (SRBDQP_FLAG_ANY_HORIZON)
        assert eng.stage_contact_normals().shape == (eng.stage()["capacity"], 3, 12)
        for fn, call in other(3, 31).items():
            assert refused(eng, call) == E + f"{fn}: {TAIL['live']}", fn
    with BatchMPC(horizon=24) as eng:
        for fn, call in other(24, 32).items():
            msg = refused(eng, call)
            assert msg is not None and msg.startswith(E + f"{fn}: contact normals: not at N = 24"), msg
    for kern in (_lib.KERNEL_COMPACT, _lib.KERNEL_SPLIT, _lib.KERNEL_WAVE):
        with BatchMPC(horizon=N, kernel=kern) as eng:
            for fn, call in calls.items():
                msg = refused(eng, call)
                assert msg is not None and msg.startswith(E + f"{fn}: contact normals") and "are read by the general kernel only" in msg, (kern, fn, msg)
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH) as eng:    # ... and the explicit general kernel is accepted
        assert staged_normals(eng, x0, xr, ft, ct, nr)["status"][0] == orc.STATUS_SOLVED


def _bad_nan(n):
    n[0] = np.nan


def _bad_zero(n):
    n[:] = 0.0


def _bad_steep(n):
    n[:] = (np.sqrt(1.0 - 0.09), 0.0, 0.3)


@pytest.mark.parametrize("spoil,why,qp,step,contact,swing", [(_bad_nan, "every entry must be finite", 0, 3, 1, False), (_bad_zero, "need 0.5 <= |n| <= 2", 2, 0, 3, True),
                                                             (_bad_steep, "need n_z >= 0.5 |n| (slopes to 60 degrees)", 1, 9, 0, True)])
def test_a_bad_normal_is_named_and_nothing_is_launched(torch_first, built_lib, spoil, why, qp, step, contact, swing):
    from g1_locomotion_amd import BatchMPC, _lib
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
    want = (f"srbdqp error {_lib.E_INVALID}: srbdqp_solve_staged_normals_f64: the normal of (qp {qp}, step {step}, contact {contact}) is invalid "
            f"({why}); nothing was launched")
    with BatchMPC(horizon=N) as eng:
        st, _ = _fill(eng, x0, xr, ft, ct, nr)
        for k in ("u", "x", "y"):
            st[k][:] = SENTINEL
        st["status"][:], st["iters"][:] = ISENTINEL, ISENTINEL
        assert _refusal(lambda: eng.solve_staged_normals(B, want_x=True, want_y=True)) == want
        assert all(np.all(st[k] == SENTINEL) for k in ("u", "x", "y")) and np.all(st["status"] == ISENTINEL) and np.all(st["iters"] == ISENTINEL)
        good = si._normals_case(B, N, "mixed")[4]
        eng.stage_contact_normals()[:B] = good                       # (a refused update leaves the staged normals array as it was: the caller's array is tested where it is)
        rc, one = update_normals(eng, x0[qp], xr[qp], ft[qp], ct[qp], nr[qp])
        assert np.array_equal(eng.stage_contact_normals()[:B], good)
        assert rc == _lib.E_INVALID and f"srbdqp_update_normals_f64: the normal of (qp 0, step {step}, contact {contact}) is invalid ({why})" in eng._lib.srbdqp_last_error(eng._h).decode()
        assert np.all(one["u"] == SENTINEL) and np.all(one["x"] == SENTINEL) and one["status"][0] == ISENTINEL
        assert all(np.all(st[k] == SENTINEL) for k in ("u", "x", "y")) and np.all(st["status"] == ISENTINEL)
        eng.solve_staged_normals(B)                                  # ... and the good normals on the same handle are solved
        assert np.all(np.isin(st["status"][:B], (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER)))


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
        clean = staged_normals(eng, x0, xr, ft, ct, nr)
        st = eng.stage()
        for k in ("u", "x", "y"):
            st[k][:] = SENTINEL
        st["status"][:], st["iters"][:] = ISENTINEL, ISENTINEL
        out = staged_normals(eng, d["x0"], xr, d["foot"], ct, nr)
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
    x0, xr, ft, ct, nr, p, refs = _case(N, "mixed")
    ref = refs[0]
    assert ref["status"] == orc.STATUS_SOLVED
    with BatchMPC(horizon=N) as eng:
        direct = staged_normals(eng, x0[:1], xr[:1], ft[:1], ct[:1], nr[:1])

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
        check_primal(dict(u=mpc.u_opt.reshape(1, N, 12), x=mpc.x_opt[None], status=[mpc.status], iters=[mpc.iters]), N, p, ref, ct[0])
        assert np.abs(mpc.u_opt.reshape(N, 12) - ud.reshape(N, 12)).max() <= si.TOL_TWIN_N and std == mpc.status
        with pytest.raises(ValueError, match="contact_normals and external_wrench together"):
            mpc.update(ct[0], ft[0].reshape(N, 12), None, external_wrench=np.zeros((N, 6)), contact_normals=nr[0])
        u0p, x1p = mpc.update(ct[0], ft[0].reshape(N, 12), None)
    finally:
        mpc.close()
    assert np.array_equal(u0p, u0f) and np.array_equal(x1p, x1f)
