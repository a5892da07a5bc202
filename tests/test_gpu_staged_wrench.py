"""GPU tests of the external wrench of ONE CALL on the staged path (include/srbdqp.h srbdqp_stage_ext_wrench, srbdqp_solve_staged_wrench_f64,
srbdqp_update_wrench_f64): the general kernel's low-latency MODE 7 instantiation (wrench_f64_n<N>_lat_ew: N <= 10, B <= 8) and its batch instantiation over the
staging arrays (wrench_f64_n<N>_ew: N in {12, 16, 20}, or 8 < B <= 16).  The twin, the bars (check_qp), the batches, the draw and the seeds are those of
tests/side_inputs.py; the engine keeps its default rho restart and the twin runs the same one."""
import ctypes as C

import numpy as np
import pytest

import side_inputs as si
import srbd_oracle as orc
from gpu_helpers import refusal as _refusal, torch_first  # noqa: F401  (torch_first: the fixture)

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = 12345.678, 777


def _fill(eng, x0, xr, ft, ct, w=None):
    """B QPs (and their wrenches) into the first rows of the staging arrays -> (the arrays, B)."""
    st, B = eng.stage(), len(x0)
    st["x0"][:B], st["x_ref"][:B], st["foot"][:B], st["contact"][:B] = x0, xr, ft, np.asarray(ct) != 0
    if w is not None:
        eng.stage_ext_wrench()[:B] = w
    return st, B


def _out(st, B):
    return {k: st[k][:B].copy() for k in si.KEYS}


def staged_wrench(eng, x0, xr, ft, ct, w, want_y=True):
    """srbdqp_solve_staged_wrench_f64 of the B QPs under their wrenches -> dict(u, x, y, status, iters), copies."""
    st, B = _fill(eng, x0, xr, ft, ct, w)
    eng.solve_staged_wrench(B, want_x=True, want_y=want_y)
    return _out(st, B)


def staged_plain(eng, x0, xr, ft, ct, want_y=True):
    st, B = _fill(eng, x0, xr, ft, ct)
    eng.solve_staged(B, want_x=True, want_y=want_y)
    return _out(st, B)


def update_wrench(eng, x0, xr, ft, ct, w):
    """srbdqp_update_wrench_f64 of ONE QP from the caller's own arrays into the caller's own outputs -> (rc, dict(u, x, status, iters) with a leading axis of 1)."""
    N = eng.N
    a = [np.ascontiguousarray(v, np.float64) for v in (x0, xr, ft)] + [np.ascontiguousarray(np.asarray(ct) != 0, np.uint8), np.ascontiguousarray(w, np.float64)]
    u0, u, x = np.full(12, SENTINEL), np.full((N, 12), SENTINEL), np.full((N + 1, 13), SENTINEL)
    status, iters = np.full(1, ISENTINEL, np.int32), np.full(1, ISENTINEL, np.int32)
    P = lambda v: v.ctypes.data_as(C.c_void_p)
    rc = eng._lib.srbdqp_update_wrench_f64(eng._h, P(a[0]), P(a[1]), P(a[2]), P(a[3]), None, P(a[4]), P(u0), P(u), P(x), P(status), P(iters))
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
    """check_qp's bars on what srbdqp_update_wrench_f64 returns -- it has no y_out, so the bars on the duals (the KKT residuals, the zero rows) are the staged
    call's alone: same status, iterations within one check interval, 2e-3 N from the twin, 1e-5 on x, the distance from the exact optimum, swing forces 0."""
    assert out["status"][0] == ref["status"] and ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER), (out["status"][0], ref["status"])
    assert abs(int(out["iters"][0]) - ref["iters"]) <= p.check_every, (out["iters"][0], ref["iters"])
    assert np.abs(out["u"][0] - ref["u"]).max() <= si.TOL_TWIN_N, np.abs(out["u"][0] - ref["u"]).max()
    assert np.abs(out["x"][0] - ref["x"]).max() <= 1e-5, np.abs(out["x"][0] - ref["x"]).max()
    _, vi, _ = orc.presolve(ref["qp_loc"], contact)
    if ref["status"] == orc.STATUS_SOLVED:
        xs, _ = orc.solve_reference(p, ref["qp_loc"])
        s = p.force_scale
        twin_gap = np.abs(ref["u_loc"] - xs).max() * s
        assert np.abs(out["u"][0].reshape(-1) / s - xs).max() * s <= max(si.TOL_EXACT_N, twin_gap + si.TOL_TWIN_N)
    assert np.all(out["u"][0].reshape(-1)[np.setdiff1d(np.arange(12 * N), vi)] == 0.0)


def _case(N, schedule, B):
    x0, xr, ft, ct = si.batch(16, N, si.wrench_batch_seed(N, schedule), schedule)
    w = si.draw_wrench(16, N, si.wrench_seed(N))
    return x0[:B], xr[:B], ft[:B], ct[:B], w[:B]


@pytest.mark.parametrize("schedule", si.SCHEDULES)
@pytest.mark.parametrize("N", (4, 8, 10))
def test_the_low_latency_form_matches_the_twin(torch_first, built_lib, N, schedule):
    """The first 8 QPs of the wrench suite's batch in ONE staged call of B = 8, each against the twin run under its wrench; QP 0 once more, alone, through
    srbdqp_update_wrench_f64 (inputs and wrench in the kernel-argument segment).  No QP is left out: none whose twin count is the restart mark differed on
    the hardware."""
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct, w = _case(N, schedule, 8)
    p = si.params(N)
    with BatchMPC(horizon=N) as eng:
        out = staged_wrench(eng, x0, xr, ft, ct, w)
        assert eng.kernel_name() == f"wrench_f64_n{N}_lat_ew"
        rc, one = update_wrench(eng, x0[0], xr[0], ft[0], ct[0], w[0])
        assert rc == 0 and eng.kernel_name() == f"wrench_f64_n{N}_lat_ew"
    refs = [si.twin(p, x0[b], xr[b], ft[b], ct[b], ext_wrench=w[b]) for b in range(8)]
    du = max(np.abs(out["u"][b] - refs[b]["u"]).max() for b in range(8))
    dx = max(np.abs(out["x"][b] - refs[b]["x"]).max() for b in range(8))
    print(f"N={N} {schedule}: max |u - twin| {du:.3e} N, max |x - twin| {dx:.3e}, iters {out['iters'].tolist()} twin {[r['iters'] for r in refs]}; "
          f"update: |u - twin| {np.abs(one['u'][0] - refs[0]['u']).max():.3e} N, iters {int(one['iters'][0])}")
    for b in range(8):
        si.check_qp(out, b, N, p, refs[b], ct[b])
    check_primal(one, N, p, refs[0], ct[0])


@pytest.mark.parametrize("N,schedule", [(4, "double"), (8, "mixed"), (10, "mixed")])
def test_a_warm_start_under_the_wrench(torch_first, built_lib, N, schedule):
    """use_warm = 1: the caller's start -- 20 N on every normal force, zero duals -- against the twin started from the same point (P x^0 goes through the
    G'v tables, whose layout over the threads the low-latency MODE 7 form changes).  B = 4, the bars of check_qp."""
    from g1_locomotion_amd import BatchMPC
    B = 4
    x0, xr, ft, ct, w = _case(N, schedule, B)
    p = si.params(N)
    wu, wy = np.tile([0.0, 0.0, 20.0], (B, 4 * N)), np.zeros((B, 20 * N))
    with BatchMPC(horizon=N) as eng:
        st, _ = _fill(eng, x0, xr, ft, ct, w)
        st["warm_u"][:B], st["warm_y"][:B] = wu, wy
        eng.solve_staged_wrench(B, use_warm=True, want_x=True, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}_lat_ew"
        out = _out(st, B)
        cold = staged_wrench(eng, x0, xr, ft, ct, w)
    for b in range(B):
        ref = si.twin(p, x0[b], xr[b], ft[b], ct[b], ext_wrench=w[b], warm=(wu[b] / p.force_scale, wy[b]))
        si.check_qp(out, b, N, p, ref, ct[b])
    print(f"N={N} {schedule}: iters warm {out['iters'].tolist()} cold {cold['iters'].tolist()}, max |u warm - u cold| {np.abs(out['u'] - cold['u']).max():.3e} N")


def test_a_restart_pass_carries_the_wrench(torch_first, built_lib):
    """N = 4, full double support, QP 2 of the suite's batch: the twin runs past the restart mark of 55 iterations, so the staged call's host-driven loop
    starts a second pass -- which must solve under the same wrench.  Alone in a B = 1 call."""
    from g1_locomotion_amd import BatchMPC
    N = 4
    x0, xr, ft, ct, w = (v[2:3] for v in _case(N, "double", 8))
    p = si.params(N)
    ref = si.twin(p, x0[0], xr[0], ft[0], ct[0], ext_wrench=w[0])
    assert ref["iters"] > 55 and ref["status"] == orc.STATUS_SOLVED, ref["iters"]
    with BatchMPC(horizon=N) as eng:
        out = staged_wrench(eng, x0, xr, ft, ct, w)
        assert eng.kernel_name() == f"wrench_f64_n{N}_lat_ew"
    print(f"iters {int(out['iters'][0])} twin {ref['iters']}, |u - twin| {np.abs(out['u'][0] - ref['u']).max():.3e} N")
    si.check_qp(out, 0, N, p, ref, ct[0])


@pytest.mark.parametrize("N,schedule,B", [(12, "mixed", 4), (16, "mixed", 4), (20, "mixed", 4), (10, "double", 16)])
def test_the_batch_form_over_the_staging_arrays(torch_first, built_lib, N, schedule, B):
    """The long horizons, and more QPs than the low-latency form takes: the batch instantiation _ew reads the staged wrench array, with the completion word."""
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct, w = _case(N, schedule, B)
    p = si.params(N)
    with BatchMPC(horizon=N) as eng:
        out = staged_wrench(eng, x0, xr, ft, ct, w)
        assert eng.kernel_name() == f"wrench_f64_n{N}_ew"
    for b in range(B):
        si.check_qp(out, b, N, p, si.twin(p, x0[b], xr[b], ft[b], ct[b], ext_wrench=w[b]), ct[b])


ZERO_CASES = [(10, "mixed"), (10, "double"), (4, "single")]


@pytest.mark.parametrize("N,schedule", ZERO_CASES)
def test_a_zero_wrench_is_the_plain_staged_call(torch_first, built_lib, N, schedule):
    """An all-zero block against srbdqp_solve_staged_f64 on the same handle and inputs, B = 4; the largest differences are printed."""
    from g1_locomotion_amd import BatchMPC
    B = 4
    x0, xr, ft, ct, _ = _case(N, schedule, B)
    p = si.params(N)
    with BatchMPC(horizon=N) as eng:
        ref = staged_plain(eng, x0, xr, ft, ct)
        plain_kernel = eng.kernel_name()
        out = staged_wrench(eng, x0, xr, ft, ct, np.zeros((B, N, 6)))
        assert eng.kernel_name() == f"wrench_f64_n{N}_lat_ew"
    d = {k: np.abs(out[k].astype(float) - ref[k].astype(float)).max() for k in si.KEYS}
    bits = all(np.array_equal(out[k], ref[k]) for k in si.KEYS)
    print(f"N={N} {schedule}: plain call on {plain_kernel}; max |du| {d['u']:.3e} N, |dx| {d['x']:.3e}, |dy| {d['y']:.3e}, |d iters| {int(d['iters'])}, bit-identical: {bits}")
    assert np.array_equal(out["status"], ref["status"])
    assert d["iters"] <= p.check_every and d["u"] <= si.TOL_TWIN_N
    if N == 10:                                          # more than 60 presolved variables: the plain call runs the MODE 0 twin, and x_ref - 0.0 and s + 0.0 are exact
        assert plain_kernel == f"wrench_f64_n{N}_lat", plain_kernel
        assert bits, d
    else:
        assert plain_kernel == f"compact_f64_n{N}_s2_lat", plain_kernel


def test_the_wrench_is_the_calls(torch_first, built_lib):
    """Plain update, wrench update, plain update, three rounds on one handle (on whichever launch path the handle has): the two plain results of a round are
    bit-equal -- nothing was set and nothing had to be cleared -- and the wrench moved the forces by more than 1 N."""
    from g1_locomotion_amd import BatchMPC
    N = 10
    x0, xr, ft, ct, w = _case(N, "mixed", 3)
    with BatchMPC(horizon=N) as eng:
        for r in range(3):
            a = update_plain(eng, x0[r], xr[r], ft[r], ct[r])
            ka = eng.kernel_name()
            rc, m = update_wrench(eng, x0[r], xr[r], ft[r], ct[r], w[r])
            assert rc == 0 and eng.kernel_name() == f"wrench_f64_n{N}_lat_ew"
            b = update_plain(eng, x0[r], xr[r], ft[r], ct[r])
            assert eng.kernel_name() == ka
            assert all(np.array_equal(a[k], b[k]) for k in ("u", "x", "status", "iters")), r
            assert np.abs(m["u"] - a["u"]).max() > 1.0, r
        print("launch path:", eng.batch1_launch_path())


def test_refusals(torch_first, built_lib):
    """Every handle of the header's list refuses the two solve calls with SRBDQP_E_INVALID and a message that names the reason; the staging array itself
    is handed out on any handle."""
    from g1_locomotion_amd import BatchMPC, _lib
    from g1_locomotion_amd.mpc import robots_array, weights_array
    from test_gpu_variant_refusals import TAIL
    N, E = 4, f"srbdqp error {_lib.E_INVALID}: "
    x0, xr, ft, ct, w = _case(N, "double", 1)
    calls = {"srbdqp_solve_staged_wrench_f64": lambda eng: eng.solve_staged_wrench(1),
             "srbdqp_update_wrench_f64": lambda eng: eng._check(update_wrench(eng, x0[0], xr[0], ft[0], ct[0], w[0])[0])}
    sides = dict(robots=lambda e: e.set_robots(robots_array(1)), weights=lambda e: e.set_weights(weights_array(1)),
                 normals=lambda e: e.set_contact_normals(si.flat_normals(1, N)), ext_wrench=lambda e: e.set_external_wrench(w))
    for name, setit in sides.items():
        with BatchMPC(horizon=N) as eng:
            _fill(eng, x0, xr, ft, ct, w)
            setit(eng)
            for fn, call in calls.items():
                assert _refusal(lambda: call(eng)) == E + f"{fn}: {TAIL[name]}", (name, fn)
    with BatchMPC(horizon=N, rank_aware=True) as eng:
        for fn, call in calls.items():
            assert _refusal(lambda: call(eng)) == E + f"{fn}: {TAIL['rank_aware']}", fn
    def other(Nh, seed):                                             # the same two calls on a QP of another horizon
        q = orc.synthetic_batch(1, Nh, seed=seed, schedule="double")
        wq = si.draw_wrench(1, Nh, seed)
        return {"srbdqp_solve_staged_wrench_f64": lambda eng: eng.solve_staged_wrench(1),
                "srbdqp_update_wrench_f64": lambda eng: eng._check(update_wrench(eng, q[0][0], q[1][0], q[2][0], q[3][0], wq[0])[0])}
    with BatchMPC(horizon=3) as eng:                               # a live horizon (SRBDQP_FLAG_ANY_HORIZON)
        assert eng.stage_ext_wrench().shape == (eng.stage()["capacity"], 3, 6)
        for fn, call in other(3, 31).items():
            assert _refusal(lambda: call(eng)) == E + f"{fn}: {TAIL['live']}", fn
    with BatchMPC(horizon=24) as eng:
        for fn, call in other(24, 32).items():
            msg = _refusal(lambda: call(eng))
            assert msg is not None and msg.startswith(E + f"{fn}: an external wrench: not at N = 24"), msg
    for kern in (_lib.KERNEL_COMPACT, _lib.KERNEL_SPLIT, _lib.KERNEL_WAVE):
        with BatchMPC(horizon=N, kernel=kern) as eng:
            for fn, call in calls.items():
                msg = _refusal(lambda: call(eng))
                assert msg is not None and msg.startswith(E + f"{fn}: ") and "is read by the general kernel only" in msg, (kern, fn, msg)
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH) as eng:    # ... and the explicit general kernel is accepted
        assert staged_wrench(eng, x0, xr, ft, ct, w)["status"][0] == orc.STATUS_SOLVED


@pytest.mark.parametrize("value,qp,step,comp", [(np.nan, 0, 3, 1), (np.inf, 2, 0, 5), (2e6, 1, 9, 0)])
def test_a_bad_wrench_value_is_named_and_nothing_is_launched(torch_first, built_lib, value, qp, step, comp):
    from g1_locomotion_amd import BatchMPC, _lib
    N, B = 10, 3
    x0, xr, ft, ct, w = _case(N, "mixed", B)
    w = w.copy()
    w[qp, step, comp] = value
    if qp < B - 1:
        w[B - 1, 0, 0] = -np.inf                                    # (a later bad value: the FIRST one is named)
    want = (f"srbdqp error {_lib.E_INVALID}: srbdqp_solve_staged_wrench_f64: the wrench at (qp {qp}, step {step}, component {comp}) is invalid "
            "(every value must be finite with |value| <= 1e6); nothing was launched")
    with BatchMPC(horizon=N) as eng:
        st, _ = _fill(eng, x0, xr, ft, ct, w)
        for k in ("u", "x", "y"):
            st[k][:] = SENTINEL
        st["status"][:], st["iters"][:] = ISENTINEL, ISENTINEL
        assert _refusal(lambda: eng.solve_staged_wrench(B, want_x=True, want_y=True)) == want
        assert all(np.all(st[k] == SENTINEL) for k in ("u", "x", "y")) and np.all(st["status"] == ISENTINEL) and np.all(st["iters"] == ISENTINEL)
        good = si.draw_wrench(B, N, 5)
        eng.stage_ext_wrench()[:B] = good                            # (a refused update leaves the staged wrench array as it was: the caller's array is tested where it is)
        rc, one = update_wrench(eng, x0[qp], xr[qp], ft[qp], ct[qp], w[qp])
        assert np.array_equal(eng.stage_ext_wrench()[:B], good)
        assert rc == _lib.E_INVALID and f"srbdqp_update_wrench_f64: the wrench at (qp 0, step {step}, component {comp}) is invalid" in eng._lib.srbdqp_last_error(eng._h).decode()
        assert np.all(one["u"] == SENTINEL) and np.all(one["x"] == SENTINEL) and one["status"][0] == ISENTINEL
        assert all(np.all(st[k] == SENTINEL) for k in ("u", "x", "y")) and np.all(st["status"] == ISENTINEL)
        eng.solve_staged_wrench(B)                                   # ... and the good wrench on the same handle is solved
        assert np.all(st["status"][:B] == orc.STATUS_SOLVED)


@pytest.mark.parametrize("N,B", [(10, 4), (12, 2)])
def test_main_inputs_that_are_not_finite(torch_first, built_lib, N, B):
    """The contract of include/srbdqp.h under the wrench of the call, on both forms.  NaN in the foot position of a stance contact: status -1, u = y = 0,
    iters 0, and x_out FINITE, the roll-out of zero forces plus the wrench's response D, to 1e-9.  NaN in x0: status -1, u = y = 0, iters 0 or check_every; row 0
    of x_out is the caller's x0 and the other rows carry no meaning (the header: x_out is finite only where x0 is).  The clean QPs beside them meet the twin."""
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct, w = _case(N, "mixed", B)
    p = si.params(N)
    x0, ft = x0.copy(), ft.copy()
    k0 = int(np.flatnonzero(ct[0].any(1))[0]); c0 = int(np.flatnonzero(ct[0, k0])[0])
    ft[0, k0, 3 * c0 + 1] = np.nan
    x0[1, 4] = np.nan
    with BatchMPC(horizon=N) as eng:
        out = staged_wrench(eng, x0, xr, ft, ct, w)
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
    x0, xr, ft, ct, w = _case(N, "mixed", B)
    ct = ct.copy()
    ct[2] = 0
    p = si.params(N)
    with BatchMPC(horizon=N) as eng:
        out = staged_wrench(eng, x0, xr, ft, ct, w)
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
    x0, xr, ft, ct, w = _case(N, "mixed", 1)
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
        check_primal(dict(u=mpc.u_opt[None], x=mpc.x_opt[None], status=[mpc.status], iters=[mpc.iters]), N, p, ref, ct[0])
        assert np.abs(u0.reshape(-1) - ref["u"][0]).max() <= si.TOL_TWIN_N and np.abs(x1 - ref["x"]).max() <= 1e-5
        with pytest.raises(ValueError, match="contact_normals and external_wrench together"):
            mpc.update(ct[0], ft[0], None, external_wrench=w[0], contact_normals=np.tile([0.0, 0.0, 1.0], (N, 4)))
        u0p, x1p = mpc.update(ct[0], ft[0], None)
    finally:
        mpc.close()
    assert np.array_equal(u0p, u0f) and np.array_equal(x1p, x1f)
    assert np.abs(u0p - u0).max() > 1.0
