"""The two side inputs one staged call can carry -- an external wrench, contact normals -- as tests/test_gpu_staged_wrench.py and tests/test_gpu_staged_normals.py see them: one row per kind (the
test-side image of what srbdqp.hip's ExtWrenchIn / NormalsIn say about the staged path) the helpers that fill the staging arrays, make the calls and hold
the primal bars, and the one body of every test the two kinds share.  The twin, the batches, the draws and the seeds are those of tests/side_inputs.py."""
import ctypes as C
import functools
from typing import Callable, NamedTuple

import numpy as np

import side_inputs as si
import srbd_oracle as orc
from gpu_helpers import refusal

SENTINEL, ISENTINEL = 12345.678, 777


def _wrench_case(N, schedule, B):
    """The first B QPs of the wrench suite's batch of 16 and their wrenches."""
    x0, xr, ft, ct = si.batch(16, N, si.wrench_batch_seed(N, schedule), schedule)
    w = si.draw_wrench(16, N, si.wrench_seed(N))
    return x0[:B], xr[:B], ft[:B], ct[:B], w[:B]


def _normals_case(N, schedule, B):
    return si._normals_case(B, N, schedule)


class Staged(NamedTuple):
    name: str                       # the test ids
    base: si.Kind                   # its handle-level kind: the twin's keyword (slot), the kernel-name suffix
    width: int                      # doubles per horizon step
    stage: str                      # the methods of BatchMPC: the view of the staged array, the staged solve
    solve: str
    solve_fn: str                   # the C calls, as the messages name them
    update_fn: str
    case: Callable                  # (N, schedule, B) -> (x0, x_ref, foot, contact, the input of each QP)
    neutral: Callable               # (B, N) -> the input that says what no input says: zero / flat
    draw: Callable                  # (B, N, seed) -> some valid input at any horizon
    n24: str                        # behind "<call>: " on an N = 24 handle
    general_only: tuple             # where the kernel is not the general one: what follows "<call>: ", and the sentence's verb


WRENCH = Staged(name="wrench", base=si.EXT_WRENCH, width=6, stage="stage_ext_wrench", solve="solve_staged_wrench", solve_fn="srbdqp_solve_staged_wrench_f64",
                update_fn="srbdqp_update_wrench_f64", case=_wrench_case, neutral=lambda B, N: np.zeros((B, N, 6)), draw=si.draw_wrench,
                n24="an external wrench: not at N = 24", general_only=("", "is read by the general kernel only"))
NORMALS = Staged(name="normals", base=si.NORMALS, width=12, stage="stage_contact_normals", solve="solve_staged_normals", solve_fn="srbdqp_solve_staged_normals_f64",
                 update_fn="srbdqp_update_normals_f64", case=_normals_case, neutral=si.flat_normals, draw=lambda B, N, seed: si.flat_normals(B, N),
                 n24="contact normals: not at N = 24", general_only=("contact normals", "are read by the general kernel only"))
KINDS = (WRENCH, NORMALS)


def twin(kind, p, x0, xr, ft, ct, v, **kw):
    return si.twin(p, x0, xr, ft, ct, **{kind.base.slot: v}, **kw)


def suite8(kind, N, schedule):
    """The first 8 QPs of the kind's batch with their inputs, and the twin of each under its input (computed once, shared, left unchanged)."""
    return _suite8(kind.name, N, schedule)


@functools.lru_cache(maxsize=None)
def _suite8(name, N, schedule):
    kind = {k.name: k for k in KINDS}[name]
    x0, xr, ft, ct, v = kind.case(N, schedule, 8)
    p = si.params(N)
    refs = tuple(twin(kind, p, x0[b], xr[b], ft[b], ct[b], v[b]) for b in range(8))
    return x0, xr, ft, ct, v, p, refs


def lat_name(kind, N):
    return f"wrench_f64_n{N}_lat{kind.base.suffix}"


def batch_name(kind, N):
    return f"wrench_f64_n{N}{kind.base.suffix}"


def staged_view(kind, eng):
    return getattr(eng, kind.stage)()


def fill(eng, x0, xr, ft, ct, kind=None, v=None):
    """B QPs (and their side inputs of `kind`) into the first rows of the staging arrays -> (the arrays, B)."""
    st, B = eng.stage(), len(x0)
    st["x0"][:B], st["x_ref"][:B], st["foot"][:B], st["contact"][:B] = x0, xr, np.asarray(ft).reshape(B, eng.N, 12), np.asarray(ct) != 0
    if v is not None:
        staged_view(kind, eng)[:B] = v
    return st, B


def out_of(st, B):
    return {k: st[k][:B].copy() for k in si.KEYS}


def mark_outputs(st):
    for k in ("u", "x", "y"):
        st[k][:] = SENTINEL
    st["status"][:], st["iters"][:] = ISENTINEL, ISENTINEL


def outputs_untouched(st, iters=True):
    return all(np.all(st[k] == SENTINEL) for k in ("u", "x", "y")) and np.all(st["status"] == ISENTINEL) and (not iters or np.all(st["iters"] == ISENTINEL))


def staged(kind, eng, x0, xr, ft, ct, v, want_y=True):
    """The staged solve of the B QPs under their side inputs (v None: the staged array as it stands) -> dict(u, x, y, status, iters), copies."""
    st, B = fill(eng, x0, xr, ft, ct, kind, v)
    getattr(eng, kind.solve)(B, want_x=True, want_y=want_y)
    return out_of(st, B)


def staged_plain(eng, x0, xr, ft, ct, want_y=True):
    st, B = fill(eng, x0, xr, ft, ct)
    eng.solve_staged(B, want_x=True, want_y=want_y)
    return out_of(st, B)


def update_side(kind, eng, x0, xr, ft, ct, v):
    """The update call of ONE QP from the caller's own arrays into the caller's own outputs -> (rc, dict(u, x, status, iters) with a leading axis of 1)."""
    N = eng.N
    a = [np.ascontiguousarray(q, np.float64) for q in (x0, xr, ft)] + [np.ascontiguousarray(np.asarray(ct) != 0, np.uint8), np.ascontiguousarray(v, np.float64)]
    u0, u, x = np.full(12, SENTINEL), np.full((N, 12), SENTINEL), np.full((N + 1, 13), SENTINEL)
    status, iters = np.full(1, ISENTINEL, np.int32), np.full(1, ISENTINEL, np.int32)
    P = lambda q: q.ctypes.data_as(C.c_void_p)
    rc = getattr(eng._lib, kind.update_fn)(eng._h, P(a[0]), P(a[1]), P(a[2]), P(a[3]), None, P(a[4]), P(u0), P(u), P(x), P(status), P(iters))
    if rc == 0:
        assert np.array_equal(u0, u[0])
    return rc, dict(u=u[None], x=x[None], status=status, iters=iters)


def update_plain(eng, x0, xr, ft, ct):
    N = eng.N
    a = [np.ascontiguousarray(q, np.float64) for q in (x0, xr, ft)] + [np.ascontiguousarray(np.asarray(ct) != 0, np.uint8)]
    u0, u, x = np.empty(12), np.empty((N, 12)), np.empty((N + 1, 13))
    status, iters = np.zeros(1, np.int32), np.zeros(1, np.int32)
    P = lambda q: q.ctypes.data_as(C.c_void_p)
    eng._check(eng._lib.srbdqp_update_f64(eng._h, P(a[0]), P(a[1]), P(a[2]), P(a[3]), None, P(u0), P(u), P(x), P(status), P(iters)))
    return dict(u=u[None], x=x[None], status=status, iters=iters)


def check_primal(out, N, p, ref, contact):
    """check_qp's bars on what an update call returns -- it has no y_out, so the bars on the duals (the KKT residuals, the zero rows) are the staged call's
    alone: same status, iterations within one check interval, 2e-3 N from the twin, 1e-5 on x, the distance from the exact optimum, swing forces 0."""
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


# ---- the tests both kinds share: one body each; tests/test_gpu_staged_wrench.py and tests/test_gpu_staged_normals.py call them with their kind, under the
# names and cases their tests have always had ----
LOW_LATENCY_HORIZONS = (4, 8, 10)
WARM_CASES = [(4, "double"), (8, "mixed"), (10, "mixed")]
BATCH_FORM_CASES = [(12, "mixed", 4), (16, "mixed", 4), (20, "mixed", 4), (10, "double", 16)]
NEUTRAL_CASES = [(10, "mixed"), (10, "double"), (4, "single")]

# the one QP of the normals' 96 that the twin solves at exactly iteration 250 = max_iter: its status may legitimately read MAX_ITER on the hardware, so it alone is
# held to the forces and the roll-out
AT_THE_CAP = (10, "single", 3)


def low_latency_form_matches_the_twin(kind, N, schedule):
    """The first 8 QPs of the kind's batch in ONE staged call of B = 8, each against the twin run under its input.  No QP is left out: none whose twin count is
    the restart mark differed on the hardware.  Several pass the restart mark of 55 (normals, N = 8 double QP 1: 90; N = 8 three QP 5: 170; N = 10 double QP 0:
    70), so the host-driven restart pass runs under the input too.  The wrench's QP 0 once more, alone, through srbdqp_update_wrench_f64 (inputs and wrench in
    the kernel-argument segment); the normals have test_one_qp_in_the_argument_segment for that."""
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct, v, p, refs = suite8(kind, N, schedule)
    one = None
    with BatchMPC(horizon=N) as eng:
        out = staged(kind, eng, x0, xr, ft, ct, v)
        assert eng.kernel_name() == lat_name(kind, N)
        if kind is WRENCH:
            rc, one = update_side(kind, eng, x0[0], xr[0], ft[0], ct[0], v[0])
            assert rc == 0 and eng.kernel_name() == lat_name(kind, N)
    du = max(np.abs(out["u"][b] - refs[b]["u"]).max() for b in range(8))
    dx = max(np.abs(out["x"][b] - refs[b]["x"]).max() for b in range(8))
    print(f"N={N} {schedule}: max |u - twin| {du:.3e} N, max |x - twin| {dx:.3e}, iters {out['iters'].tolist()} twin {[r['iters'] for r in refs]}"
          + (f"; update: |u - twin| {np.abs(one['u'][0] - refs[0]['u']).max():.3e} N, iters {int(one['iters'][0])}" if one else ""))
    if kind is NORMALS:
        assert all(r["status"] == orc.STATUS_SOLVED for r in refs)
    for b in range(8):
        if kind is NORMALS and (N, schedule, b) == AT_THE_CAP:
            assert refs[b]["iters"] == p.max_iter
            assert np.abs(out["u"][b] - refs[b]["u"]).max() <= si.TOL_TWIN_N and np.abs(out["x"][b] - refs[b]["x"]).max() <= 1e-5
            continue
        si.check_qp(out, b, N, p, refs[b], ct[b])
    if one:
        check_primal(one, N, p, refs[0], ct[0])


def warm_start_under_the_input(kind, N, schedule):
    """use_warm = 1 against the twin started from the same point, B = 4, the bars of check_qp.  Under the wrench the start is 20 N on every normal force and zero
    duals (P x^0 goes through the G'v tables, whose layout over the threads the low-latency MODE 7 form changes); on the normals it is the twin's own solution
    as warm_u (world frame, newtons) and warm_y: the world -> local conversion of the start."""
    from g1_locomotion_amd import BatchMPC
    B = 4
    x0, xr, ft, ct, v, p, refs = suite8(kind, N, schedule)
    x0, xr, ft, ct, v = x0[:B], xr[:B], ft[:B], ct[:B], v[:B]
    if kind is WRENCH:
        wu, wy = np.tile([0.0, 0.0, 20.0], (B, 4 * N)), np.zeros((B, 20 * N))
    else:
        wu, wy = np.stack([refs[b]["u"].reshape(-1) for b in range(B)]), np.stack([refs[b]["y"] for b in range(B)])
    with BatchMPC(horizon=N) as eng:
        st, _ = fill(eng, x0, xr, ft, ct, kind, v)
        st["warm_u"][:B], st["warm_y"][:B] = wu, wy
        getattr(eng, kind.solve)(B, use_warm=True, want_x=True, want_y=True)
        assert eng.kernel_name() == lat_name(kind, N)
        out = out_of(st, B)
        cold = staged(kind, eng, x0, xr, ft, ct, v) if kind is WRENCH else None
    warm = [twin(kind, p, x0[b], xr[b], ft[b], ct[b], v[b], warm=(wu[b] / p.force_scale, wy[b])) for b in range(B)]
    if kind is WRENCH:
        print(f"N={N} {schedule}: iters warm {out['iters'].tolist()} cold {cold['iters'].tolist()}, max |u warm - u cold| {np.abs(out['u'] - cold['u']).max():.3e} N")
    else:
        print(f"N={N} {schedule}: iters warm {out['iters'].tolist()} twin warm {[r['iters'] for r in warm]} twin cold {[refs[b]['iters'] for b in range(B)]}")
    for b in range(B):
        si.check_qp(out, b, N, p, warm[b], ct[b])


def batch_form_over_the_staging_arrays(kind, N, schedule, B):
    """The long horizons, and more QPs than the low-latency form takes: the batch instantiation _ew / _cn reads the staged array, with the completion word.
    (Normals, N = 20: QPs 1 and 2 pass that horizon's restart mark of 125.)"""
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct, v = kind.case(N, schedule, B)
    p = si.params(N)
    with BatchMPC(horizon=N) as eng:
        out = staged(kind, eng, x0, xr, ft, ct, v)
        assert eng.kernel_name() == batch_name(kind, N)
    for b in range(B):
        si.check_qp(out, b, N, p, twin(kind, p, x0[b], xr[b], ft[b], ct[b], v[b]), ct[b])


def neutral_input_is_the_plain_staged_call(kind, N, schedule):
    """An all-zero wrench block / (0, 0, 1) everywhere against srbdqp_solve_staged_f64 on the same handle and inputs, B = 4; the largest differences are
    printed.  The zero wrench: the twin's bars, and bit identity at N = 10.  Flat normals: to rounding, by the project's bars for the batch form (si.NORMALS)."""
    from g1_locomotion_amd import BatchMPC
    B = 4
    x0, xr, ft, ct, _ = kind.case(N, schedule, B)
    p = si.params(N)
    with BatchMPC(horizon=N) as eng:
        ref = staged_plain(eng, x0, xr, ft, ct)
        plain_kernel = eng.kernel_name()
        out = staged(kind, eng, x0, xr, ft, ct, kind.neutral(B, N))
        assert eng.kernel_name() == lat_name(kind, N)
    d = {k: np.abs(out[k].astype(float) - ref[k].astype(float)).max() for k in si.KEYS}
    bits = all(np.array_equal(out[k], ref[k]) for k in si.KEYS)
    print(f"N={N} {schedule}: plain call on {plain_kernel}; max |du| {d['u']:.3e} N, |dx| {d['x']:.3e}, |dy| {d['y']:.3e}, |d iters| {int(d['iters'])}"
          + (f", bit-identical: {bits}" if kind is WRENCH else ""))
    assert np.array_equal(out["status"], ref["status"])
    if kind is NORMALS:
        assert d["iters"] <= si.NORMALS.neutral_iters and d["u"] <= si.NORMALS.neutral_tol, d
        return
    assert d["iters"] <= p.check_every and d["u"] <= si.TOL_TWIN_N
    if N == 10:                                          # more than 60 presolved variables: the plain call runs the MODE 0 twin, and x_ref - 0.0 and s + 0.0 are exact
        assert plain_kernel == f"wrench_f64_n{N}_lat", plain_kernel
        assert bits, d
    else:
        assert plain_kernel == f"compact_f64_n{N}_s2_lat", plain_kernel


def input_is_the_calls(kind):
    """Plain update, update with the input, plain update, three rounds on one handle (on whichever launch path the handle has): the two plain results of a round
    are bit-equal -- nothing was set and nothing had to be cleared -- and the input (a drawn wrench; a ridge) moved the forces by more than 1 N.  A block of the
    staged normals array nobody wrote acts as flat ground."""
    from g1_locomotion_amd import BatchMPC
    N = 10
    if kind is WRENCH:
        x0, xr, ft, ct, v = kind.case(N, "mixed", 3)
    else:
        x0, xr, ft, ct = si.batch(3, N, 4210, "double")
        v = si.ridge_normals(3, N)
    with BatchMPC(horizon=N) as eng:
        if kind is NORMALS:
            assert np.array_equal(eng.stage_contact_normals(), si.flat_normals(eng.stage()["capacity"], N))
        for r in range(3):
            a = update_plain(eng, x0[r], xr[r], ft[r], ct[r])
            ka = eng.kernel_name()
            rc, m = update_side(kind, eng, x0[r], xr[r], ft[r], ct[r], v[r])
            assert rc == 0 and eng.kernel_name() == lat_name(kind, N)
            b = update_plain(eng, x0[r], xr[r], ft[r], ct[r])
            assert eng.kernel_name() == ka
            assert all(np.array_equal(a[k], b[k]) for k in ("u", "x", "status", "iters")), r
            assert np.abs(m["u"] - a["u"]).max() > 1.0, r
        if kind is WRENCH:
            print("launch path:", eng.batch1_launch_path())
            return
        # blocks 1 and 2 were never written (update writes block 0): a B = 3 call solves QPs 1 and 2 on flat ground
        assert np.array_equal(eng.stage_contact_normals()[1:3], si.flat_normals(2, N))
        mixed = staged(kind, eng, x0, xr, ft, ct, None)
        eng.stage_contact_normals()[0] = si.flat_normals(1, N)[0]
        flat = staged(kind, eng, x0, xr, ft, ct, None)
        assert all(np.array_equal(mixed[k][1:], flat[k][1:]) for k in si.KEYS)
        assert np.abs(mixed["u"][0] - flat["u"][0]).max() > 1.0
        plain = staged_plain(eng, x0, xr, ft, ct)
        assert np.array_equal(flat["status"], plain["status"]) and np.abs(flat["u"] - plain["u"]).max() <= si.NORMALS.neutral_tol


def refusals(kind):
    """Every handle of the header's list refuses the two solve calls with SRBDQP_E_INVALID and a message that names the reason, and leaves the outputs alone;
    the staging array itself is handed out on any handle."""
    from g1_locomotion_amd import BatchMPC, _lib
    from g1_locomotion_amd.mpc import robots_array, weights_array
    from test_gpu_variant_refusals import TAIL
    N, E = 4, f"srbdqp error {_lib.E_INVALID}: "
    x0, xr, ft, ct, v = kind.case(N, "double", 1)
    outs = []

    def upd(eng, q, vq):
        rc, one = update_side(kind, eng, q[0][0], q[1][0], q[2][0], q[3][0], vq[0])
        outs.append(one)
        eng._check(rc)

    def calls_on(q, vq):
        return {kind.solve_fn: lambda eng: getattr(eng, kind.solve)(1), kind.update_fn: lambda eng: upd(eng, q, vq)}
    calls = calls_on((x0, xr, ft, ct), v)

    def refused(eng, call):
        st = eng.stage()
        mark_outputs(st)
        del outs[:]
        msg = refusal(lambda: call(eng))
        assert outputs_untouched(st)
        assert all(np.all(o["u"] == SENTINEL) and np.all(o["x"] == SENTINEL) and o["status"][0] == ISENTINEL for o in outs)
        return msg
    sides = dict(robots=lambda e: e.set_robots(robots_array(1)), weights=lambda e: e.set_weights(weights_array(1)),
                 normals=lambda e: e.set_contact_normals(si.flat_normals(1, N)), ext_wrench=lambda e: e.set_external_wrench(si.draw_wrench(1, N, 3)))
    for name, setit in sides.items():
        with BatchMPC(horizon=N) as eng:
            fill(eng, x0, xr, ft, ct, kind, v)
            setit(eng)
            for fn, call in calls.items():
                assert refused(eng, call) == E + f"{fn}: {TAIL[name]}", (name, fn)
    with BatchMPC(horizon=N, rank_aware=True) as eng:
        for fn, call in calls.items():
            assert refused(eng, call) == E + f"{fn}: {TAIL['rank_aware']}", fn

    def other(Nh, seed):                                             # the same two calls on a QP of another horizon
        return calls_on(orc.synthetic_batch(1, Nh, seed=seed, schedule="double"), kind.draw(1, Nh, seed))
    with BatchMPC(horizon=3) as eng:                               # a live horizon (SRBDQP_FLAG_ANY_HORIZON)
        assert staged_view(kind, eng).shape == (eng.stage()["capacity"], 3, kind.width)
        for fn, call in other(3, 31).items():
            assert refused(eng, call) == E + f"{fn}: {TAIL['live']}", fn
    with BatchMPC(horizon=24) as eng:
        for fn, call in other(24, 32).items():
            msg = refused(eng, call)
            assert msg is not None and msg.startswith(E + f"{fn}: {kind.n24}"), msg
    lead, sentence = kind.general_only
    for kern in (_lib.KERNEL_COMPACT, _lib.KERNEL_SPLIT, _lib.KERNEL_WAVE):
        with BatchMPC(horizon=N, kernel=kern) as eng:
            for fn, call in calls.items():
                msg = refused(eng, call)
                assert msg is not None and msg.startswith(E + f"{fn}: {lead}") and sentence in msg, (kern, fn, msg)
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH) as eng:    # ... and the explicit general kernel is accepted
        assert staged(kind, eng, x0, xr, ft, ct, v)["status"][0] == orc.STATUS_SOLVED


def bad_value_is_named(kind, N, B, x0, xr, ft, ct, bad, good, qp, where, why, solved):
    """The staged solve over `bad` (B blocks, the first bad value in QP qp at `where`) is refused in those words and nothing is launched; so is the update call
    of QP qp from the caller's own array, which leaves the staged array as it was (`good`); then the good input on the same handle is solved."""
    from g1_locomotion_amd import BatchMPC, _lib
    want = f"srbdqp error {_lib.E_INVALID}: {kind.solve_fn}: {where.format(qp=qp)} is invalid ({why}); nothing was launched"
    with BatchMPC(horizon=N) as eng:
        st, _ = fill(eng, x0, xr, ft, ct, kind, bad)
        mark_outputs(st)
        assert refusal(lambda: getattr(eng, kind.solve)(B, want_x=True, want_y=True)) == want
        assert outputs_untouched(st)
        staged_view(kind, eng)[:B] = good                         # (a refused update leaves the staged array as it was: the caller's array is tested where it is)
        rc, one = update_side(kind, eng, x0[qp], xr[qp], ft[qp], ct[qp], bad[qp])
        assert np.array_equal(staged_view(kind, eng)[:B], good)
        assert rc == _lib.E_INVALID and f"{kind.update_fn}: {where.format(qp=0)} is invalid ({why})" in eng._lib.srbdqp_last_error(eng._h).decode()
        assert np.all(one["u"] == SENTINEL) and np.all(one["x"] == SENTINEL) and one["status"][0] == ISENTINEL
        assert outputs_untouched(st, iters=False)
        getattr(eng, kind.solve)(B)                                  # ... and the good input on the same handle is solved
        assert np.all(np.isin(st["status"][:B], solved))
