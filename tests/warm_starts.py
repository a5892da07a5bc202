"""What the tests of a CALLER's warm start share (tests/test_warm_starts_cpu.py, tests/test_gpu_warm_starts.py) -- TEST INFRASTRUCTURE ONLY: the starts, the one
twin of every solve path, the cases and the bars.

The C-ABI takes a caller's start as warm_u / warm_y on the four batch solves, as use_warm on the staged call and through the ragged warm pair
(include/srbdqp.h).  Every kernel has its own code for it: the per-lane loads warm_u[b n + 3 act + ax] / s and warm_y[b m + irow], z^0 = clip(A x^0), the
closed-form P x^0, and -- on the general kernel -- the fp32-tile instantiation's late P x^0, the per-QP r s^2 of the weights form, the world-to-local change of
warm_u under contact normals, the row offsets of ragged buckets and a live horizon's own stride.

The starts.
  shifted_start   what a receding-horizon caller has: the solution of the previous control step's QP (rows [0, 0, 1, ..., N - 2] of this one), shifted by one
                  step, the last step repeated.  Where the gait changes inside the horizon it carries force on contacts that swing now.
  neighbour_start the solution of the next QP of the batch: a poor start (tests/test_gpu_parity.py::test_restart_in_place_from_a_warm_start).
  with_junk       the same start with +1e6 on every force entry and -1e6 on every dual row of a swing contact: the twins drop those entries (x^0[vi], y^0[ri]),
                  so a kernel that reads one of them differs from its own clean run.

The sharp instrument is ONE check interval from the start (max_iter = check_every = 5, no rho restart): there the iterate from a shifted start is 6 - 75 N
from the cold one (tests/test_warm_starts_cpu.py asserts > 1 N on every QP), so a start that is ignored, mis-scaled or mis-indexed cannot meet a 1e-4 N bar;
a full solve ends within ~1e-3 N of the cold solve whatever its start.  P x^0 enters the stopping test only (the iteration does not read it): what a test can
see of it is the decision at the first checks of a full solve -- the counts of the full solves and of the restarts from the own solution -- and nothing else.

The bars, all from the suite as it stands.
  fp64  status equal; iteration counts within one check_every; forces <= 2e-3 N (tests/test_gpu_wrench.py), and <= 1e-4 N where the counts are equal (the
        large-batch tests' bar for QPs of equal count, tightened by the ten-fold the five-iteration runs allow: kernel and twin differ by summation order only);
        roll-out <= 1e-5; a SOLVED QP <= 5e-2 N from orc.solve_reference.
  fp32  the bars of tests/test_gpu_wrench.py: 2e-2 N to the fp32 twin, counts within two check intervals, roll-out 1e-3, 1e-1 N to the exact optimum of the
        fp32-rounded QP.
  duals the force bar's relative size (bar / 200 N, a nominal stance force) on the twin's own magnitude: fp64 5e-7 max(1, |y_twin|_inf) (1e-4 N / 200 N),
        whatever the counts; fp32 1e-4 (2e-2 N / 200 N).
"""
import functools
from dataclasses import replace
from typing import NamedTuple, Optional

import numpy as np

import degenerate_twin as dt
import rank_aware_twin as rt
import side_inputs as si
import srbd_oracle as orc

TOL_TWIN_N, TOL_EXACT_N, TOL_EQUAL_N, TOL_X = si.TOL_TWIN_N, si.TOL_EXACT_N, 1e-4, 1e-5
TOL32_TWIN_N, TOL32_EXACT_N, TOL32_X = 2e-2, 1e-1, 1e-3
DUAL64, DUAL32 = 5e-7, 1e-4
JUNK = 1.0e6
# The weights records: the kind's draw without its two special records (zero angular weights, all-zero q: the second is SOLVED inside the first interval, where
# nothing is left to compare), from a seed -- the case's plus this -- at which the twin's full solves without a rho restart, from either foreign start, stop
# within 5e-2 N of the exact optimum: drawn weights move the ADMM's stopping point, 0.1 - 1.6 N out at most seeds, and the exact bar is the kernel's, not the rule's
WEIGHTS_SEED = 2144
B8 = 8


# ---- the starts ---------------------------------------------------------------------------------------------------------------------------------
def shifted_start(p, x0, x_ref, foot, contact, solve):
    """The start a receding-horizon caller carries into this QP: solve(p, x0, x_ref', foot', contact') -> dict(u (N, 12) newtons, y (20 N,)) of the previous
    control step's QP -- rows [0, 0, 1, ..., N - 2] of x_ref, foot and contact --, forces and duals shifted by one step with the last step repeated.
    -> (warm_u (12 N,) newtons, warm_y (20 N,))."""
    N = np.asarray(x_ref).shape[0]
    prev = np.concatenate([[0], np.arange(N - 1)])
    o = solve(p, x0, np.asarray(x_ref)[prev], np.asarray(foot).reshape(N, -1)[prev], np.asarray(contact).reshape(N, -1)[prev])
    ahead = np.concatenate([np.arange(1, N), [N - 1]])
    return np.asarray(o["u"], np.float64).reshape(N, 12)[ahead].reshape(-1).copy(), np.asarray(o["y"], np.float64).reshape(N, 20)[ahead].reshape(-1).copy()


def neighbour_start(outs, b):
    """The solution of QP b + 1 of the batch (the first one for the last): outs = dict(u (B, N, 12), y (B, 20 N)) -> (warm_u (12 N,), warm_y (20 N,))."""
    B = len(outs["u"])
    return np.asarray(outs["u"][(b + 1) % B], np.float64).reshape(-1).copy(), np.asarray(outs["y"][(b + 1) % B], np.float64).reshape(-1).copy()


def with_junk(warm_u, warm_y, contact):
    """The same start (one QP, or a batch with a leading axis) with + JUNK on every force entry and - JUNK on every dual row of a swing contact.  Finite values."""
    swing = np.asarray(contact).reshape(-1, 4) == 0
    wu, wy = np.array(warm_u, np.float64), np.array(warm_y, np.float64)
    wu.reshape(-1, 4, 3)[swing] += JUNK
    wy.reshape(-1, 4, 5)[swing] -= JUNK
    return wu, wy


def swing_force(warm_u, contact):
    """The largest |warm_u| entry of one QP on a contact that swings now [N]."""
    swing = np.asarray(contact).reshape(-1, 4) == 0
    return float(np.abs(np.asarray(warm_u).reshape(-1, 4, 3)[swing]).max(initial=0.0))


# ---- the one twin -------------------------------------------------------------------------------------------------------------------------------
PATHS = ("dense", "wrench_f64", "wrench_f32", "wrench_f32t", "side", "rank_aware")


def twin(path, p, q, warm=None):
    """The twin of one solve of the QP q = dict(x0, x_ref, foot, contact[, normals, ext_wrench]) with parameters p on `path`, from the caller's start
    warm = (warm_u (12 N,) world newtons, warm_y (20 N,)) or from zero:
      dense        orc.update: the one-wave, split and 4-wave kernels;
      wrench_f64   orc.update_split(float64): the general kernel; wrench_f32 / wrench_f32t: its fp32 iterations on fp64 tiles / tile_dtype="auto" (an _f32 call
                   sees the start rounded to float32 too);
      side         si.twin: the side-input forms (records and weights are in p, normals and the wrench in q);
      rank_aware   rank_aware_twin.update_rank_aware.
    -> the twin's dict(u, x, y, iters, status, qp ...)."""
    f32 = path in ("wrench_f32", "wrench_f32t")
    w = None
    if warm is not None:
        wu, wy = (np.asarray(v, np.float32 if f32 else np.float64).astype(np.float64).reshape(-1) for v in warm)
        w = (wu / p.force_scale, wy)
    a = (q["x0"], q["x_ref"], q["foot"], q["contact"])
    if path == "dense":
        return orc.update(p, *a, warm=w)
    if path == "wrench_f64":
        return orc.update_split(p, *a, warm=w, dtype=np.float64)
    if f32:
        return orc.update_split(p, *a, warm=w, dtype=np.float32, tile_dtype="auto" if path == "wrench_f32t" else np.float64)
    if path == "side":
        return si.twin(p, *a, normals=q.get("normals"), ext_wrench=q.get("ext_wrench"), warm=w)
    if path == "rank_aware":
        return rt.update_rank_aware(p, *a, warm=w)
    raise ValueError(path)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    """One solve path: its batch, its twin, the handle that runs it and the kernel name that handle has to report."""
    id: str
    path: str                       # PATHS
    N: int
    schedule: str                   # si.SCHEDULES, "three34" (3 or 4 stance contacts on every step: fp32 tiles), or a degenerate_twin.BATCHES name
    seed: int
    name: str                       # srbdqp_kernel_name() after the solve
    kernel: str = "AUTO"            # _lib.KERNEL_<kernel>
    cfg: tuple = ()                 # further srbdqp_config fields, as (key, value) pairs
    flags: tuple = ()               # _lib.FLAG_<flag> names
    call: str = "host"              # "host": solve(); "device": solve_device() and flush()
    sides: tuple = ()               # si.Kind names set on the handle
    rank_aware: bool = False
    iters: int = 5                  # what one interval is on this path (wave_defer: 6, below)
    B: int = B8

    @property
    def f32(self):
        return self.path in ("wrench_f32", "wrench_f32t")


def _c(*a, **kw):
    return Case(*a, **kw)


# One check interval from the caller's start.  (wave_defer_*: the planner picks that kernel only with a rho restart inside the cap, so its case is the shortest run
# that has one -- five iterations from the caller's start, a re-balancing, one more in the deferred continuation: rho_restart_iter = 5, max_iter = 6, on both sides.)
CASES = (
    _c("wave_n10_s2", "dense", 10, "single", 9110, "wave_f64_n10_s2", cfg=(("max_contacts_per_step", 2),)),
    _c("wave_n4_s2", "dense", 4, "single", 11858, "wave_f64_n4_s2", cfg=(("max_contacts_per_step", 2),)),
    _c("wave_n4_s4", "dense", 4, "mixed", 13504, "wave_f64_n4_s4"),
    _c("split_n10_s2", "dense", 10, "single", 9110, "split_f64_n10_s2", kernel="SPLIT", cfg=(("max_contacts_per_step", 2),)),
    _c("compact_n10_s4", "dense", 10, "mixed", 9110, "compact_f64_n10_s4"),
    _c("wave_defer_n10_s2", "dense", 10, "single", 10410, "wave_defer_f64_n10_s2", cfg=(("max_contacts_per_step", 2), ("rho_restart_iter", 5), ("max_iter", 6)),
       flags=("DEFER_TAIL",), call="device", iters=6),
    _c("wrench_f64_n4_double", "wrench_f64", 4, "double", 9104, "wrench_f64_n4", kernel="WRENCH"),
    _c("wrench_f64_n10_mixed", "wrench_f64", 10, "mixed", 9110, "wrench_f64_n10", kernel="WRENCH"),
    _c("wrench_f64_n20_double", "wrench_f64", 20, "double", 9120, "wrench_f64_n20", kernel="WRENCH"),
    _c("wrench_f64_n20_three", "wrench_f64", 20, "three", 9120, "wrench_f64_n20", kernel="WRENCH"),
    _c("wrench_f64_n24_mixed", "wrench_f64", 24, "mixed", 9124, "wrench_f64_n24", kernel="WRENCH"),
    _c("wrench_f32_n12_three", "wrench_f32", 12, "three", 9112, "wrench_f32_n12", kernel="WRENCH"),
    _c("wrench_f32_n20_double", "wrench_f32", 20, "double", 9120, "wrench_f32_n20", kernel="WRENCH"),
    _c("wrench_f32t_n12_double", "wrench_f32t", 12, "double", 9112, "wrench_f32_n12", kernel="WRENCH", flags=("F32_TILES",)),
    _c("wrench_f32t_n12_three", "wrench_f32t", 12, "three34", 9112, "wrench_f32_n12", kernel="WRENCH", flags=("F32_TILES",)),
    _c("wrench_f32t_n20_double", "wrench_f32t", 20, "double", 9120, "wrench_f32_n20", kernel="WRENCH", flags=("F32_TILES",)),
    _c("wrench_f32t_n20_three", "wrench_f32t", 20, "three34", 9120, "wrench_f32_n20", kernel="WRENCH", flags=("F32_TILES",)),
    _c("wrench_f64_h15_mixed", "wrench_f64", 15, "mixed", 9115, "wrench_f64_n16_h15"),
    _c("robots_n10_mixed", "side", 10, "mixed", 9110, "wrench_f64_n10_rb", sides=("robots",)),
    _c("weights_n10_mixed", "side", 10, "mixed", 9110, "wrench_f64_n10_wt", sides=("weights",)),
    _c("normals_n10_mixed", "side", 10, "mixed", 9110, "wrench_f64_n10_cn", sides=("normals",)),
    _c("ext_wrench_n10_mixed", "side", 10, "mixed", 9110, "wrench_f64_n10_ew", sides=("ext_wrench",)),
    _c("combined_n16_mixed", "side", 16, "mixed", 9316, "wrench_f64_n16_ew", sides=("robots", "weights", "ext_wrench")),
    _c("rank_aware_n10_mixed", "rank_aware", 10, "mixed", 9110, "wrench_f64_n10_ra", kernel="WRENCH", rank_aware=True),
    _c("rank_aware_n10_ladder", "rank_aware", 10, "n10_three", 0, "wrench_f64_n10_ra", kernel="WRENCH", rank_aware=True, B=0),
)
BY_ID = {c.id: c for c in CASES}
# Full solves from a foreign start: one fp64 and one fp32 case per kernel family (the presolved families have no fp32 form), N among 4, 10, 12, 20
FULL_CASES = ("wave_n10_s2", "wave_n4_s4", "split_n10_s2", "compact_n10_s4", "wave_defer_n10_s2", "wrench_f64_n10_mixed", "wrench_f64_n20_double",
              "wrench_f32_n12_three", "wrench_f32t_n20_three", "weights_n10_mixed", "normals_n10_mixed", "rank_aware_n10_mixed")
KINDS = {k.name: k for k in si.KINDS}


def restarts(case):
    """Whether the full solves of a case run with the default rho restart, on both sides: wave_defer_* exists only with a restart inside the cap."""
    return "DEFER_TAIL" in case.flags


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The batch of a case: dict(x0, x_ref, foot, contact, rec = {kind name: its array}); computed once, left unchanged."""
    if case.schedule in dt.BATCHES:                                  # every rung of the ladder pair
        x0, xr, ft, ct = dt.inputs(case.schedule)[:4]
    elif case.schedule == "three34":                                 # as tests/test_gpu_wrench.py builds its fp32-tile "three" pattern
        x0, xr, ft, ct = si.batch(case.B, case.N, case.seed, "double")
        rng = np.random.default_rng(case.N)
        for b in range(case.B):
            for k in range(case.N):
                if rng.random() < 0.5:
                    ct[b, k, rng.integers(0, 4)] = 0
    else:
        x0, xr, ft, ct = si.batch(case.B, case.N, case.seed, case.schedule)
    B, N = x0.shape[0], case.N
    rec = {}
    for s in case.sides:
        if s == "normals":
            rec[s] = si.wedge_normals(B, N)
        elif s == "weights":
            rec[s] = si.draw_weights(B + 2, case.seed + WEIGHTS_SEED)[2:].copy()
        else:
            rec[s] = KINDS[s].draw(B, N, case.seed + {"robots": 1000, "ext_wrench": 4000}[s])
    d = dict(x0=x0, x_ref=xr, foot=ft, contact=np.ascontiguousarray(ct, np.uint8), rec=rec)
    for a in (d["x0"], d["x_ref"], d["foot"], d["contact"], *rec.values()):
        a.setflags(write=False)
    return d


def qp_of(case, b):
    """QP b of a case as twin() takes it."""
    d = inputs(case)
    q = dict(x0=d["x0"][b], x_ref=d["x_ref"][b], foot=d["foot"][b], contact=d["contact"][b])
    for s in ("normals", "ext_wrench"):
        if s in d["rec"]:
            q[s] = d["rec"][s][b]
    return q


def params(case, b, full=False, restart=False):
    """The oracle's parameters of QP b of a case: one interval (max_iter = check_every = 5, no restart; the case's own cfg where it has one), or -- full -- the
    default cap, without the rho restart or -- restart -- with the engine's default one."""
    rec = inputs(case)["rec"]
    p = si.params(case.N, rec["robots"][b] if "robots" in rec else None, rec["weights"][b] if "weights" in rec else None)
    if case.f32:
        p = replace(p, eps_abs=2e-6, eps_rel=2e-6)                   # the fp32 path's tolerance floor
    if full:
        return p if restart else replace(p, rho_restart_iter=0)
    cfg = dict(case.cfg)
    return replace(p, max_iter=cfg.get("max_iter", 5), rho_restart_iter=cfg.get("rho_restart_iter", 0), rho_restart_count=1)


@functools.lru_cache(maxsize=None)
def starts(case):
    """The shifted start of every QP of a case, (B, 12 N) newtons and (B, 20 N): the previous step's QP solved by the dense twin (the side-input forms: by their
    own, with this step's normals and wrench) at the default cap without restart.  Cases with the same batch share it."""
    d = inputs(case)
    B = d["x0"].shape[0]
    first = next(c for c in CASES if (c.N, c.schedule, c.seed, c.B, c.sides) == (case.N, case.schedule, case.seed, case.B, case.sides))
    if first is not case:
        return starts(first)
    WU, WY = np.empty((B, 12 * case.N)), np.empty((B, 20 * case.N))
    for b in range(B):
        q = qp_of(case, b)
        if case.path == "side":
            solve = lambda p, x0, xr, ft, ct: twin("side", p, dict(q, x0=x0, x_ref=xr, foot=ft, contact=ct))
        else:
            solve = lambda p, x0, xr, ft, ct: orc.update(p, x0, xr, ft, ct)
        p = replace(params(case, b, full=True), eps_abs=1e-6, eps_rel=1e-6)
        WU[b], WY[b] = shifted_start(p, q["x0"], q["x_ref"], q["foot"], q["contact"], solve)
    WU.setflags(write=False); WY.setflags(write=False)
    return WU, WY


# ---- the bars -----------------------------------------------------------------------------------------------------------------------------------
def measure(out, b, ref):
    """(|du| N, |dx|, |dy|, |y_twin|_inf, d iters) of QP b of the engine's out against ref = twin(...)."""
    f = lambda v: np.asarray(v, np.float64)
    return (float(np.abs(f(out["u"][b]) - ref["u"]).max()), float(np.abs(f(out["x"][b]) - ref["x"]).max()),
            float(np.abs(f(out["y"][b]).reshape(-1) - ref["y"]).max()), float(np.abs(ref["y"]).max(initial=0.0)), int(out["iters"][b]) - int(ref["iters"]))


def check(case, out, b, ref, p, exact=False):
    """QP b of the engine's out = dict(u, x, y, status, iters) against ref = twin(...) with parameters p by the bars of the docstring; exact: a SOLVED QP against
    orc.solve_reference of the twin's QP too.  -> measure(...)."""
    du, dx, dy, yn, di = m = measure(out, b, ref)
    tag = (case.id, b, m)
    assert int(out["status"][b]) == ref["status"] and ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER), (tag, out["status"][b], ref["status"])
    if case.f32:
        assert abs(di) <= 2 * p.check_every, tag
        assert du <= TOL32_TWIN_N and dx <= TOL32_X and dy <= DUAL32 * max(1.0, yn), tag
    else:
        assert abs(di) <= p.check_every, tag
        assert du <= (TOL_EQUAL_N if di == 0 else TOL_TWIN_N) and dx <= TOL_X and dy <= DUAL64 * max(1.0, yn), tag
    if exact and ref["status"] == orc.STATUS_SOLVED:
        qp = ref.get("qp_loc", ref["qp"])
        xs, _ = orc.solve_reference(p, qp)
        u = np.asarray(out["u"][b], np.float64).reshape(-1)
        u_loc = u if ref.get("T") is None else ref["T"].T @ u
        assert np.abs(u_loc - xs * p.force_scale).max() <= (TOL32_EXACT_N if case.f32 else TOL_EXACT_N), tag
    return m


def report(title, ms):
    """One line of the measured maxima of a case (what the summary's table is made of)."""
    ms = list(ms)
    print(f"{title}: max |u - twin| {max(m[0] for m in ms):.3e} N, |x - twin| {max(m[1] for m in ms):.3e}, |y - twin| {max(m[2] for m in ms):.3e} "
          f"(|y_twin| {max(m[3] for m in ms):.3e}), |iters - twin| {max(abs(m[4]) for m in ms)}")


# ---- the twins' runs, computed once per distinct (twin, batch, cap) and shared by the tests that need them ------------------------------------------
def _first(case):
    key = lambda c: (c.path, c.N, c.schedule, c.seed, c.B, c.sides, c.iters)
    return next(c for c in CASES if key(c) == key(case))


@functools.lru_cache(maxsize=None)
def interval_twins(case, start="shifted"):
    """Per QP of a case the twin's one-interval run from `start`: "cold", "shifted" or "junk" (the shifted start through with_junk)."""
    if _first(case) is not case:
        return interval_twins(_first(case), start)
    d = inputs(case)
    WU, WY = starts(case)
    out = []
    for b in range(d["x0"].shape[0]):
        w = None if start == "cold" else (WU[b], WY[b])
        if start == "junk":
            w = with_junk(*w, d["contact"][b])
        out.append(twin(case.path, params(case, b), qp_of(case, b), w))
    return out


@functools.lru_cache(maxsize=None)
def full_twins(case, start="cold", restart=False):
    """Per QP of a case the twin's full solve (default cap; restart: with the engine's default rho restart) from `start`: "cold", "shifted", or "neighbour" (the
    cold twin's own solution of the next QP of the batch)."""
    if _first(case) is not case:
        return full_twins(_first(case), start, restart)
    return [twin(case.path, params(case, b, full=True, restart=restart), qp_of(case, b), full_start(case, start, b))
            for b in range(inputs(case)["x0"].shape[0])]


def full_start(case, start, b):
    """The start of QP b of a full solve, (warm_u, warm_y) or None."""
    if start == "cold":
        return None
    if start == "shifted":
        WU, WY = starts(case)
        return WU[b], WY[b]
    cold = full_twins(case, "cold")
    return neighbour_start(dict(u=[r["u"] for r in cold], y=[r["y"] for r in cold]), b)
