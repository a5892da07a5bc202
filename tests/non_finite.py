"""What the tests of NON-FINITE MAIN INPUTS share (tests/test_non_finite_cpu.py, tests/test_gpu_non_finite.py) -- TEST INFRASTRUCTURE ONLY: the poison table, the
cases, and the one checker of the contract.  It imports no GPU.

The contract is include/srbdqp.h's: a QP whose main inputs (x0, x_ref, foot, pcom, warm_u, warm_y) are not finite ends with SRBDQP_NUMERICAL, forces and duals
exactly 0, after at most the first residual check, and is never run again; no other QP of the batch changes by a bit.  The oracles are NOT the reference for
the rejected QP (tests/test_non_finite_cpu.py shows what they return for one); they are the reference for what surrounds it: the neighbours' status, the
zero-force roll-out, and the swing-foot rows.

The poison table (ROWS).  A row names an array, an index rule on one QP's contact schedule, its class, and whether the zero-force roll-out reads the entry:
  rejects   the QP must end SRBDQP_NUMERICAL;
  harmless  (a swing contact's foot position only) every output of the QP is bit-identical to the clean solve.
The roll-out x_{k+1} = A_k x_k + B_k u_k reads x0 and the yaw column of x_ref (A_k, and the frame of B_k); with u = 0 it reads nothing else -- lever arms
(foot, pcom) only weigh forces, the other x_ref entries and the warm arrays only enter the QP.  tests/test_non_finite_cpu.py derives both columns from the
oracle.  Values: nan, +inf, -inf; fp32 host calls add 1e39 (finite in float64, inf once the call rounds it to float32).

check_contract holds a solve's outputs to all of it.  Sentinel: the device-buffer calls of the GPU file prefill every output with SENTINEL (a finite value no
solve produces), so "written at all" can be told from "written with the right value".
"""
import functools
from typing import Callable, NamedTuple, Optional

import numpy as np

import side_inputs as si
import srbd_oracle as orc

SENTINEL, ISENTINEL = 12345.0, 12345
NUMERICAL, PENDING, SOLVED, MAX_ITER = orc.STATUS_NUMERICAL, 0, orc.STATUS_SOLVED, orc.STATUS_MAX_ITER
KEYS = ("u", "x", "y", "status", "iters")
VALUES = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}
F32_VALUES = dict(VALUES, big=1.0e39)                     # 1e39: finite in float64, inf as float32
TOL_X64, TOL_X32 = 1e-9, 1e-3                            # the suite's own bars of a roll-out without forces (tests/test_gpu_parity.py), of an fp32 roll-out (tests/test_gpu_wrench.py)
B12 = 12


# ---- the poison table -----------------------------------------------------------------------------------------------------------------------------
def _steps(ct, lo, hi):
    c = (np.asarray(ct).reshape(-1, 4) != 0).sum(1)
    return [k for k in range(len(c)) if lo <= c[k] <= hi]


def _stance_le2(N, ct):
    ks = _steps(ct, 1, 2)
    return None if not ks else (ks[len(ks) // 2], 3 * int(np.flatnonzero(ct[ks[len(ks) // 2]])[0]) + 1)


def _stance_ge3(N, ct):
    ks = _steps(ct, 3, 4)
    return None if not ks else (ks[len(ks) // 2], 3 * int(np.flatnonzero(ct[ks[len(ks) // 2]])[-1]) + 0)


def _swing(N, ct):
    """A swing contact's z coordinate: of a step with exactly three stance contacts where the QP has one (there the general kernel weighs the swing column inside
    the step's 6 x 6 block), of the first step with a swing contact otherwise."""
    ks = _steps(ct, 3, 3) or _steps(ct, 0, 3)
    return None if not ks else (ks[0], 3 * int(np.flatnonzero(ct[ks[0]] == 0)[0]) + 2)


def _first_stance(ct):
    k = _steps(ct, 1, 4)
    return None if not k else (k[0], int(np.flatnonzero(ct[k[0]])[0]))


class Row(NamedTuple):
    name: str
    array: str                      # the key of arrays() the poison goes to
    rejects: bool                   # False: harmless
    rollout_reads: bool             # the zero-force roll-out reads the entry
    index: Callable                 # (N, contact (N, 4) of the QP) -> the index into the QP's own array, or None where the QP has no such entry
    needs: str = "plain"            # the call the row needs: "plain", "pcom" (pcom given) or "warm" (warm_u and warm_y given)


ROWS = (
    Row("x0_pos", "x0", True, True, lambda N, ct: (4,)),
    Row("x0_vel", "x0", True, True, lambda N, ct: (10,)),
    Row("xref_yaw_mid", "x_ref", True, True, lambda N, ct: (N // 2, 2)),
    Row("xref_last", "x_ref", True, False, lambda N, ct: (N - 1, 7)),          # (an angular velocity: columns 3:6 are the lever arms' CoM where no pcom is given)
    Row("xref_com_last", "x_ref", True, False, lambda N, ct: (N - 1, 4)),      # (no pcom given: the lever arms' origin, like pcom)
    Row("xref_com_pcom", "x_ref", True, False, lambda N, ct: (N - 1, 4), "pcom"),   # (pcom given: a tracking target only, like xref_last)
    Row("foot_stance_le2", "foot", True, False, _stance_le2),
    Row("foot_stance_ge3", "foot", True, False, _stance_ge3),
    Row("foot_swing", "foot", False, False, _swing),
    Row("pcom", "pcom", True, False, lambda N, ct: (N // 2, 0), "pcom"),
    Row("warm_u", "warm_u", True, False, lambda N, ct: None if _first_stance(ct) is None else (12 * _first_stance(ct)[0] + 3 * _first_stance(ct)[1] + 2,), "warm"),
    Row("warm_y", "warm_y", True, False, lambda N, ct: None if _first_stance(ct) is None else (20 * _first_stance(ct)[0] + 5 * _first_stance(ct)[1] + 4,), "warm"),
)
ROW = {r.name: r for r in ROWS}
FEW = ("x0_pos", "foot_stance_le2", "foot_stance_ge3", "foot_swing")       # the families that do not take the whole table: x0, a stance foot, the swing foot; nan only


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    """One kernel family at one of its smallest horizons: the batch, the handle that runs it and the kernel name that handle has to report."""
    id: str
    N: int
    schedule: str                   # si.SCHEDULES, or "alt_three": every other QP with 3 or 4 stance contacts on every step (fp32 tiles), the rest a mixed gait (fp64 tiles)
    twin: str                       # "dense" (orc.update), "wrench" (orc.update_split)
    name: str                       # srbdqp_kernel_name() after the solve
    kernel: str = "AUTO"            # _lib.KERNEL_<kernel>
    cfg: tuple = ()                 # further srbdqp_config fields
    flags: tuple = ()               # _lib.FLAG_<flag> names
    f32: bool = False
    full: bool = False              # the whole table x {nan, +inf, -inf} (fp32: and 1e39), or FEW x nan
    sides: tuple = ()               # si.Kind names set on the handle
    rank_aware: bool = False
    B: int = B12

    @property
    def seed(self):
        return 900 + self.N

    @property
    def bad_qps(self):
        """The first QP, one in the middle (neighbours on both sides), the last."""
        return (0, self.B // 2, self.B - 1)


def _c(*a, **kw):
    return Case(*a, **kw)


S2 = (("max_contacts_per_step", 2),)
CASES = (
    _c("wave_n4_double", 4, "double", "dense", "wave_f64_n4_s4", kernel="WAVE", full=True),
    _c("wave_n8_single", 8, "single", "dense", "wave_f64_n8_s2", kernel="WAVE", cfg=S2, full=True),
    _c("split_n4_double", 4, "double", "dense", "split_f64_n4_s4", kernel="SPLIT"),
    _c("split_n8_single", 8, "single", "dense", "split_f64_n8_s2", kernel="SPLIT", cfg=S2),
    _c("compact_n4_double", 4, "double", "dense", "compact_f64_n4_s4", kernel="COMPACT"),
    _c("compact_n12_single", 12, "single", "dense", "compact_f64_n12_s2", kernel="COMPACT", cfg=S2),
    _c("wrench_f64_n4_double", 4, "double", "wrench", "wrench_f64_n4", kernel="WRENCH", full=True),
    _c("wrench_f64_n8_mixed", 8, "mixed", "wrench", "wrench_f64_n8", kernel="WRENCH", full=True),
    _c("wrench_f64_n10_three", 10, "three", "wrench", "wrench_f64_n10", kernel="WRENCH", full=True),
    _c("wrench_f32_n4_double", 4, "double", "wrench", "wrench_f32_n4", f32=True, full=True),
    _c("wrench_f32_n8_mixed", 8, "mixed", "wrench", "wrench_f32_n8", f32=True, full=True),
    _c("wrench_f32t_n4_alt", 4, "alt_three", "wrench", "wrench_f32_n4", flags=("F32_TILES",), f32=True),
    _c("live_h5_mixed", 5, "mixed", "wrench", "wrench_f64_n8_h5"),
    _c("live_h13_mixed", 13, "mixed", "wrench", "wrench_f64_n16_h13"),
    _c("robots_n4_double", 4, "double", "wrench", "wrench_f64_n4_rb", sides=("robots",)),
    _c("weights_n4_double", 4, "double", "wrench", "wrench_f64_n4_wt", sides=("weights",)),
    _c("ext_wrench_n4_double", 4, "double", "wrench", "wrench_f64_n4_ew", sides=("ext_wrench",)),
    _c("normals_n4_double", 4, "double", "wrench", "wrench_f64_n4_cn", sides=("normals",)),
    _c("rank_aware_n4_double", 4, "double", "wrench", "wrench_f64_n4_ra", kernel="WRENCH", rank_aware=True),
)
# A poisoned QP beside the rho restart: every QP of these batches is past the first mark (25) in the oracle, in place (one-wave kernel), as further launches
# (general kernel), and deferred (SRBDQP_FLAG_DEFER_TAIL: handed to the next solve / run on the tail stream)
RESTART = (("rho_restart_iter", 25), ("rho_restart_count", 2))
RESTART_ROWS = ("x0_pos", "foot_swing", "warm_u", "warm_y")
RESTART_CASES = (
    _c("restart_wave_n4_double", 4, "double", "dense", "wave_f64_n4_s4", kernel="WAVE", cfg=RESTART),
    _c("restart_wave_defer_n4_double", 4, "double", "dense", "wave_defer_f64_n4_s4", kernel="WAVE", cfg=RESTART, flags=("DEFER_TAIL",)),
    _c("restart_wave_n8_single", 8, "single", "dense", "wave_f64_n8_s2", kernel="WAVE", cfg=S2 + RESTART),
    _c("restart_wrench_n12_mixed", 12, "mixed", "wrench", "wrench_f64_n12", kernel="WRENCH", cfg=RESTART),
    _c("restart_wrench_defer_n12_mixed", 12, "mixed", "wrench", "wrench_f64_n12", kernel="WRENCH", cfg=RESTART, flags=("DEFER_TAIL",)),
)
BY_ID = {c.id: c for c in CASES + RESTART_CASES}


def restart_rows(case):
    """The rows of RESTART_ROWS that have an entry in a poisoned QP of a restart case (full double support has no swing contact)."""
    return [ROW[n] for n in RESTART_ROWS if picks_of(case, ROW[n], np.nan)]
KINDS = {k.name: k for k in si.KINDS}
# the live horizons poison the LAST real step (the rows behind it are the instantiation's padding): x_ref there, and a stance foot there
LIVE_ROWS = (ROW["xref_last"],
             Row("foot_last_step", "foot", True, False, lambda N, ct: None if not ct[N - 1].any() else (N - 1, 3 * int(np.flatnonzero(ct[N - 1])[0]) + 1)))


def batch(B, N, seed, schedule):
    x0, xr, ft, ct = si.batch(B, N, seed, "mixed" if schedule == "alt_three" else schedule)
    if schedule == "alt_three":      # (as tests/test_gpu_wrench.py builds its fp32-tile "three" pattern; step 0 always has three, so every such QP has a swing contact)
        rng = np.random.default_rng(seed)
        for b in range(0, B, 2):
            ct[b] = 1
            for k in range(N):
                if k == 0 or rng.random() < 0.5:
                    ct[b, k, rng.integers(0, 4)] = 0
    return x0, xr, ft, ct


@functools.lru_cache(maxsize=None)
def arrays(case):
    """The clean batch of a case: dict(x0, x_ref, foot, contact, pcom, warm_u, warm_y, rec = {kind name: its array}); computed once, left unchanged.  pcom is
    x_ref's own CoM horizon moved by up to 3 cm, warm_u 20 N on every normal force (the kernels drop the entries of swing contacts), warm_y zero."""
    x0, xr, ft, ct = batch(case.B, case.N, case.seed, case.schedule)
    B, N = case.B, case.N
    pc = xr[:, :, 3:6] + np.random.default_rng(case.seed).uniform(-0.03, 0.03, (B, N, 3))
    wu = np.tile([0.0, 0.0, 20.0], (B, 4 * N))
    rec = {}
    for s in case.sides:
        rec[s] = si.wedge_normals(B, N) if s == "normals" else KINDS[s].draw(B + 2, N, case.seed + 7)[2:].copy()   # (weights: without the draw's two special records)
    d = dict(x0=x0, x_ref=xr, foot=ft.reshape(B, N, 12), contact=np.ascontiguousarray(ct, np.uint8).reshape(B, N, 4), pcom=pc, warm_u=wu,
             warm_y=np.zeros((B, 20 * N)), rec=rec)
    for a in (*[d[k] for k in ("x0", "x_ref", "foot", "contact", "pcom", "warm_u", "warm_y")], *rec.values()):
        a.setflags(write=False)
    return d


def index_of(case, row, b):
    """Where `row` poisons QP b of a case (an index into arrays(case)[row.array][b]), or None."""
    return row.index(case.N, arrays(case)["contact"][b])


def picks_of(case, row, value):
    """(b, row, value) for the poisoned QPs of a case in which the row has an entry."""
    return [(b, row, value) for b in case.bad_qps if index_of(case, row, b) is not None]


def rows_of(case):
    """The (row, value name) pairs a case takes, by its share of the table: the rows that have an entry in at least one of the poisoned QPs."""
    rows = ROWS if case.full else tuple(ROW[n] for n in FEW)
    if case.id.startswith("live_"):
        rows = (ROW["x0_pos"], ROW["foot_swing"]) + LIVE_ROWS
    if case.sides or case.rank_aware:
        rows = tuple(r for r in rows if r.needs == "plain")
    values = (F32_VALUES if case.f32 else VALUES) if case.full else {"nan": np.nan}
    return [(r, v) for r in rows if picks_of(case, r, np.nan) for v in values]


def poisoned(case, picks):
    """arrays(case) with the value of every pick (b, row, value) written at the row's place in QP b: fresh copies of the arrays that change."""
    d = dict(arrays(case))
    for b, row, value in picks:
        if not d[row.array].flags.writeable:
            d[row.array] = d[row.array].copy()
        d[row.array][(b,) + tuple(index_of(case, row, b))] = value
    return d


def call_args(d, needs):
    """(pcom, warm_u, warm_y) of a call of kind `needs` on the arrays d."""
    return (d["pcom"] if needs == "pcom" else None, d["warm_u"] if needs == "warm" else None, d["warm_y"] if needs == "warm" else None)


# ---- the oracle's side ----------------------------------------------------------------------------------------------------------------------------
def params(case, **kw):
    """The oracle's parameters of a case: no rho restart (the engines of these tests run with rho_restart_iter = -1 unless a test is about restarts); the fp32
    path's tolerance floor."""
    kw = dict({k: v for k, v in case.cfg if k.startswith("rho_restart")}, **kw)         # (RESTART_CASES: the restart the handle is created with)
    if case.f32:
        kw = dict(dict(eps_abs=2e-6, eps_rel=2e-6), **kw)
    return orc.params_for(case.N, **kw)


def oracle(case, d, b, needs="plain", p=None):
    """The oracle's solve of QP b of the arrays d as the case's kernel family runs it (no side input: the side-input cases share the plain twin's verdict)."""
    p = p or params(case)
    pc, wu, wy = call_args(d, needs)
    warm = None if wu is None else (wu[b] / p.force_scale, wy[b])
    a = (p, d["x0"][b], d["x_ref"][b], d["foot"][b], d["contact"][b], None if pc is None else pc[b])
    if case.twin == "dense":
        return orc.update(*a, warm=warm)
    return orc.update_split(*a, warm=warm, dtype=np.float32 if case.f32 else np.float64, tile_dtype="auto" if "F32_TILES" in case.flags else np.float64)


def zero_rollout(case, d, b, needs="plain"):
    """The oracle's roll-out of QP b without forces (orc.update with the contact array zeroed, as tests/test_gpu_parity.py::
    test_contact_bound_and_empty_contact_set): (N + 1, 13).  An fp32 call sees its inputs rounded to float32."""
    pc = call_args(d, needs)[0]
    rnd = (lambda v: np.asarray(v, np.float32).astype(np.float64)) if case.f32 else (lambda v: np.asarray(v, np.float64))
    p = orc.params_for(case.N)
    x = orc.update(p, rnd(d["x0"][b]), rnd(d["x_ref"][b]), rnd(d["foot"][b]), np.zeros_like(d["contact"][b]), None if pc is None else rnd(pc[b]))["x"]
    if "ext_wrench" in case.sides:   # (include/srbdqp.h: a QP that gets zero forces is still pushed -- "the roll-out under the wrench")
        x[1:] += si.response(p, d["x_ref"][b], d["rec"]["ext_wrench"][b])
    return x


# ---- the contract ---------------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_contract(out, clean, bad, p, *, x0, zero_x, f32=False, allow_pending=False, tag=""):
    """The outputs `out` of a solve with poisoned QPs against the contract; `clean`: the same batch without poison on the same engine.  Both are
    dict(u, x, y, status, iters), each indexed by the QP (arrays with a leading batch axis, or lists of per-QP arrays); x or y may be None where not asked for.
      bad     {QP index: its Row}
      p       the solve's parameters (check_every, max_iter)
      x0      the x0 array as the call received it (poison included)
      zero_x  b -> the oracle's zero-force roll-out of QP b (zero_rollout); called for the rows whose roll-out does not read the poison
      allow_pending  the test left deferred work unflushed on purpose: a QP that is not rejected may read SRBDQP_PENDING
    -> {QP index: iters} of the rejected QPs (what the GPU file's header table records)."""
    B = len(out["status"])
    seen = {}
    fl = np.float32 if f32 else np.float64
    for b in range(B):
        t = (tag, b, getattr(bad.get(b), "name", None))
        st = int(out["status"][b])
        if b in bad and bad[b].rejects:
            row = bad[b]
            assert st != PENDING, (t, "a rejected QP is never PENDING")
            assert st == NUMERICAL, (t, "status", st)
            u = np.asarray(out["u"][b])
            assert not np.isnan(u).any() and np.all(u == 0.0), (t, "forces of a rejected QP are exactly 0", u.ravel()[np.flatnonzero(~(u.ravel() == 0.0))[:4]])
            if out.get("y") is not None:
                assert np.all(np.asarray(out["y"][b]) == 0.0), (t, "duals of a rejected QP are exactly 0")
            it = int(out["iters"][b])
            assert it in (0, p.check_every), (t, "iters of a rejected QP: 0 or the first check", it)
            seen[b] = it
            if out.get("x") is not None:
                x = np.asarray(out["x"][b])
                assert x.dtype == fl, (t, x.dtype)
                if row.rollout_reads:
                    assert same_bits(x[0], np.asarray(x0[b], fl)), (t, "row 0 of x is the caller's x0, bit for bit")
                else:
                    ref = zero_x(b)
                    err = np.abs(x.astype(np.float64) - ref).max()
                    assert err <= (TOL_X32 if f32 else TOL_X64), (t, "x of a rejected QP is the zero-force roll-out", err)     # (NaN fails the comparison)
            for k in ("u", "x", "y"):
                if out.get(k) is not None:
                    assert not np.any(np.asarray(out[k][b]) == SENTINEL), (t, k, "holds the sentinel: not written")
            assert it != ISENTINEL and st != ISENTINEL, t
            continue
        # every other QP (a harmless row's too): bit-identical to the clean solve, in every key
        assert st in (SOLVED, MAX_ITER) or (allow_pending and st == PENDING), (t, "status", st)
        for k in KEYS:
            if out.get(k) is None:
                assert clean.get(k) is None, (t, k)
                continue
            assert same_bits(out[k][b], clean[k][b]), (t, k, "differs from the clean solve")
    return seen
