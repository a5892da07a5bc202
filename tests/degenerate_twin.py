"""Ladders of nearly collinear stance contacts and what the CPU oracle says about each rung -- TEST INFRASTRUCTURE ONLY (plain module, imported by
tests/test_degenerate_contacts_cpu.py and tests/test_gpu_degenerate_contacts.py).

A ladder = one base QP of synthetic_batch() deformed by scenarios.collinear_contacts() at every eps of scenarios.EPS_LADDER; a batch = two ladders
(two geometries).  For every rung reference() computes, once per process,
  * the exact optimum (orc.solve_reference) and the dense twin (orc.update), which the degeneracy does not touch: the dense twin has to be SOLVED,
    within 2e-3 N of the optimum and below a fifth of the bound, else the rung is not a fair input and reference() raises;
  * the wrench twin WITHOUT the guard (orc.update_split(guard=False)): the rung is FREE-OK when that is SOLVED within a fifth of the bound, and BAD when it
    is non-finite, NUMERICAL, or answered outside the bound.  A free-ok rung above the guard's threshold is MUST-ANSWER.  A free-ok rung below it is
    OVER-REJECTED: the guard looks at one step's geometry alone, and at equal pivot ratio the error grows with the horizon and with the number and place
    of the degenerate steps (2.6e-10 on the last step of N = 10 is 1e-2 N off, 2.5e-8 on every step of N = 20 is 0.12 N off), so a threshold that
    keeps the second kind out refuses some of the first.  These rungs are counted (test_degenerate_contacts_cpu.py) and listed in DESIGN.md;
  * the wrench twin WITH the guard: the status a must-answer rung has to come back with.
The contract (check_contract): a QP is either answered -- SOLVED or MAX_ITER, forces within the bound of the exact optimum, with SOLVED the KKT
residuals at the suite's bounds, swing entries exactly 0 -- or rejected: SRBDQP_NUMERICAL, u, y and iters exactly 0, x the finite roll-out of zero
forces.  A must-answer QP has to be answered, with the guarded twin's status.

A rung whose pivot ratio lies within a factor 4 of a guard threshold is where kernel and twin may legitimately decide differently (fma and summation
order): such a rung is MOVED to a neighbouring eps (MOVED below; the table in DESIGN.md lists them) rather than excused.
"""
import functools

import numpy as np

import srbd_oracle as orc
import scenarios as sc

BOUND = {"f64": 5e-2, "f32": 1e-1, "f32t": 1e-1}          # the suite's force bounds against the exact optimum [N] (tests/test_gpu_wrench.py)
RUNGS4 = (1e-1, 1e-3, 1e-5, 0.0)                            # the N = 20 ladder

# (kind, nominal eps) -> eps used: rungs of the issue's ladder that fell inside the factor-4 band of a threshold
MOVED = {("tandem", 1e-3): 3e-4, ("tandem", 1e-2): 2.2e-2, ("point", 3e-3): 1.5e-3}

# name -> N, schedule, [(seed, kind, placement)] -- one ladder per geometry --, the arithmetic modes the batch is run in ("f64", "f32" = fp32 iterations on fp64
# tiles, "f32t" = fp32 iterations on fp32 tiles)
BATCHES = {
    "n4_double": dict(N=4, schedule="double", geoms=((11, "tandem", "all"), (12, "point", "all")), modes=("f64", "f32t")),
    "n10_mixed": dict(N=10, schedule="mixed", geoms=((11, "tandem", "first"), (20, "point", "last")), modes=("f64",)),
    "n10_three": dict(N=10, schedule="three", geoms=((11, "tandem", "all"), (12, "point", "first")), modes=("f64",)),
    "n10_double": dict(N=10, schedule="double", geoms=((11, "tandem", "all"), (12, "point", "last")), modes=("f64", "f32")),
    "n20_double": dict(N=20, schedule="double", geoms=((11, "tandem", "all"), (12, "point", "all")), rungs=RUNGS4, modes=("f32t",)),
    "n7_mixed": dict(N=7, schedule="mixed", geoms=((11, "tandem", "last"), (12, "point", "all")), modes=("f64",)),
    "n8_mixed": dict(N=8, schedule="mixed", geoms=((11, "tandem", "all"), (12, "point", "first")), modes=("f64",)),
    "n12_mixed": dict(N=12, schedule="mixed", geoms=((11, "tandem", "first"), (12, "point", "all")), modes=("f64",)),
}
CASES = [(name, mode) for name, d in BATCHES.items() for mode in d["modes"]]


def threshold(mode):
    return orc.GUARD_RATIO_F64 if mode == "f64" else orc.GUARD_RATIO_F32


def rungs_of(name):
    return BATCHES[name].get("rungs", sc.EPS_LADDER)


def eps_used(kind, eps):
    return MOVED.get((kind, eps), eps)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The deformed QPs of a batch, geometry-major: x0, x_ref, foot, contact, and [(geometry index, nominal eps)] per QP."""
    d = BATCHES[name]
    parts, meta = [], []
    for g, (seed, kind, placement) in enumerate(d["geoms"]):
        parts.append(sc.collinear_ladder(d["N"], d["schedule"], seed, kind, placement, tuple(eps_used(kind, e) for e in rungs_of(name))))
        meta += [(g, e) for e in rungs_of(name)]
    x0, xr, ft, ct = (np.concatenate([p[i] for p in parts]) for i in range(4))
    for a in (x0, xr, ft, ct):
        a.setflags(write=False)
    return x0, xr, ft, ct, meta


@functools.lru_cache(maxsize=None)
def healthy(name):
    """As many undeformed synthetic_batch() QPs as the batch has rungs (same horizon and schedule)."""
    d = BATCHES[name]
    B = len(inputs(name)[4])
    x0, xr, ft, ct = orc.synthetic_batch(B, d["N"], 900 + d["N"], "mixed" if d["schedule"] == "three" else d["schedule"])
    if d["schedule"] == "three":
        ct = sc.three_contacts(ct, 900 + d["N"])
    return x0, xr, ft, ct


def interleaved(name):
    """Every second QP healthy: x0, x_ref, foot, contact of 2 B QPs; deformed QP i sits at 2 i, healthy QP i at 2 i + 1."""
    dd, hh = inputs(name)[:4], healthy(name)
    out = []
    for a, h in zip(dd, hh):
        z = np.empty((2 * a.shape[0],) + a.shape[1:], a.dtype)
        z[0::2], z[1::2] = a, h
        out.append(z)
    return tuple(out)


def params(N, mode, **kw):
    return orc.params_for(N, **kw) if mode == "f64" else orc.params_for(N, eps_abs=2e-6, eps_rel=2e-6, **kw)     # (the fp32 path's tolerance floor)


def _twin(p, mode, x0, xr, ft, ct, guard):
    kw = dict(dtype=np.float64) if mode == "f64" else dict(dtype=np.float32, tile_dtype="auto" if mode == "f32t" else np.float64)
    with np.errstate(all="ignore"):
        return orc.update_split(p, x0, xr, ft, ct, guard=guard, **kw)


@functools.lru_cache(maxsize=None)
def reference(name, mode="f64", restart=False):
    """Per deformed QP of the batch: dict(eps, geom, ratio, us (exact forces, (N, 12)), qp, dense_err, free (unguarded twin: err, status), must_answer,
    bad, guarded (the guarded twin's result))."""
    d = BATCHES[name]
    N = d["N"]
    x0, xr, ft, ct, meta = inputs(name)
    kw = dict(zip(("rho_restart_iter", "rho_restart_count"), orc.default_restart(N))) if restart else {}
    p = params(N, mode, **kw)
    bound = BOUND[mode]
    refs = []
    for b, (g, eps) in enumerate(meta):
        a = (x0[b], xr[b], ft[b]) if mode == "f64" else tuple(np.asarray(v, np.float32).astype(np.float64) for v in (x0[b], xr[b], ft[b]))
        dense = orc.update(p, *a, ct[b])                                     # the dense path on the inputs as the kernel sees them
        xs, _ = orc.solve_reference(p, dense["qp"])
        us = (xs * p.force_scale).reshape(N, 12)
        dense_err = float(np.abs(dense["u"] - us).max())
        if not (dense["status"] == orc.STATUS_SOLVED and dense_err <= 2e-3 and dense_err < bound / 5):
            raise AssertionError(f"{name} rung {b} (eps {eps:g}): the dense twin is no reference here: status {dense['status']}, {dense_err:.2e} N")
        free = _twin(p, mode, x0[b], xr[b], ft[b], ct[b], False)
        finite = bool(np.all(np.isfinite(free["u"])))
        err = float(np.abs(free["u"] - us).max()) if finite else np.inf
        answered = free["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER)
        refs.append(dict(eps=eps, geom=g, ratio=free["pivot_ratio"], us=us, qp=dense["qp"], dense_err=dense_err, free_err=err, free_status=free["status"],
                         free_ok=bool(free["status"] == orc.STATUS_SOLVED and err <= bound / 5),
                         bad=bool(not finite or not answered or err > bound),
                         guarded=_twin(p, mode, x0[b], xr[b], ft[b], ct[b], True)))
        r = refs[-1]
        r["must_answer"] = r["free_ok"] and r["ratio"] > threshold(mode)
        r["over_rejected"] = r["free_ok"] and not r["ratio"] > threshold(mode)
    return refs, p


def zero_rollout(qp, x0):
    return orc.rollout(qp, x0, np.zeros(qp["P"].shape[0]), 1.0)


def check_contract(tag, u, x, y, status, iters, ref, ct, p, mode, x0, must_status=True, frames=None, world_qp=None):
    """The either-or contract on one QP; returns "answered" or "rejected".  frames, world_qp: a solve with contact normals -- ref["qp"] is the QP in the
    contacts' own frames T = frames (side_inputs.frames_matrix), u stays in the world frame."""
    bound = BOUND[mode]
    u64 = np.asarray(u, np.float64).reshape(-1)
    assert np.all(np.isfinite(u64)), (tag, "non-finite forces")
    if x is not None:
        assert np.all(np.isfinite(x)), (tag, "non-finite states")
    red, vi, ri = orc.presolve(ref["qp"], ct)
    if status == orc.STATUS_NUMERICAL:
        assert not ref["must_answer"], (tag, "a must-answer QP was rejected", ref["ratio"])
        assert np.all(u64 == 0.0) and iters == 0, (tag, iters, np.abs(u64).max())
        if y is not None:
            assert np.all(np.asarray(y) == 0.0), tag
        if x is not None:
            assert np.abs(np.asarray(x, np.float64) - zero_rollout(world_qp or ref["qp"], x0)).max() <= (1e-9 if mode == "f64" else 1e-4), tag
        return "rejected"
    assert status in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER), (tag, status)
    err = float(np.abs(u64 - ref["us"].reshape(-1)).max())
    assert err <= bound, (tag, f"answered {err:.3e} N from the optimum (status {status}, ratio {ref['ratio']:.2e})")
    assert np.all(u64[np.setdiff1d(np.arange(u64.size), vi)] == 0.0), (tag, "swing entries")
    if status == orc.STATUS_SOLVED and y is not None:
        u_loc = u64 if frames is None else frames.T @ u64
        kr = orc.kkt_residuals(red["P"], red["q"], red["A"], red["l"], red["u"], u_loc[vi] / p.force_scale, np.asarray(y, np.float64).reshape(-1)[ri])
        qn = max(1.0, float(np.abs(ref["qp"]["q"]).max()))
        assert kr["primal"] <= 1e-4 and kr["stationarity"] <= 1e-3 * qn, (tag, kr)      # (the suite's bounds: tests/test_gpu_wrench.py)
    if ref["must_answer"] and must_status:
        assert status == ref["guarded"]["status"], (tag, status, ref["guarded"]["status"])
    return "answered"
