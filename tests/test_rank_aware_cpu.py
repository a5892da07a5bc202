"""Rank-aware wrench steps on the oracle's twin (tests/rank_aware_twin.py), without a GPU: the cure for the nearly collinear stance contacts that the general
kernel's conditioning guard refuses (tests/test_degenerate_contacts_cpu.py).  Every rung of every fp64 ladder of degenerate_twin.BATCHES -- 148 QPs, 82 of them
with a step at or below the guard and 105 with a step in normalised coordinates (rank_aware_twin.SELECT_RATIO), n20_double included -- has to be answered: SOLVED, within a fifth of the suite's force bound (1e-2 N) of the exact optimum,
in exactly as many iterations as the dense twin orc.update.  No rung is left out.  (The prototype's worst case was 3.9e-3 N.)  The same QPs run on the GPU in
tests/test_gpu_rank_aware.py.
"""
import functools
import os

import numpy as np
import pytest

import srbd_oracle as orc
import degenerate_twin as dt
import rank_aware_twin as rt

FORCE_BOUND = dt.BOUND["f64"] / 5                                   # 1e-2 N


@functools.lru_cache(maxsize=None)
def _dense(name, restart):
    """Per rung: the dense twin's result and the exact forces (N, 12)."""
    N = dt.BATCHES[name]["N"]
    kw = dict(zip(("rho_restart_iter", "rho_restart_count"), orc.default_restart(N))) if restart else {}
    p = dt.params(N, "f64", **kw)
    x0, xr, ft, ct, meta = dt.inputs(name)
    out = []
    for b in range(len(meta)):
        dense = orc.update(p, x0[b], xr[b], ft[b], ct[b])
        xs, _ = orc.solve_reference(p, dense["qp"])
        out.append((dense, (xs * p.force_scale).reshape(N, 12)))
    return out, p


def _check_ladder(name, restart):
    refs, p = _dense(name, restart)
    x0, xr, ft, ct, meta = dt.inputs(name)
    below = 0
    for b, (g, eps) in enumerate(meta):
        dense, us = refs[b]
        o = rt.update_rank_aware(p, x0[b], xr[b], ft[b], ct[b])
        err = float(np.abs(o["u"] - us).max())
        tag = (name, b, g, eps, err, o["iters"], dense["iters"])
        assert o["status"] == orc.STATUS_SOLVED and dense["status"] == orc.STATUS_SOLVED, tag
        assert err <= FORCE_BOUND, tag
        assert o["iters"] == dense["iters"], tag
        assert np.all(np.isfinite(o["x"])) and np.all(o["u"].reshape(-1)[np.setdiff1d(np.arange(o["u"].size), orc.presolve(o["qp"], ct[b])[1])] == 0.0), tag
        below += bool(o["ra_steps"][0])
    return below


@pytest.mark.parametrize("name", list(dt.BATCHES))
def test_twin_answers_every_rung(name):
    below = _check_ladder(name, False)
    assert below >= 2, (name, below)                                   # (both geometries have their exactly collinear rung)


@pytest.mark.parametrize("name", list(dt.BATCHES))
def test_twin_answers_every_rung_with_the_restart_rule(name):
    N = dt.BATCHES[name]["N"]
    r_iter, _ = orc.default_restart(N)
    assert 0 < r_iter < orc.params_for(N).max_iter
    _check_ladder(name, True)


def test_the_ladders_reach_below_the_guard():
    total = below = refused = 0
    for name, d in dt.BATCHES.items():
        x0, xr, ft, ct, meta = dt.inputs(name)
        p = dt.params(d["N"], "f64")
        for b in range(len(meta)):
            w = rt.rank_aware_reduce(p, xr[b], ft[b], ct[b])
            total += 1
            below += bool(w["ra_steps"])
            refused += not w["pivot_ratio"] > orc.GUARD_RATIO_F64
            assert bool(w["ra_steps"]) == (not w["pivot_ratio"] > rt.SELECT_RATIO)
    assert (total, below, refused) == (148, 105, 82)            # (what the guard refuses is a subset of what takes the new path)
    assert orc.GUARD_RATIO_F64 < rt.SELECT_RATIO < 30 * orc.GUARD_RATIO_F32   # ... which stays below the healthy stances (test_degenerate_contacts_cpu.py)


def test_without_a_step_to_normalise_the_reduction_is_wrench_reduce():
    for name, d in dt.BATCHES.items():
        x0, xr, ft, ct = dt.healthy(name)
        p = dt.params(d["N"], "f64")
        for b in range(0, x0.shape[0], 5):
            w0 = orc.wrench_reduce(p, xr[b], ft[b], ct[b])
            w1 = rt.rank_aware_reduce(p, xr[b], ft[b], ct[b])
            assert w1["ra_steps"] == [] and w1["dropped"] == 0
            for k in ("T", "V", "Bd", "D", "S", "goff", "gsz"):
                assert np.array_equal(w0[k], w1[k]), (name, b, k)


def test_normalised_steps_have_orthonormal_rows_and_the_same_inverse():
    """V D^1/2 has orthonormal rows on a normalised step -- to the rounding of its smallest pivot, 2^-52 / ratio --, both reductions apply the same K^-1 where the
    plain coordinates are still accurate (every wrench step normalised on a rung far above the guard), and a dropped pivot leaves a zero row of V and an
    identity row of T."""
    x0, xr, ft, ct, meta = dt.inputs("n10_three")
    p = dt.params(10, "f64")
    ulp = 2.0 ** -52
    for eps, every in ((1e-1, True), (1e-4, False)):
        b = [i for i, (g, e) in enumerate(meta) if g == 0 and e == eps][0]
        w0 = orc.wrench_reduce(p, xr[b], ft[b], ct[b])
        w1 = rt.rank_aware_reduce(p, xr[b], ft[b], ct[b], every_step=every)
        assert len(w1["ra_steps"]) >= 6 and w1["dropped"] == 0
        uoff = np.concatenate([[0], np.cumsum(3 * w1["csz"])])
        for k in w1["ra_steps"]:
            gs, us = slice(w1["goff"][k], w1["goff"][k + 1]), slice(uoff[k], uoff[k + 1])
            Vk = w1["V"][gs, us] * np.sqrt(w1["D"][us])
            assert np.abs(Vk @ Vk.T - np.eye(6)).max() <= 16 * ulp / w0["pivot_ratio"], (eps, k)
        if every:
            assert w0["pivot_ratio"] > 1e3 * orc.GUARD_RATIO_F64
            rhs = np.random.default_rng(3).standard_normal(w0["V"].shape[1])
            k0, k1 = orc.wrench_kinv_op(w0)(rhs), orc.wrench_kinv_op(w1)(rhs)
            assert np.abs(k0 - k1).max() <= 1e-9 * np.abs(k0).max()
    b0 = [i for i, (g, e) in enumerate(meta) if g == 0 and e == 0.0][0]          # exactly collinear: one pivot per step at rounding level
    w2 = rt.rank_aware_reduce(p, xr[b0], ft[b0], ct[b0])
    if w2["dropped"]:
        rows = [r for r in range(w2["n_g"]) if not w2["V"][r].any()]
        assert len(rows) == w2["dropped"]
        for r in rows:
            e = np.zeros(w2["n_g"]); e[r] = 1.0
            assert np.array_equal(w2["T"][r], e)


def test_truncating_at_the_guard_is_wrong():
    """Why a column is dropped at rounding level only: dropped at the guard's threshold, the torque about the contact line goes missing and the forces are
    newtons off (DESIGN.md has the table)."""
    x0, xr, ft, ct, meta = dt.inputs("n10_three")
    refs, p = _dense("n10_three", False)
    worst = 0.0
    for b, (g, eps) in enumerate(meta):
        if g == 0 and 0.0 < eps <= 1e-4:
            o = rt.update_rank_aware(p, x0[b], xr[b], ft[b], ct[b], drop=orc.GUARD_RATIO_F64)
            worst = max(worst, float(np.abs(o["u"] - refs[b][1]).max()))
    assert worst > 10 * FORCE_BOUND, worst


def test_flag_constant_and_keyword_plumbing():
    from g1_locomotion_amd import _lib, MPC, BatchMPC, RaggedMPC, SrbdqpError
    assert _lib.FLAG_RANK_AWARE == 256
    flags = [v for k, v in vars(_lib).items() if k.startswith("FLAG_")]
    assert len(set(flags)) == len(flags)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srbdqp.h")).read()
    assert "#define SRBDQP_FLAG_RANK_AWARE 256" in hdr
    m = MPC(horizon=10, rank_aware=True)
    assert m._overrides["rank_aware"] is True and "rank_aware" not in MPC(horizon=10)._overrides
    # srbdqp_create refuses the flag where no instantiation exists before it looks for a device: N = 24, a live horizon -- by keyword and through flags=
    for kw in (dict(horizon=24, rank_aware=True), dict(horizon=24, flags=_lib.FLAG_RANK_AWARE), dict(horizon=7, rank_aware=True)):
        with pytest.raises(SrbdqpError, match="SRBDQP_FLAG_RANK_AWARE"):
            BatchMPC(**kw)
    with pytest.raises(SrbdqpError, match="SRBDQP_FLAG_RANK_AWARE"):
        RaggedMPC(horizons=(8, 12), flags=_lib.FLAG_RANK_AWARE)
