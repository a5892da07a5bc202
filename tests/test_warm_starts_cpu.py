"""The inputs of tests/test_gpu_warm_starts.py, fixed on the twins alone: the conditions that keep the GPU tests from passing vacuously, with the seeds and
cases those tests use (tests/warm_starts.py CASES).

  * every one-interval twin run ends at its cap with status MAX_ITER (so kernel and twin are compared at equal counts, on an iterate that is still moving);
  * its forces from the shifted start differ from the cold ones by more than 1 N on every QP (a kernel that ignores the start cannot meet 1e-4 N);
  * at least a quarter of the QPs of a case carry more than 10 N of warm_u on a contact that swings now (full double support has none: exempt);
  * the dual start matters on at least one QP of a case (a kernel that drops warm_y cannot meet the bar either);
  * the junk on swing-contact entries changes nothing in the twin, bit for bit;
  * si.twin and rank_aware_twin.update_rank_aware without the keyword are what they were;
  * a full solve from the neighbour's start ends at another count than the cold one on at least half of the QPs of a case (the counts can tell a start apart);
  * the twin's own full solves from the foreign starts stop within 0.8 of the exact-optimum bar (the bar then measures the kernel, not the stopping rule).
"""
from dataclasses import replace

import numpy as np
import pytest

import rank_aware_twin as rt
import side_inputs as si
import srbd_oracle as orc
import warm_starts as ws

by_case = pytest.mark.parametrize("case", ws.CASES, ids=lambda c: c.id)


@by_case
def test_one_interval_runs_are_sharp(request, case):
    if "robots" in case.sides:                                       # (robot records come from robots_array(), which reads the library's default config)
        request.getfixturevalue("built_lib")
    d = ws.inputs(case)
    B = d["x0"].shape[0]
    WU, WY = ws.starts(case)
    cold, warm, junk = (ws.interval_twins(case, s) for s in ("cold", "shifted", "junk"))
    moved = [float(np.abs(warm[b]["u"] - cold[b]["u"]).max()) for b in range(B)]
    swing = [ws.swing_force(WU[b], d["contact"][b]) for b in range(B)]
    print(f"{case.id}: shifted vs cold after {case.iters} iterations {min(moved):.1f} ... {max(moved):.1f} N, |warm_u| on swing contacts up to {max(swing):.1f} N "
          f"({sum(s > 10.0 for s in swing)} of {B} QPs above 10 N)")
    for b in range(B):
        assert warm[b]["status"] == cold[b]["status"] == orc.STATUS_MAX_ITER and warm[b]["iters"] == cold[b]["iters"] == case.iters, (b, warm[b]["iters"])
        assert moved[b] > 1.0, (b, moved[b])
        for k in ("u", "y"):
            assert np.array_equal(junk[b][k], warm[b][k]), (b, k)
        assert junk[b]["iters"] == warm[b]["iters"] and junk[b]["status"] == warm[b]["status"]
    if not np.all(d["contact"] != 0):
        assert 4 * sum(s > 10.0 for s in swing) >= B, swing
    # ... and the dual start matters: without warm_y the same run ends more than 0.1 N away (1000 x the bar) on at least one QP (N = 4: the short horizons
    # seldom leave a row active, and the seeds of those cases were chosen for it)
    no_y = [float(np.abs(ws.twin(case.path, ws.params(case, b), ws.qp_of(case, b), (WU[b], np.zeros_like(WY[b])))["u"] - warm[b]["u"]).max()) for b in range(B)]
    print(f"{case.id}: without warm_y the forces move by up to {max(no_y):.2f} N")
    assert max(no_y) > 0.1, no_y
    if "rho_restart_iter" in dict(case.cfg):
        # (wave_defer_*: a re-balancing follows the first interval.  Its rho comes from the check's maxima, and a primal residual at rounding level -- no row of the
        #  start active: 9e-16 on one QP of seed 9110 -- is 0 on one side and not on the other; the case's seed keeps every QP's residuals far above that)
        for b in range(B):
            q, p = ws.qp_of(case, b), ws.params(case, b)
            red, vi, ri = orc.presolve(warm[b]["qp"], q["contact"])
            info = {}
            orc.admm_solve(replace(p, max_iter=p.rho_restart_iter, rho_restart_iter=0), red["P"], red["q"], red["A"], red["l"], red["u"],
                           (WU[b] / p.force_scale)[vi], WY[b][ri], info=info)
            assert info["r_prim"] > 1e-4 * info["n_prim"] and info["r_dual"] > 1e-4 * info["n_dual"], (b, info)
    jU, jY = ws.with_junk(WU, WY, d["contact"])
    assert np.all(np.isfinite(jU)) and np.all(np.isfinite(jY))
    off = np.repeat(d["contact"].reshape(B, -1) == 0, 3, axis=1)
    assert np.array_equal(jU[~off], WU[~off]) and (not off.any() or np.abs(jU[off]).min() > 0.5 * ws.JUNK)


@pytest.mark.parametrize("cid", ws.FULL_CASES)
def test_full_solves_from_the_neighbour_end_at_other_counts(cid):
    case = ws.BY_ID[cid]
    rst = ws.restarts(case)
    cold, nb = ws.full_twins(case, "cold", rst), ws.full_twins(case, "neighbour", rst)
    other = sum(int(a["iters"] != b["iters"]) for a, b in zip(cold, nb))
    print(f"{cid}: cold {[r['iters'] for r in cold]}, from the neighbour {[r['iters'] for r in nb]}")
    assert 2 * other >= len(cold), (other, len(cold))
    # ... and the twin's own stopping point from either foreign start is well inside the exact bar, so that bar measures the kernel and not the stopping rule
    # (drawn weights move that point: the weights records' seed was chosen for it, tests/warm_starts.py WEIGHTS_SEED)
    gaps = []
    for start in ("shifted", "neighbour"):
        for b, r in enumerate(ws.full_twins(case, start, rst)):
            assert r["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER)
            if r["status"] == orc.STATUS_SOLVED:
                p = ws.params(case, b, full=True, restart=rst)
                xs, _ = orc.solve_reference(p, r.get("qp_loc", r["qp"]))
                gaps.append(float(np.abs(r.get("u_loc", r["u_hat"]) - xs).max()) * p.force_scale)
    print(f"{cid}: the twin's full solves stop within {max(gaps):.2e} N of the exact optimum")
    assert max(gaps) <= 0.8 * (ws.TOL32_EXACT_N if case.f32 else ws.TOL_EXACT_N), max(gaps)


def test_twins_without_the_keyword_are_unchanged(built_lib):
    """warm=None is the call without the keyword, bit for bit; and a start changes the result (the keyword is read)."""
    for cid in ("normals_n10_mixed", "combined_n16_mixed", "rank_aware_n10_mixed"):
        case = ws.BY_ID[cid]
        b = 1
        q, p = ws.qp_of(case, b), ws.params(case, b)
        a = (q["x0"], q["x_ref"], q["foot"], q["contact"])
        if case.path == "side":
            kw = {k: q[k] for k in ("normals", "ext_wrench") if k in q}
            plain, none = si.twin(p, *a, **kw), si.twin(p, *a, **kw, warm=None)
        else:
            plain, none = rt.update_rank_aware(p, *a), rt.update_rank_aware(p, *a, warm=None)
        for k in ("u", "x", "y"):
            assert np.array_equal(plain[k], none[k]), (cid, k)
        assert plain["iters"] == none["iters"] and plain["status"] == none["status"]
        assert np.array_equal(plain["u"], ws.interval_twins(case, "cold")[b]["u"])
        assert not np.array_equal(plain["u"], ws.interval_twins(case, "shifted")[b]["u"])


def test_a_start_under_normals_is_taken_in_the_world_frame():
    """si.twin(warm=) from its own solution u (world newtons) and y stops at the first check: the start was turned into the contacts' frames."""
    case = ws.BY_ID["normals_n10_mixed"]
    b = 0
    q, p = ws.qp_of(case, b), ws.params(case, b, full=True)
    own = ws.full_twins(case, "cold")[b]
    again = ws.twin("side", p, q, (own["u"].reshape(-1), own["y"]))
    assert own["status"] == orc.STATUS_SOLVED and again["status"] == orc.STATUS_SOLVED and again["iters"] == p.check_every < own["iters"]


def test_the_ladder_case_reaches_below_the_guard():
    case = ws.BY_ID["rank_aware_n10_ladder"]
    d = ws.inputs(case)
    p = ws.params(case, 0)
    with np.errstate(all="ignore"):
        ratios = [orc.wrench_reduce(p, d["x_ref"][b], d["foot"][b], d["contact"][b])["pivot_ratio"] for b in range(d["x0"].shape[0])]
    assert sum(not r > orc.GUARD_RATIO_F64 for r in ratios) >= 2, ratios
