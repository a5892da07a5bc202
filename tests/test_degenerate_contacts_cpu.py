"""Nearly collinear stance contacts on the oracle's twin of the general kernel (orc.update_split = wrench_reduce + admm_solve_split), without a GPU.

The step coordinates of the general kernel lose rank when a step's stance contact points lie on one line (E = Y D^-1 Y' has rank 5), while the QP stays
well posed: the dense path solves every rung below.  Without the conditioning guard the twin returns SOLVED with forces newtons away from the optimum, or
raises LinAlgError; with it every QP is either answered within the suite's bounds or rejected with STATUS_NUMERICAL and zero forces
(tests/degenerate_twin.py states the contract).  The same ladders run on the GPU in tests/test_gpu_degenerate_contacts.py; the counts asserted here keep a
later change of the generators from hollowing that test out.
"""
import numpy as np
import pytest

import srbd_oracle as orc
import scenarios as sc
import degenerate_twin as dt


def test_collinear_contacts_generator():
    x0, xr, ft, ct = orc.synthetic_batch(1, 6, 11, "mixed")
    ws = sc.wrench_steps(ct[0])
    assert ws and len(ws) < 6                                   # wrench steps next to identity-coordinate steps
    for kind in sc.COLLINEAR_KINDS:
        for eps in (1e-2, 0.0):
            f = sc.collinear_contacts(ft[0], ct[0], eps, kind, ws[:1]).reshape(6, 4, 3)
            other = [k for k in range(6) if k != ws[0]]
            assert np.array_equal(f[other], ft[0].reshape(6, 4, 3)[other])          # only the chosen step moves
            assert np.array_equal(f[ws[0], :, 2], ft[0].reshape(6, 4, 3)[ws[0], :, 2])
            pts = f[ws[0], :, :2]
            d = (pts[2] - pts[0]) if kind == "point" else (pts[1] - pts[0])
            d = d / np.linalg.norm(d)
            off = np.abs((pts - pts[0]) @ np.array([-d[1], d[0]]))               # distance of every point from the line
            assert off.max() <= eps * (1 + 1e-9) + 1e-15 and (eps == 0.0 or off.max() >= eps * (1 - 1e-9))
    with pytest.raises(ValueError):
        sc.collinear_contacts(ft[0], ct[0], 1e-3, "sideways")


def test_exactly_collinear_raises_nothing_and_is_rejected():
    """eps = 0: np.linalg.inv(E) raises LinAlgError (or returns 1e16) -- neither may leave wrench_reduce() or update_split()."""
    for name in ("n4_double", "n10_three"):
        x0, xr, ft, ct, meta = dt.inputs(name)
        N = dt.BATCHES[name]["N"]
        for b, (g, eps) in enumerate(meta):
            if eps != 0.0:
                continue
            for dtype in (np.float64, np.float32):
                with np.errstate(all="ignore"):
                    wr = orc.wrench_reduce(orc.params_for(N), xr[b], ft[b], ct[b])
                    assert not wr["pivot_ratio"] > orc.guard_ratio(dtype)
                    out = orc.update_split(orc.params_for(N), x0[b], xr[b], ft[b], ct[b], dtype=dtype)
                assert out["status"] == orc.STATUS_NUMERICAL and out["iters"] == 0
                assert np.all(out["u"] == 0.0) and np.all(out["y"] == 0.0) and np.all(np.isfinite(out["x"]))


# (batch, mode) -> free-ok rungs the guard refuses (degenerate_twin.py: OVER-REJECTED); every other case has none
OVER_REJECTED = {("n4_double", "f64"): 3, ("n10_mixed", "f64"): 3, ("n10_three", "f64"): 1, ("n10_double", "f64"): 3, ("n10_double", "f32"): 2,
                 ("n7_mixed", "f64"): 3, ("n8_mixed", "f64"): 3, ("n12_mixed", "f64"): 1}


@pytest.mark.parametrize("name,mode", dt.CASES)
def test_guarded_twin_answers_or_rejects(name, mode):
    refs, p = dt.reference(name, mode)                          # (raises where the dense twin is no reference for a rung)
    x0, xr, ft, ct, meta = dt.inputs(name)
    thr = dt.threshold(mode)
    full = len(dt.rungs_of(name)) == len(sc.EPS_LADDER)
    for g in range(len(dt.BATCHES[name]["geoms"])):
        mine = [r for r in refs if r["geom"] == g]
        n_must, n_bad = sum(r["must_answer"] for r in mine), sum(r["bad"] for r in mine)
        # the balance of a ladder: enough rungs that have to be answered, enough on which the algorithm without the guard is wrong.  (The 4-rung ladder of
        # N = 20 -- 1e-1, 1e-3, 1e-5, 0 -- has one rung of the first kind in fp32 and two of the second: what its four rungs can give.)
        assert n_must >= ((4 if mode == "f64" else 2) if full else 1), (name, mode, g, n_must)
        assert n_bad >= (3 if full else 2), (name, mode, g, n_bad)
    for b, r in enumerate(refs):
        tag = (name, mode, b, r["eps"])
        # no rung inside the band where kernel and twin may decide differently
        assert not (thr / 4 <= r["ratio"] <= 4 * thr), (tag, r["ratio"], thr)
        # the guard rejects exactly below the threshold, and rejects every rung on which the unguarded algorithm is wrong
        o = r["guarded"]
        assert (o["status"] == orc.STATUS_NUMERICAL) == (not r["ratio"] > thr), (tag, o["status"], r["ratio"])
        kind = dt.check_contract(tag, o["u"], o["x"], o["y"], o["status"], o["iters"], r, ct[b], p, mode, x0[b] if mode == "f64" else np.float32(x0[b]).astype(np.float64))
        if r["must_answer"]:
            assert kind == "answered", tag
    # what the geometry-only guard costs: rungs the algorithm without it would have answered well and the guard refuses (pinned, so that a change of the
    # thresholds or of the generators shows here)
    assert sum(r["over_rejected"] for r in refs) <= OVER_REJECTED.get((name, mode), 0), [(r["eps"], r["geom"]) for r in refs if r["over_rejected"]]


def test_restart_passes_keep_a_rejection():
    """The automatic rho restart on: a rejected QP stays rejected (zero forces, iters 0), an answered one keeps the contract."""
    refs, p = dt.reference("n10_mixed", "f64", restart=True)
    assert 0 < p.rho_restart_iter < p.max_iter
    x0, xr, ft, ct, meta = dt.inputs("n10_mixed")
    kinds = {dt.check_contract(("restart", b), r["guarded"]["u"], r["guarded"]["x"], r["guarded"]["y"], r["guarded"]["status"], r["guarded"]["iters"], r, ct[b], p, "f64", x0[b])
             for b, r in enumerate(refs)}
    assert kinds == {"answered", "rejected"}


def test_healthy_stances_pass_the_guard():
    """The undeformed QPs that the GPU test interleaves with the ladders: ratios two orders of magnitude above the fp32 threshold."""
    for name, d in dt.BATCHES.items():
        x0, xr, ft, ct = dt.healthy(name)
        for b in range(x0.shape[0]):
            assert orc.wrench_reduce(orc.params_for(d["N"]), xr[b], ft[b], ct[b])["pivot_ratio"] > 30 * orc.GUARD_RATIO_F32
