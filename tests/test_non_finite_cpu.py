"""The poison table and the contract checker of tests/non_finite.py, validated without a GPU.

What the oracles return for a QP with a non-finite main input (measured here, N = 10, "single" and "mixed", orc.update and orc.update_split):
  * NaN or Inf in x0, x_ref, a stance foot or pcom: status -1 with NaN forces and iters = 250 -- the residual pre-test `max |A x - z| <= e_prim_last` is False
    for NaN, so no full check runs before the iteration cap;
  * 1e200 in x0 or x_ref: status -1 at iteration 5 with forces of order 1e201 N;
  * NaN, Inf or 1e200 in a SWING foot: status 1 at 30 iterations with the forces of the clean QP -- and a NaN roll-out, since orc.rollout multiplies the
    swing contact's column of B_qp (NaN) by its exact zero force.
So the oracle is not the reference for a rejected QP: include/srbdqp.h is (zero forces, at most the first check).  Its status alone is compared here (-1 for
every "rejects" row: the table does not ask a kernel to reject what the algorithm could answer); its forces and iteration count are not.  The oracle IS the
reference for the columns of the table: which rows are harmless, and which entries the zero-force roll-out reads."""
import numpy as np
import pytest

import non_finite as nf
import srbd_oracle as orc

ALL_CASES = nf.CASES + nf.RESTART_CASES
PLAIN_CASES = [c for c in ALL_CASES if not c.sides and not c.rank_aware]


# ---- check_contract rejects what it must ----------------------------------------------------------------------------------------------------------
def _fabricated(f32=False):
    """A clean output set of 5 QPs, N = 4, and a conforming poisoned one: QP 2 rejected by a row whose roll-out does not read the poison, QP 4 by x0."""
    rng = np.random.default_rng(3)
    fl = np.float32 if f32 else np.float64
    B, N = 5, 4
    clean = dict(u=rng.normal(size=(B, N, 12)).astype(fl), x=rng.normal(size=(B, N + 1, 13)).astype(fl), y=rng.normal(size=(B, 20 * N)).astype(fl),
                 status=np.ones(B, np.int32), iters=np.full(B, 30, np.int32))
    out = {k: v.copy() for k, v in clean.items()}
    zero = rng.normal(size=(N + 1, 13))
    x0 = rng.normal(size=(B, 13))
    x0[4, 4] = np.nan
    for b in (2, 4):
        out["u"][b] = 0.0; out["y"][b] = 0.0; out["status"][b] = nf.NUMERICAL
    out["iters"][2], out["iters"][4] = 0, 5
    out["x"][2] = zero.astype(fl)
    out["x"][4] = np.nan
    out["x"][4][0] = x0[4].astype(fl)
    bad = {2: nf.ROW["foot_stance_ge3"], 4: nf.ROW["x0_pos"]}
    kw = dict(x0=x0, zero_x=lambda b: zero, f32=f32)
    return out, clean, bad, orc.params_for(N), kw


@pytest.mark.parametrize("f32", [False, True])
def test_check_contract_passes_a_conforming_output(f32):
    out, clean, bad, p, kw = _fabricated(f32)
    assert nf.check_contract(out, clean, bad, p, **kw) == {2: 0, 4: 5}
    out["status"][1] = nf.PENDING
    with pytest.raises(AssertionError):
        nf.check_contract(out, clean, bad, p, **kw)
    clean["status"][1] = nf.PENDING
    nf.check_contract(out, clean, bad, p, allow_pending=True, **kw)


def _nan_in_u(o, c):
    o["u"][2][1, 3] = np.nan


def _tiny_force(o, c):
    o["u"][4][0, 0] = 1e-300


def _dual_left(o, c):
    o["y"][2][7] = -1e-300


def _neighbour_ulp(o, c):
    o["u"][3][2, 5] = np.nextafter(o["u"][3][2, 5], np.inf)


def _neighbour_x_ulp(o, c):
    o["x"][1][4, 0] = np.nextafter(o["x"][1][4, 0], -np.inf)


def _neighbour_iters(o, c):
    o["iters"][0] += 5


def _sentinel_in_x(o, c):
    o["x"][4][3, 7] = nf.SENTINEL


def _iters_at_cap(o, c):
    o["iters"][4] = 250


def _rejected_pending(o, c):
    o["status"][2] = nf.PENDING


def _rejected_solved(o, c):
    o["status"][2] = nf.SOLVED


def _nan_rollout(o, c):
    o["x"][2][2, 6] = np.nan


def _rollout_off(o, c):
    o["x"][2][2, 6] += 1e-8


def _x0_row_changed(o, c):
    o["x"][4][0, 4] = 0.0


DEFECTS = [_nan_in_u, _tiny_force, _dual_left, _neighbour_ulp, _neighbour_x_ulp, _neighbour_iters, _sentinel_in_x, _iters_at_cap, _rejected_pending, _rejected_solved,
           _nan_rollout, _rollout_off, _x0_row_changed]


@pytest.mark.parametrize("defect", DEFECTS, ids=[d.__name__.strip("_") for d in DEFECTS])
def test_check_contract_fails_on(defect):
    """One fabricated defect each: a NaN left in u, a force of 1e-300, a neighbour off by one ulp, a sentinel left in x, iters == max_iter, a rejected QP marked
    PENDING, and the checker's other clauses."""
    out, clean, bad, p, kw = _fabricated()
    defect(out, clean)
    with pytest.raises(AssertionError):
        nf.check_contract(out, clean, bad, p, allow_pending=True, **kw)


# ---- the table's columns, derived from the oracle --------------------------------------------------------------------------------------------------
def _distinct(cases, key):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


BATCHES = _distinct(PLAIN_CASES, lambda c: (c.N, c.schedule))           # every schedule and horizon the GPU file uses


@pytest.mark.parametrize("case", BATCHES, ids=lambda c: f"n{c.N}_{c.schedule}")
def test_harmless_rows_do_not_reach_the_oracles_qp(case):
    """A swing contact's foot position, NaN / +-Inf / 1e39: orc.update and orc.update_split (fp64, fp32) return bit-identical forces, duals, status and iteration
    count with and without it.  Their roll-out does not -- orc.rollout multiplies the swing contact's column of B_qp by its zero force, and NaN * 0 is NaN; the
    oracles stay as they are -- so x is held to what the oracle's roll-out IS on the variables that exist: every column of the stance variables, and the
    free response, are bit-identical, and the swing variables are exact zeros."""
    d = nf.arrays(case)
    rows = [r for r in nf.ROWS + nf.LIVE_ROWS if not r.rejects]
    p = nf.params(case)
    for row in rows:
        for b in case.bad_qps:
            if nf.index_of(case, row, b) is None:
                continue
            a = (d["x0"][b], d["x_ref"][b], d["foot"][b], d["contact"][b])
            clean = [orc.update(p, *a), orc.update_split(p, *a, dtype=np.float64), orc.update_split(p, *a, dtype=np.float32)]
            for value in nf.F32_VALUES.values():
                e = nf.poisoned(case, [(b, row, value)])
                a2 = (e["x0"][b], e["x_ref"][b], e["foot"][b], e["contact"][b])
                got = [orc.update(p, *a2), orc.update_split(p, *a2, dtype=np.float64), orc.update_split(p, *a2, dtype=np.float32)]
                for c, g in zip(clean, got):
                    for k in ("u", "y", "iters", "status"):
                        assert nf.same_bits(np.asarray(c[k]), np.asarray(g[k])), (row.name, b, value, k)
                    vi = orc.presolve(c["qp"], d["contact"][b])[1]
                    off = np.setdiff1d(np.arange(12 * case.N), vi)
                    assert nf.same_bits(c["qp"]["B_qp"][:, vi], g["qp"]["B_qp"][:, vi]) and nf.same_bits(c["qp"]["A_qp"], g["qp"]["A_qp"]), (row.name, b, value)
                    assert np.all(g["u_hat"][off] == 0.0), (row.name, b, value)
                    # x: the rows up to the poisoned step k (x_0 .. x_k: B_k is the first block the position enters) bit for bit, and the roll-out formed from
                    # the stance variables only -- what orc.rollout computes but for the zero terms -- bit for bit and finite
                    k = nf.index_of(case, row, b)[0]
                    assert nf.same_bits(c["x"][:k + 1], g["x"][:k + 1]), (row.name, b, value)
                    stance = [o["qp"]["A_qp"] @ d["x0"][b] + (o["qp"]["B_qp"][:, vi] * p.force_scale) @ o["u_hat"][vi] for o in (c, g)]
                    assert nf.same_bits(stance[0], stance[1]) and np.isfinite(stance[1]).all(), (row.name, b, value)


@pytest.mark.parametrize("case", BATCHES, ids=lambda c: f"n{c.N}_{c.schedule}")
def test_which_entries_the_zero_force_rollout_reads(case):
    """Every row of the table, the entry replaced by two different finite values: the oracle's zero-force roll-out is bit-identical where the row says the
    roll-out does not read it (that licenses check_contract's comparison of x with the roll-out of the CLEAN inputs), and differs where the row says it does."""
    for row in nf.ROWS + nf.LIVE_ROWS[1:]:
        for b in case.bad_qps:
            if nf.index_of(case, row, b) is None:
                continue
            base = nf.zero_rollout(case, nf.arrays(case), b, row.needs)
            if row.needs == "warm":   # (zero_rollout takes no start: that the oracle's solve without a stance contact reads none is asserted on orc.update itself)
                e = [nf.poisoned(case, [(b, row, v)]) for v in (0.37, -7.25)]
                xs = [orc.update(nf.params(case), v["x0"][b], v["x_ref"][b], v["foot"][b], np.zeros_like(v["contact"][b]),
                                 warm=(v["warm_u"][b] / 100.0, v["warm_y"][b]))["x"] for v in e]
            else:
                xs = [nf.zero_rollout(case, nf.poisoned(case, [(b, row, v)]), b, row.needs) for v in (0.37, -7.25)]
            if row.rollout_reads:
                assert not np.array_equal(xs[0], xs[1]), (row.name, b)
            else:
                assert nf.same_bits(xs[0], xs[1]) and (row.needs == "warm" or nf.same_bits(xs[0], base)), (row.name, b)


@pytest.mark.parametrize("case", PLAIN_CASES, ids=lambda c: c.id)
def test_the_oracle_rejects_every_rejects_row(case):
    """Status -1 from the case's own oracle for every "rejects" row and value the case takes.  Run at a cap of two check intervals: a finite QP ends there with
    MAX_ITER (asserted for the clean one), so -1 is the oracle's finding of a non-finite residual; at the full cap it is the same finding 240 iterations later
    (the module docstring).  Forces and iteration count of the oracle are not compared: it is not the reference for a rejected QP."""
    p = nf.params(case, max_iter=10, rho_restart_iter=0)
    b = case.bad_qps[1]
    rows = nf.rows_of(case) if case in nf.CASES else [(r, "nan") for r in nf.restart_rows(case)]
    for needs in sorted({r.needs for r, _ in rows}):
        assert nf.oracle(case, nf.arrays(case), b, needs, p)["status"] == nf.MAX_ITER
    for row, vname in rows:
        if not row.rejects or nf.index_of(case, row, b) is None:
            continue
        with np.errstate(all="ignore"):
            o = nf.oracle(case, nf.poisoned(case, [(b, row, nf.F32_VALUES[vname])]), b, row.needs, p)
        assert o["status"] == nf.NUMERICAL, (row.name, vname, o["status"])


# ---- the cases stay honest as neighbour tests -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PLAIN_CASES, ids=lambda c: c.id)
def test_every_clean_qp_is_solved_and_the_restart_cases_restart(case):
    """Every QP of every clean batch ends SOLVED in the oracle, in each kind of call the case makes (plain, with pcom, from the warm arrays); every QP of a
    restart case is past the first restart mark."""
    d = nf.arrays(case)
    restart = case in nf.RESTART_CASES
    kinds = ("plain", "warm") if restart else (("plain", "pcom", "warm") if case.full else ("plain",))
    for needs in kinds:
        outs = [nf.oracle(case, d, b, needs) for b in range(case.B)]
        assert all(o["status"] == nf.SOLVED for o in outs), (needs, [o["status"] for o in outs])
        if restart:
            assert all(o["iters"] > dict(case.cfg)["rho_restart_iter"] for o in outs), (needs, [o["iters"] for o in outs])


def test_every_case_poisons_first_middle_and_last_and_names_its_rows():
    for case in ALL_CASES:
        assert case.bad_qps == (0, case.B // 2, case.B - 1) and 0 < case.B // 2 < case.B - 1
        assert nf.rows_of(case)
    full = [c for c in nf.CASES if c.full]
    assert {c.twin for c in full} == {"dense", "wrench"} and any(c.f32 for c in full)
    for c in full:                                                     # a family that takes the whole table sees every row in one of its cases
        fam = [k for k in full if k.name.split("_n")[0] == c.name.split("_n")[0]]
        assert {r.name for k in fam for r, _ in nf.rows_of(k)} == {r.name for r in nf.ROWS}, c.id
