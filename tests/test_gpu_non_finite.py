"""GPU tests of the non-finite-input contract of include/srbdqp.h, table-driven over tests/non_finite.py: a QP whose main inputs (x0, x_ref, foot, pcom,
warm_u, warm_y) are not finite ends with SRBDQP_NUMERICAL, forces and duals exactly 0, iters 0 or the first check, x the zero-force roll-out (where the roll-out
does not read the poison) -- and every other QP of the batch, and a QP poisoned on a swing contact's foot position only, equals the clean solve bit for bit.
The reference for the rejected QP is the header; the oracle is the reference for its surroundings (tests/test_non_finite_cpu.py).

Every case poisons the first QP, one in the middle and the last (where the row has an entry in them), runs a device-buffer call into outputs prefilled
with the sentinel 12345.0 and a host-buffer call, and asserts the kernel name it ran.

WHERE a poisoned QP is caught, per array (AT_FIRST_CHECK below: the iters the kernels report, asserted; the same for every family, since every kernel forms the same
quantities from each array):
  array                      caught                                                                                            iters
  x0                         first residual check (x0 enters the gradient and the roll-out only: the factorisation never sees it)  check_every
  x_ref, an entry that is    first residual check (gradient only; xref_last poisons an angular velocity of the last step)     check_every
  neither yaw nor CoM
  x_ref, CoM (no pcom given) before the iterations: the lever arms' origin, like pcom (row xref_com_last)                      0
  x_ref, CoM (pcom given)    first residual check: a tracking target only (row xref_com_pcom)                                  check_every
  x_ref, yaw                 before the iterations: the frames R_z(yaw) go into every lever arm -- the conditioning guard of    0
                             phase E (general kernel, a step with >= 3 stance contacts) or a non-positive pivot (T; K of the
                             dense kernels)
  foot (stance), pcom        before the iterations, the same way: guard (>= 3 stance contacts) or pivot (<= 2; dense kernels)   0
  warm_u, warm_y             first residual check (the start enters the iterates only)                                        check_every
  foot (swing)               never: not read
The two-phase call's PREDICTED x0 enters the gradient like x0 (first check); its roll-out starts from the measured state.
"""
import os

import numpy as np
import pytest

import non_finite as nf
import side_inputs as si
from gpu_helpers import sentinel_solve, torch_first  # noqa: F401  (torch_first: the fixture)

pytestmark = pytest.mark.gpu

# iters of a rejected QP, by the poisoned row (measured on the GPU, see the table above); every other row: 0
AT_FIRST_CHECK = ("x0_pos", "x0_vel", "xref_last", "xref_com_pcom", "warm_u", "warm_y", "x0_predicted")


def expected_iters(row, p):
    return p.check_every if row.name in AT_FIRST_CHECK else 0


def make_engine(case, **more):
    from g1_locomotion_amd import BatchMPC, _lib
    kw = dict(case.cfg)
    kw.setdefault("rho_restart_iter", -1)
    flags = 0
    for f in case.flags:
        flags |= getattr(_lib, "FLAG_" + f)
    if flags:
        kw["flags"] = flags
    kw.update(more)
    eng = BatchMPC(horizon=case.N, kernel=getattr(_lib, "KERNEL_" + case.kernel), rank_aware=case.rank_aware, **kw)
    for s in case.sides:
        getattr(eng, nf.KINDS[s].setter)(nf.arrays(case)["rec"][s])
    return eng


def run(torch, eng, case, d, needs, call, flush=False):
    """One solve of the arrays d on eng: "device" (outputs prefilled with the sentinel) or "host" (BatchMPC.solve) -> dict(u, x, y, status, iters)."""
    pc, wu, wy = nf.call_args(d, needs)
    if call == "device":
        return sentinel_solve(torch, eng, d, nf.SENTINEL, nf.ISENTINEL, f32=case.f32, pcom=pc, warm_u=wu, warm_y=wy, flush=flush)
    with np.errstate(over="ignore"):                                 # (1e39 rounded to float32)
        return eng.solve(d["x0"], d["x_ref"], d["foot"], d["contact"], pcom=pc, warm_u=wu, warm_y=wy, want_y=True, dtype=np.float32 if case.f32 else np.float64)


class Engines:
    """One handle per case and the clean solves on it, made on first use and shared by the tests of the module."""

    def __init__(self, torch):
        self.torch, self.eng, self.clean = torch, {}, {}

    def engine(self, case):
        if case.id not in self.eng:
            self.eng[case.id] = make_engine(case)
        return self.eng[case.id]

    def clean_run(self, case, needs, call, flush=False):
        key = (case.id, needs, call)
        if key not in self.clean:
            self.clean[key] = run(self.torch, self.engine(case), case, nf.arrays(case), needs, call, flush)
            st = self.clean[key]["status"]
            assert np.isin(st, (nf.SOLVED, nf.MAX_ITER)).all() and self.engine(case).kernel_name() == case.name, (case.id, st, self.engine(case).kernel_name())
        return self.clean[key]

    def close(self):
        for e in self.eng.values():
            e.close()


@pytest.fixture(scope="module")
def engines(torch_first, built_lib):
    e = Engines(torch_first)
    yield e
    e.close()


def contract(case, out, clean, bad, d, needs, tag, **kw):
    """nf.check_contract of one solve of a case, and the iters of its rejected QPs against the header table."""
    p = nf.params(case)
    seen = nf.check_contract(out, clean, bad, p, x0=d["x0"], zero_x=lambda b: nf.zero_rollout(case, nf.arrays(case), b, needs), f32=case.f32, tag=tag, **kw)
    print(f"{tag}: iters of the rejected QPs {seen}")
    for b, it in seen.items():
        assert it == expected_iters(bad[b], p), (tag, b, bad[b].name, it)
    return seen


# ---- every family, table-driven ---------------------------------------------------------------------------------------------------------------------
TABLE = [pytest.param(c.id, r.name, v, id=f"{c.id}-{r.name}-{v}") for c in nf.CASES for r, v in nf.rows_of(c)]
ALL_ROWS = {r.name: r for r in nf.ROWS + nf.LIVE_ROWS}


@pytest.mark.parametrize("cid,rname,vname", TABLE)
def test_poisoned_qp_is_rejected_and_nothing_else_changes(torch_first, engines, cid, rname, vname):
    case, row = nf.BY_ID[cid], ALL_ROWS[rname]
    picks = nf.picks_of(case, row, nf.F32_VALUES[vname])
    d = nf.poisoned(case, picks)
    bad = {b: row for b, _, _ in picks}
    eng = engines.engine(case)
    for call in ("device", "host"):
        clean = engines.clean_run(case, row.needs, call)
        out = run(torch_first, eng, case, d, row.needs, call)
        assert eng.kernel_name() == case.name, eng.kernel_name()
        seen = contract(case, out, clean, bad, d, row.needs, f"{cid}-{rname}-{vname}-{call}")
        assert len(seen) == (len(bad) if row.rejects else 0)
    if case.id.startswith("wrench_f32t"):                            # one QP on fp32 tiles and one on fp64 tiles were poisoned
        elig = {b: bool(np.isin((nf.arrays(case)["contact"][b] != 0).sum(1), (0, 3, 4)).all()) for b in bad}
        assert rname != "x0_pos" or set(elig.values()) == {True, False}, elig


@pytest.mark.parametrize("cid", ["live_h5_mixed", "live_h13_mixed"])
def test_live_horizon_writes_nothing_outside_a_rejected_qps_rows(torch_first, engines, cid):
    """The guard-row method of tests/test_gpu_any_horizon.py::test_no_write_outside_a_qps_rows: outputs one QP longer at each end, prefilled; the first and the
    last QP poisoned in their LAST real step (behind it lie the padding rows of the instantiation for N*)."""
    torch = torch_first
    case = nf.BY_ID[cid]
    B, n = case.B, case.N
    eng = engines.engine(case)
    for row in nf.LIVE_ROWS:
        picks = [(b, row, np.nan) for b in (0, B - 1) if nf.index_of(case, row, b) is not None]
        assert picks
        d = nf.poisoned(case, picks)
        t = [torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("x0", "x_ref", "foot", "contact")]
        u = torch.full((B + 2, n, 12), nf.SENTINEL, dtype=torch.float64, device="cuda")
        x = torch.full((B + 2, n + 1, 13), nf.SENTINEL, dtype=torch.float64, device="cuda")
        y = torch.full((B + 2, 20 * n), nf.SENTINEL, dtype=torch.float64, device="cuda")
        st = torch.full((B + 2,), nf.ISENTINEL, dtype=torch.int32, device="cuda")
        it = torch.full((B + 2,), nf.ISENTINEL, dtype=torch.int32, device="cuda")
        eng.solve_device(B, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), u[1:].data_ptr(), x_out=x[1:].data_ptr(), y_out=y[1:].data_ptr(),
                         status=st[1:].data_ptr(), iters=it[1:].data_ptr())
        eng.synchronize()
        assert eng.kernel_name() == case.name
        u, x, y, st, it = (v.cpu().numpy() for v in (u, x, y, st, it))
        for a in (u, x, y):
            assert np.all(a[0] == nf.SENTINEL) and np.all(a[-1] == nf.SENTINEL) and not np.any(a[1:-1] == nf.SENTINEL), row.name
        assert st[0] == st[-1] == it[0] == it[-1] == nf.ISENTINEL
        out = dict(u=u[1:-1], x=x[1:-1], y=y[1:-1], status=st[1:-1], iters=it[1:-1])
        contract(case, out, engines.clean_run(case, "plain", "device"), {b: row for b, _, _ in picks}, d, "plain", f"{cid}-guard-{row.name}")


# ---- the fp32 host call across the tile threshold ---------------------------------------------------------------------------------------------------
def test_f32_host_call_of_512_qps_rejects_in_both_tile_launches(torch_first, built_lib):
    """A host fp32 call of 512 QPs splits the batch by tile class into two launches over the same grid: one poisoned QP in each class, x0 NaN and 1e39 (inf once
    rounded); the neighbours of BOTH launches equal the clean call bit for bit."""
    case = nf.Case("f32_b512_n4_alt", 4, "alt_three", "wrench", "wrench_f32_n4", f32=True, B=512)
    ct = nf.arrays(case)["contact"]
    elig = lambda b: bool(np.isin((ct[b] != 0).sum(1), (0, 3, 4)).all())
    assert elig(200) and not elig(301)
    with make_engine(case) as eng:
        clean = run(torch_first, eng, case, nf.arrays(case), "plain", "host")
        assert eng.kernel_name() == case.name
        for rname, value in (("x0_pos", np.nan), ("x0_vel", 1e39), ("foot_stance_ge3", np.nan)):
            row = nf.ROW[rname]
            picks = [(b, row, value) for b in (200, 301) if nf.index_of(case, row, b) is not None]
            d = nf.poisoned(case, picks)
            out = run(torch_first, eng, case, d, "plain", "host")
            assert eng.kernel_name() == case.name
            seen = contract(case, out, clean, {b: row for b, _, _ in picks}, d, "plain", f"f32_b512-{rname}-{value}")
            assert len(seen) == len(picks) and (rname == "foot_stance_ge3" or len(seen) == 2)


# ---- the staged batch-1 call ----------------------------------------------------------------------------------------------------------------------------
STAGED = [(4, "single", "compact_f64_n4_s2_lat"), (8, "double", "wrench_f64_n8_lat")]
NO_LAT_NAME = {"compact_f64_n4_s2_lat": "compact_f64_n4_s2", "wrench_f64_n8_lat": "wrench_f64_n8"}     # SRBDQP_FLAG_NO_LAT: the batch instantiation of the same family


@pytest.mark.parametrize("launch", ["own_queue", "hip", "no_lat"])
@pytest.mark.parametrize("N,schedule,name", STAGED, ids=[s[2] for s in STAGED])
def test_staged_batch1_rejects_and_keeps_nothing(torch_first, built_lib, N, schedule, name, launch):
    """A clean QP, a poisoned one, the clean one again, through the same staging arrays (what MPC.update() does): the third solve equals the first bit for bit --
    nothing of the rejected QP survives in the handle.  With the library's own queue (where this box has one), through the HIP launch, and on the batch
    instantiations (SRBDQP_FLAG_NO_LAT)."""
    from g1_locomotion_amd import _lib
    case = nf.Case(f"staged_n{N}_{schedule}", N, schedule, "dense" if schedule == "single" else "wrench", name, B=2)
    d0 = nf.arrays(case)
    more = dict(flags=_lib.FLAG_NO_LAT) if launch == "no_lat" else {}
    os.environ.pop("SRBDQP_NO_AQL", None)
    if launch == "hip":
        os.environ["SRBDQP_NO_AQL"] = "1"                           # (read at the handle's first staged one-QP call: tests/test_gpu_aql.py)

    def one(eng, st, d):
        st["x0"][0] = d["x0"][0]; st["x_ref"][0] = d["x_ref"][0]; st["foot"][0] = d["foot"][0]; st["contact"][0] = d["contact"][0]
        for k in ("u", "x"):
            st[k][0] = nf.SENTINEL
        st["status"][0] = st["iters"][0] = nf.ISENTINEL
        eng.solve_staged(1, want_x=True)
        return dict(u=st["u"][:1].copy(), x=st["x"][:1].copy(), y=None, status=st["status"][:1].copy(), iters=st["iters"][:1].copy())

    try:
        with make_engine(case, **more) as eng:
            st = eng.stage()
            first = one(eng, st, d0)
            assert first["status"][0] == nf.SOLVED
            assert eng.kernel_name() == (NO_LAT_NAME[name] if launch == "no_lat" else name), eng.kernel_name()
            for rname in ("x0_pos", "foot_stance_le2" if schedule == "single" else "foot_stance_ge3", "xref_last"):
                row = nf.ROW[rname]
                d = nf.poisoned(case, [(0, row, np.nan)])
                out = one(eng, st, d)
                contract(case, out, first, {0: row}, d, "plain", f"staged-{name}-{launch}-{rname}")
                again = one(eng, st, d0)
                for k in ("u", "x", "status", "iters"):
                    assert nf.same_bits(again[k], first[k]), (rname, k)
            path = eng.batch1_launch_path()
            print(f"staged {name} {launch}: launch path {path}")
            if launch == "hip":
                assert path.startswith("hip: SRBDQP_NO_AQL"), path
            elif launch == "own_queue":   # the queue where this box has one; where it has none the library names ITS reason (tests/test_gpu_aql.py), never the variable's
                assert path == "aql" or (path.startswith("hip: ") and "SRBDQP_NO_AQL" not in path), path
            else:
                assert path == "undecided", path                     # (the batch instantiations do not go through the one-QP launch at all)
    finally:
        os.environ.pop("SRBDQP_NO_AQL", None)


X0_PREDICTED = nf.Row("x0_predicted", "x0", True, False, lambda N, ct: (4,))


def test_two_phase_call_rejects_a_poisoned_prediction_and_a_poisoned_measurement(torch_first, built_lib):
    """srbdqp_prepare_staged_f64 / srbdqp_solve_prepared_f64, N = 4 single support.  The header says the prediction is "anything finite" and, since this change,
    that a prediction that is not ends the QP with SRBDQP_NUMERICAL whatever the measured state is (the second phase patches the gradient with
    dq/dx0 (x0 - x0_predicted)); its roll-out starts from the measured x0, so x is the zero-force roll-out.  A poisoned measured x0 rejects like x0 everywhere."""
    case = nf.Case("two_phase_n4_single", 4, "single", "dense", "prepared_f64_n4", B=6)
    d0 = nf.arrays(case)
    B, N = case.B, case.N
    rng = np.random.default_rng(4)
    pred0 = d0["x0"] + rng.normal(size=d0["x0"].shape) * np.array([0.2] * 3 + [0.05] * 3 + [0.5] * 6 + [0.0])

    def two_phase(eng, st, pred, meas):
        st["x_ref"][:B] = d0["x_ref"]; st["foot"][:B] = d0["foot"]; st["contact"][:B] = d0["contact"]
        st["x0"][:B] = pred
        for k in ("u", "x"):
            st[k][:B] = nf.SENTINEL
        st["status"][:B] = st["iters"][:B] = nf.ISENTINEL
        eng.prepare_staged(B)
        assert eng.kernel_name().startswith("prepare_f64_n"), eng.kernel_name()
        eng.synchronize()                                            # (the first phase is asynchronous and reads the staging arrays: it has read the prediction now)
        st["x0"][:B] = meas
        eng.solve_prepared(B, want_x=True)
        assert eng.kernel_name().startswith(case.name), eng.kernel_name()
        return dict(u=st["u"][:B].copy(), x=st["x"][:B].copy(), y=None, status=st["status"][:B].copy(), iters=st["iters"][:B].copy())

    with make_engine(case) as eng:
        st = eng.stage()
        clean = two_phase(eng, st, pred0, d0["x0"])
        assert (clean["status"] == nf.SOLVED).all()
        bad_qps = (0, 3, B - 1)
        for value in (np.nan, np.inf):
            pred = pred0.copy()
            pred[list(bad_qps), 4] = value
            out = two_phase(eng, st, pred, d0["x0"])
            contract(case, out, clean, {b: X0_PREDICTED for b in bad_qps}, d0, "plain", f"two_phase-predicted-{value}")
            d = nf.poisoned(case, [(b, nf.ROW["x0_pos"], value) for b in bad_qps])
            out = two_phase(eng, st, pred0, d["x0"])
            contract(case, out, clean, {b: nf.ROW["x0_pos"] for b in bad_qps}, d, "plain", f"two_phase-measured-{value}")
        again = two_phase(eng, st, pred0, d0["x0"])
        assert all(nf.same_bits(again[k], clean[k]) for k in ("u", "x", "status", "iters"))


# ---- ragged fleets -----------------------------------------------------------------------------------------------------------------------------------
def _ragged_out(out, Nq, y=False):
    """A packed ragged result as per-QP lists (what nf.check_contract indexes)."""
    off = np.concatenate([[0], np.cumsum(Nq)])
    B = len(Nq)
    return dict(u=[out["u"][off[b]:off[b + 1]] for b in range(B)], x=[out["x"][off[b] + b:off[b + 1] + b + 1] for b in range(B)], y=None,
                status=out["status"], iters=out["iters"])


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_ragged_fleet_rejects_at_the_callers_index(torch_first, built_lib, f32):
    """RaggedMPC(horizons=(4, 8, 12)), 24 QPs in shuffled order, one poisoned QP per bucket: status -1 at the CALLER's index through the bucket permutation, in
    solve_packed and in the device entry (srbdqp_solve_ragged_device_f64 / _f32, outputs prefilled with the sentinel), in the given and in the reversed order
    (other bucket positions), every other QP bit-identical to the clean call.  The C-ABI has no kernel name for a ragged object: every bucket of the clean call is
    held bit for bit to a BatchMPC of its horizon on the general kernel, whose name is asserted (wrench_f64_n<N> / wrench_f32_n<N>)."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, RaggedMPC, _lib
    from gpu_helpers import sentinel_ragged_solve
    hz, B = (4, 8, 12), 24
    Nq, x0, xr, ft, ct = si.ragged_inputs(B, hz, 19)
    off = np.concatenate([[0], np.cumsum(Nq)])
    bad_of = {int(N): int(np.flatnonzero(Nq == N)[len(np.flatnonzero(Nq == N)) // 2]) for N in hz}      # one QP per bucket
    assert len(set(bad_of.values())) == 3
    fl = np.float32 if f32 else np.float64
    p = nf.params(nf.Case("ragged", 8, "mixed", "wrench", "", f32=f32))

    def zero_x(b):
        rnd = lambda v: np.asarray(v, fl).astype(np.float64)
        sl = slice(off[b], off[b + 1])
        return nf.orc.update(nf.orc.params_for(int(Nq[b])), rnd(x0[b]), rnd(xr[sl]), rnd(ft[sl]), np.zeros_like(ct[sl]))["x"]

    def reverse(a, per_qp):
        return a[::-1].copy() if per_qp else np.concatenate([a[off[b]:off[b + 1]] for b in range(B)][::-1])

    def both_orders(solve, x0b, ftb):
        """solve(Nq, x0, x_ref, foot, contact) -> packed result, in the given order and -- mapped back to it -- in the reversed one (QP b sits at B - 1 - b)."""
        with np.errstate(over="ignore"):
            fwd = _ragged_out(solve(Nq, x0b, xr, ftb, ct), Nq)
            rev = _ragged_out(solve(Nq[::-1].copy(), reverse(x0b, True), reverse(xr, False), reverse(ftb, False), reverse(ct, False)), Nq[::-1])
        back = dict(u=list(rev["u"])[::-1], x=list(rev["x"])[::-1], y=None, status=rev["status"][::-1].copy(), iters=rev["iters"][::-1].copy())
        return (("given", fwd), ("reversed", back))

    with RaggedMPC(horizons=hz, rho_restart_iter=-1) as rg:
        entries = dict(host=lambda *a: rg.solve_packed(*a, dtype=fl),
                       device=lambda *a: sentinel_ragged_solve(torch, rg, *a, nf.SENTINEL, nf.ISENTINEL, f32=f32))
        clean = _ragged_out(rg.solve_packed(Nq, x0, xr, ft, ct, dtype=fl), Nq)
        assert np.isin(clean["status"], (nf.SOLVED, nf.MAX_ITER)).all()
        for name, solve in entries.items():                          # the clean call is the same in both entries and both orders
            for order, got in both_orders(solve, x0, ft):
                for k in ("u", "x", "status", "iters"):
                    assert all(nf.same_bits(got[k][b], clean[k][b]) for b in range(B)), (name, order, k)
        for N in hz:                                                 # ... and is what the general kernel of each horizon computes
            idx = np.flatnonzero(Nq == N)
            with BatchMPC(horizon=int(N), kernel=_lib.KERNEL_WRENCH, rho_restart_iter=-1) as one:
                ref = one.solve(x0[idx], np.stack([xr[off[i]:off[i + 1]] for i in idx]), np.stack([ft[off[i]:off[i + 1]] for i in idx]),
                                np.stack([ct[off[i]:off[i + 1]] for i in idx]), dtype=fl)
                assert one.kernel_name() == f"wrench_{'f32' if f32 else 'f64'}_n{N}", one.kernel_name()
            for j, i in enumerate(idx):
                assert nf.same_bits(ref["u"][j], clean["u"][i]) and nf.same_bits(ref["x"][j], clean["x"][i]), (N, i)
                assert ref["status"][j] == clean["status"][i] and ref["iters"][j] == clean["iters"][i], (N, i)
        for rname, value in (("x0_pos", np.nan), ("x0_vel", -np.inf), ("foot_stance", np.nan)):
            x0b, ftb = x0.copy(), ft.copy()
            bad = {}
            for N, b in bad_of.items():
                c = ct[off[b]:off[b + 1]]
                if rname == "foot_stance":
                    k = int(np.flatnonzero(c.any(1))[0])
                    ftb[off[b] + k, 3 * int(np.flatnonzero(c[k])[0]) + 1] = value
                    bad[b] = nf.ROW["foot_stance_le2"]
                else:
                    x0b[b, nf.ROW[rname].index(N, c)[0]] = value
                    bad[b] = nf.ROW[rname]
            for name, solve in entries.items():
                for order, got in both_orders(solve, x0b, ftb):
                    seen = nf.check_contract(got, clean, bad, p, x0=x0b, zero_x=zero_x, f32=f32, tag=f"ragged-{rname}-{name}-{order}")
                    assert seen == {b: expected_iters(bad[b], p) for b in bad}, (name, order, seen)


# ---- the schedule hint -------------------------------------------------------------------------------------------------------------------------------
def test_schedule_hint_keeps_the_rejected_qp_at_its_index(torch_first, built_lib):
    """N = 8 single support, 64 QPs: a hint that dispatches the poisoned QPs first and one that dispatches them last.  Every key equals the unhinted call."""
    torch = torch_first
    case = nf.Case("hint_n8_single", 8, "single", "dense", "wave_f64_n8_s2", cfg=nf.S2, B=64)
    row = nf.ROW["x0_pos"]
    bad_qps = (0, 31, 63)
    d = nf.poisoned(case, [(b, row, np.nan) for b in bad_qps] + [(17, nf.ROW["foot_stance_le2"], np.inf)])
    bad = {b: row for b in bad_qps}
    bad[17] = nf.ROW["foot_stance_le2"]
    with make_engine(case) as eng:
        clean = run(torch, eng, case, nf.arrays(case), "plain", "device")
        plain = run(torch, eng, case, d, "plain", "device")
        assert eng.kernel_name() == case.name, eng.kernel_name()
        contract(case, plain, clean, bad, d, "plain", "hint-unhinted")
        for where, val in (("front", 250), ("back", 0)):
            h = np.full(case.B, 125, np.int32)
            h[list(bad)] = val
            hint = torch.from_numpy(h).cuda()
            eng.set_schedule_hint(hint.data_ptr(), case.B)
            hinted = run(torch, eng, case, d, "plain", "device")
            eng.set_schedule_hint(0, 0)
            for k in nf.KEYS:
                assert nf.same_bits(hinted[k], plain[k]), (where, k)


# ---- rho restart: in place, further launches, deferred tails ---------------------------------------------------------------------------------------
RESTART_TABLE = [pytest.param(c, r.name, id=f"{c.id}-{r.name}") for c in nf.RESTART_CASES for r in nf.restart_rows(c)]


@pytest.mark.parametrize("case,rname", RESTART_TABLE)
def test_restart_passes_never_run_a_rejected_qp_again(torch_first, built_lib, case, rname):
    """rho_restart_iter = 25, rho_restart_count = 2: every clean QP of the batch is past the first mark (tests/test_non_finite_cpu.py), so the neighbours of the
    poisoned QPs do restart -- in place (one-wave kernel), as further launches (general kernel), or deferred (SRBDQP_FLAG_DEFER_TAIL).  Before flush() a poisoned
    QP is never PENDING; after it its outputs are still -1, 0, 0 and the neighbours equal the clean run bit for bit.  warm_u / warm_y poison: the first pass
    starts from the caller's arrays, the later ones from its own.  The swing-foot row on the cases that have a swing contact (N = 8 single, N = 12 mixed)."""
    torch = torch_first
    row = nf.ROW[rname]
    picks = nf.picks_of(case, row, np.nan)
    d = nf.poisoned(case, picks)
    bad = {b: row for b, _, _ in picks}
    defer = "DEFER_TAIL" in case.flags
    pc, wu, wy = nf.call_args(d, row.needs)
    cpc, cwu, cwy = nf.call_args(nf.arrays(case), row.needs)
    with make_engine(case) as eng:
        clean = sentinel_solve(torch, eng, nf.arrays(case), nf.SENTINEL, nf.ISENTINEL, pcom=cpc, warm_u=cwu, warm_y=cwy, flush=defer)
        assert eng.kernel_name() == case.name, eng.kernel_name()
        assert (clean["iters"] > dict(case.cfg)["rho_restart_iter"]).all(), clean["iters"]
        o = sentinel_solve(torch, eng, d, nf.SENTINEL, nf.ISENTINEL, pcom=pc, warm_u=wu, warm_y=wy, sync=False)
        torch.cuda.synchronize()
        early = o["status"].cpu().numpy()
        if row.rejects:
            assert (early[list(bad)] == nf.NUMERICAL).all(), early                   # never PENDING, before the flush
        if defer:
            eng.flush(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in o.items() if k != "_in"}
        assert eng.kernel_name() == case.name, eng.kernel_name()
        contract(case, out, clean, bad, d, row.needs, f"{case.id}-{rname}")
        if not defer:
            host = run(torch, eng, case, d, row.needs, "host")
            contract(case, host, run(torch, eng, case, nf.arrays(case), row.needs, "host"), bad, d, row.needs, f"{case.id}-{rname}-host")


# ---- assembly dumps ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["wrench_f64_n8_mixed", "wrench_f64_n10_three"])
def test_wrench_dump_marks_every_rejected_qp(torch_first, built_lib, cid):
    """srbdqp_assemble_wrench_f64: goff[N] = -1 for every "rejects" row of x0, x_ref, foot and pcom, as the header says (nothing else of such a QP is written);
    every other QP's dump, and a QP poisoned on a swing foot only, equals the clean dump bit for bit."""
    case = nf.BY_ID[cid]
    N = case.N
    keys = ("T", "q", "Bd", "Vcol", "Vrow", "goff")
    with make_engine(case) as eng:
        clean = {False: eng.assemble_wrench(*(nf.arrays(case)[k] for k in ("x0", "x_ref", "foot", "contact")))}
        clean[True] = eng.assemble_wrench(*(nf.arrays(case)[k] for k in ("x0", "x_ref", "foot", "contact")), pcom=nf.arrays(case)["pcom"])
        assert eng.kernel_name() == case.name, eng.kernel_name()       # (the dump instantiation reports the name of the solve it stands for)
        assert (clean[False]["goff"][:, N] > 0).all()
        for row in nf.ROWS:
            if row.needs == "warm":
                continue
            for value in nf.VALUES.values():
                picks = nf.picks_of(case, row, value)
                d = nf.poisoned(case, picks)
                got = eng.assemble_wrench(d["x0"], d["x_ref"], d["foot"], d["contact"], pcom=d["pcom"] if row.needs == "pcom" else None)
                ref = clean[row.needs == "pcom"]
                bad = {b for b, _, _ in picks} if row.rejects else set()
                for b in range(case.B):
                    if b in bad:
                        assert got["goff"][b, N] == -1, (row.name, value, b, got["goff"][b])
                    else:
                        for k in keys:
                            assert nf.same_bits(got[k][b], ref[k][b]), (row.name, value, b, k)


@pytest.mark.parametrize("cid", ["wave_n8_single", "compact_n12_single"])
def test_dense_dump_keeps_a_poisoned_qp_to_itself(torch_first, built_lib, cid):
    """srbdqp_assemble_f64 (the header promises nothing for a poisoned QP but that the others are not affected): the neighbours' P, q, l, u are bit-identical to
    the clean dump, a swing-foot poison changes nothing at all, and the poisoned QP's own dump is written -- no sentinel left in it."""
    import ctypes as C
    case = nf.BY_ID[cid]
    B, n, m = case.B, 12 * case.N, 20 * case.N
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def dump(eng, d):
        o = dict(P=np.full((B, n, n), nf.SENTINEL), q=np.full((B, n), nf.SENTINEL), l=np.full((B, m), nf.SENTINEL), u=np.full((B, m), nf.SENTINEL))
        a = [np.ascontiguousarray(d[k]) for k in ("x0", "x_ref", "foot", "contact")]
        eng._check(eng._lib.srbdqp_assemble_f64(eng._h, B, *(ptr(v) for v in a), None, ptr(o["P"]), ptr(o["q"]), ptr(o["l"]), ptr(o["u"])))
        return o

    with make_engine(case) as eng:
        clean = dump(eng, nf.arrays(case))
        assert eng.kernel_name().startswith(case.name.split("_")[0] + "_"), eng.kernel_name()
        assert not any(np.any(v == nf.SENTINEL) for v in clean.values())
        for rname in ("x0_pos", "xref_yaw_mid", "foot_stance_le2", "foot_swing"):
            row = nf.ROW[rname]
            picks = nf.picks_of(case, row, np.nan)
            got = dump(eng, nf.poisoned(case, picks))
            bad = {b for b, _, _ in picks} if row.rejects else set()
            for b in range(B):
                for k in ("P", "q", "l", "u"):
                    if b in bad:
                        assert not np.any(got[k][b] == nf.SENTINEL), (rname, b, k)
                    else:
                        assert nf.same_bits(got[k][b], clean[k][b]), (rname, b, k)


# ---- the drop-in object ---------------------------------------------------------------------------------------------------------------------------------
def test_mpc_update_raises_on_nan_state_and_recovers(torch_first, built_lib):
    """MPC.update() with a NaN x_current raises (strict) and reports status -1, as tests/test_gpu_degenerate_contacts.py::test_mpc_update_raises_on_a_rejected_rung
    expects of status -1; the next, clean call equals a fresh object's answer bit for bit."""
    from g1_locomotion_amd import MPC, SrbdqpError
    case = nf.Case("mpc_n10_double", 10, "double", "wrench", "wrench_f64_n10_lat", B=2)
    d = nf.arrays(case)
    x0, xr, ft, ct = d["x0"][0], d["x_ref"][0], d["foot"][0], d["contact"][0]
    M, F = MPC(dt=0.04, horizon=10, rho_restart_iter=-1), MPC(dt=0.04, horizon=10, rho_restart_iter=-1)
    try:
        M.x_ref_hor = xr.copy(); F.x_ref_hor = xr.copy()
        bad = x0.copy()
        bad[4] = np.nan
        with pytest.raises(SrbdqpError):
            M.update(ct, ft, None, x_current=bad.reshape(13, 1))
        assert M.status == nf.NUMERICAL and M.iters == 5 and np.all(M.u_opt == 0.0), (M.status, M.iters)
        assert M._engine.kernel_name() == case.name, M._engine.kernel_name()
        u0, x1 = M.update(ct, ft, None, x_current=x0.reshape(13, 1))
        v0, y1 = F.update(ct, ft, None, x_current=x0.reshape(13, 1))
        assert M.status == F.status == nf.SOLVED and M.iters == F.iters
        assert nf.same_bits(u0, v0) and nf.same_bits(x1, y1) and nf.same_bits(M.u_opt, F.u_opt)
    finally:
        M.close(); F.close()
