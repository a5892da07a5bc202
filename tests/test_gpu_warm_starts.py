"""A caller's warm start on every solve path, against the twin of that path (tests/warm_starts.py: the starts, the cases, the bars; tests/test_warm_starts_cpu.py
fixes the inputs on the twins alone).

  (a) test_one_interval_from_the_callers_start   max_iter = check_every = 5, no rho restart: engine and twin from the shifted start, u, x, y, status and iters at
      the equal-count bars (1e-4 N, 1e-5, 5e-7 |y|; fp32: 2e-2 N, 1e-3, 1e-4 |y|); the same start through with_junk is bit-identical to the clean run (the
      entries of swing contacts are not read); and -- (b) -- the device-buffer call from the same start is bit-identical to the host-buffer one.
  (b) test_staged_call_from_the_callers_start    use_warm on srbdqp_solve_staged_f64, B = 1 on both launch paths and B = 5: against the twin, against the batch
      solve from the same start (bit-identical on the live handle, 2e-4 N for the _lat kernels), and a use_warm=0 call right behind returns the cold result bit for bit.
  (c) test_full_solves_from_a_foreign_start, test_restart_passes_from_the_callers_start   default cap, shifted and neighbour start, the full bars; with the
      default rho restart the first pass starts from the caller's point and the later ones from their own.
  (d) test_own_solution_is_held_to_the_twin      every path of (a) restarted from its own (u, y): status and count as the twin's from that same start.
  (e) test_ragged_*                              srbdqp_solve_ragged_warm_device_f64 / _f32: bit-equal to the per-horizon solves from the same start, and at the
      twin's bars; the one-interval form; a live bucket; robot records beside the start, both in the caller's order.

What these tests see of P x^0 (it enters the stopping test only): the decision at the first checks, in (c) and (d).  (a) cannot see it and does not claim to.
(A P x^0 that is wrong shows there as a restart from the own solution that runs 25 - 30 iterations where the twin stops after 5, every iterate right.)
Every case prints its measured maxima (pytest -s)."""
import os
from dataclasses import replace

import numpy as np
import pytest

import side_inputs as si
import srbd_oracle as orc
import warm_starts as ws
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
KEYS = ("u", "x", "y", "status", "iters")
by_case = pytest.mark.parametrize("case", ws.CASES, ids=lambda c: c.id)


def _engine(case, full=False, restart=False, **more):
    """The handle of a case: one interval (max_iter 5, no restart, or the case's own cfg), or -- full -- the default cap without / with the default rho restart."""
    from g1_locomotion_amd import BatchMPC, _lib
    kw = dict(case.cfg)
    if full:
        kw.pop("max_iter", None); kw.pop("rho_restart_iter", None)
        if not restart:
            kw["rho_restart_iter"] = -1
    else:
        kw.setdefault("max_iter", 5); kw.setdefault("rho_restart_iter", -1)
    kw.update(more)
    flags = 0
    for f in case.flags:
        flags |= getattr(_lib, "FLAG_" + f)
    eng = BatchMPC(horizon=case.N, kernel=getattr(_lib, "KERNEL_" + case.kernel), rank_aware=case.rank_aware, flags=flags, **kw)
    rec = ws.inputs(case)["rec"]
    for s in case.sides:
        getattr(eng, ws.KINDS[s].setter)(rec[s])
    return eng


_restarts = ws.restarts


def _solve(torch, case, eng, WU, WY, call=None):
    """The case's batch from the start (WU, WY) (or from zero: None) through the host-buffer or the device-buffer call -> dict of host arrays."""
    d = ws.inputs(case)
    B, N = d["x0"].shape[0], case.N
    ft32 = np.float32 if case.f32 else np.float64
    if (call or case.call) == "host":
        return eng.solve(d["x0"], d["x_ref"], d["foot"], d["contact"], warm_u=WU, warm_y=WY, want_y=True, dtype=ft32)
    tt = torch.float32 if case.f32 else torch.float64
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, ft32)).cuda()
    t = [dev(d["x0"]), dev(d["x_ref"]), dev(d["foot"]), torch.from_numpy(np.ascontiguousarray(d["contact"], np.uint8)).cuda()]
    wu, wy = (None, None) if WU is None else (dev(WU), dev(WY))
    u = torch.zeros((B, N, 12), dtype=tt, device="cuda"); x = torch.zeros((B, N + 1, 13), dtype=tt, device="cuda"); y = torch.zeros((B, 20 * N), dtype=tt, device="cuda")
    st = torch.full((B,), -77, dtype=torch.int32, device="cuda"); it = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    eng.solve_device(B, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), u.data_ptr(), x_out=x.data_ptr(), y_out=y.data_ptr(),
                     status=st.data_ptr(), iters=it.data_ptr(), warm_u=0 if wu is None else wu.data_ptr(), warm_y=0 if wy is None else wy.data_ptr(), f32=case.f32)
    eng.flush()
    eng.synchronize()
    torch.cuda.synchronize()
    return dict(u=u.cpu().numpy(), x=x.cpu().numpy(), y=y.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy())


def _same(a, b):
    return [k for k in KEYS if not np.array_equal(a[k], b[k])]


# ---- (a), and the two doors of (b) ----------------------------------------------------------------------------------------------------------------
@by_case
def test_one_interval_from_the_callers_start(torch_first, built_lib, case):
    d = ws.inputs(case)
    B = d["x0"].shape[0]
    WU, WY = ws.starts(case)
    JU, JY = ws.with_junk(WU, WY, d["contact"])
    with _engine(case) as eng:
        cold = _solve(torch_first, case, eng, None, None)
        out = _solve(torch_first, case, eng, WU, WY)
        name = eng.kernel_name()
        junk = _solve(torch_first, case, eng, JU, JY)
        other = _solve(torch_first, case, eng, WU, WY, call="device" if case.call == "host" else "host")
        other_name = eng.kernel_name()
    assert name == case.name and other_name == case.name, (name, other_name)
    refs = ws.interval_twins(case, "shifted")
    ms = [ws.measure(out, b, refs[b]) for b in range(B)]
    ws.report(f"(a) {case.id} [{name}]", ms)
    moved = min(float(np.abs(np.asarray(out["u"][b], np.float64) - cold["u"][b]).max()) for b in range(B))
    print(f"(a) {case.id}: the start moves the engine's own forces by >= {moved:.2f} N; junk run differs in {_same(junk, out)}, other door in {_same(other, out)}")
    for b in range(B):
        m = ws.check(case, out, b, refs[b], ws.params(case, b))
        assert m[4] == 0 and int(out["iters"][b]) == case.iters, (b, out["iters"][b])
    assert moved > 1.0                                               # (as the twin: tests/test_warm_starts_cpu.py)
    assert _same(junk, out) == [], "a swing-contact entry of the start was read"
    assert _same(other, out) == [], "host-buffer and device-buffer call differ from the same start"


# ---- (b) the staged call ----------------------------------------------------------------------------------------------------------------------------
# (id, the kernel the staged call runs, the kernel choice of the batch solve it is compared with: the same family).  live_h7 runs the same kernel both ways and
# is bit-identical; a _lat instantiation has no batch form (another set-up schedule, the same iteration): both sides are within 1e-4 N of one twin at equal
# counts, so they are held to 2e-4 N of each other
STAGED_VS_BATCH_N = 2 * ws.TOL_EQUAL_N
STAGED = (("wave_n10_s2", "compact_f64_n10_s2_lat", "COMPACT"), ("wrench_f64_n10_mixed", "wrench_f64_n10_lat", "WRENCH"), ("live_h7", "wrench_f64_n8_h7", "AUTO"))
LIVE_H7 = ws.Case("live_h7", "wrench_f64", 7, "mixed", 9107, "wrench_f64_n8_h7")      # (an MPC-sized live handle: on the instantiation for N = 8)
by_staged = pytest.mark.parametrize("cid,name,family", STAGED, ids=[s[0] for s in STAGED])
_staged_cache = {}


def _staged_case(cid):
    """-> (the case, its batch, the five QPs staged, their shifted starts (B, 12 N) / (B, 20 N), their one-interval twins from those starts)"""
    if cid not in _staged_cache:
        base = LIVE_H7 if cid == "live_h7" else ws.BY_ID[cid]
        d = ws.inputs(base)
        N = base.N
        # (wrench_*_lat: the staged call takes the general kernel above 60 presolved variables)
        sel = [b for b in range(base.B) if cid != "wrench_f64_n10_mixed" or (np.asarray(d["contact"][b]) != 0).sum() * 3 > 60][:5]
        assert len(sel) == 5, sel
        if cid == "live_h7":
            WU, WY = np.zeros((base.B, 12 * N)), np.zeros((base.B, 20 * N))
            for b in sel:
                q = ws.qp_of(base, b)
                WU[b], WY[b] = ws.shifted_start(ws.params(base, b, full=True), q["x0"], q["x_ref"], q["foot"], q["contact"], orc.update)
        else:
            WU, WY = ws.starts(base)
        refs = [ws.twin(base.path, ws.params(base, b), ws.qp_of(base, b), (WU[b], WY[b])) for b in sel]
        _staged_cache[cid] = (base, d, sel, WU, WY, refs)
    return _staged_cache[cid]


def _staged(eng, cid, qs, use_warm, no_aql=False):
    """The QPs qs of the case through srbdqp_solve_staged_f64 (the staging warm_u / warm_y filled whether read or not) -> their outputs."""
    base, d, sel, WU, WY, refs = _staged_case(cid)
    N = base.N
    st = eng.stage()
    assert st["capacity"] >= len(qs)
    for i, b in enumerate(qs):
        st["x0"][i] = d["x0"][b]; st["x_ref"][i] = d["x_ref"][b]; st["foot"][i] = d["foot"][b].reshape(N, 12); st["contact"][i] = d["contact"][b].reshape(N, 4)
        st["warm_u"][i] = WU[b]; st["warm_y"][i] = WY[b]
    if no_aql:                                                       # (as tests/test_gpu_aql.py sets it: read at a handle's first staged one-QP call)
        os.environ["SRBDQP_NO_AQL"] = "1"
    try:
        eng.solve_staged(len(qs), use_warm=use_warm, want_x=True, want_y=True)
    finally:
        os.environ.pop("SRBDQP_NO_AQL", None)
    return {k: np.array(st[k][:len(qs)]) for k in KEYS}


def _check_staged(title, cid, out):
    base, d, sel, WU, WY, refs = _staged_case(cid)
    ms = [ws.check(base, out, i, refs[i], ws.params(base, sel[i])) for i in range(len(out["status"]))]
    ws.report(title, ms)
    assert all(m[4] == 0 for m in ms) and (out["iters"] == 5).all()


@by_staged
def test_staged_call_from_the_callers_start(torch_first, built_lib, cid, name, family):
    """use_warm on the staged call through the HIP launch, B = 1 and B = 5, one interval from the shifted start: at the bars of (a) against the twin; bit-identical
    to the batch solve from the same start on the live handle (the same kernel both ways), within 2e-4 N of the batch kernel of the same family for the _lat
    instantiations; a use_warm=0 call right behind one with use_warm=1 returns the cold result bit for bit."""
    from g1_locomotion_amd import BatchMPC, _lib
    base, d, sel, WU, WY, refs = _staged_case(cid)
    os.environ.pop("SRBDQP_NO_AQL", None)
    with BatchMPC(horizon=base.N, max_iter=5, rho_restart_iter=-1) as eng:
        cold1 = _staged(eng, cid, sel[:1], False, no_aql=True)
        one = _staged(eng, cid, sel[:1], True)
        assert eng.kernel_name() == name and eng.batch1_launch_path().startswith("hip: "), (eng.kernel_name(), eng.batch1_launch_path())
        again1 = _staged(eng, cid, sel[:1], False)                   # the staging arrays still hold the start
        cold5 = _staged(eng, cid, sel, False)
        five = _staged(eng, cid, sel, True)
        assert eng.kernel_name() == name, eng.kernel_name()
        again5 = _staged(eng, cid, sel, False)
    with BatchMPC(horizon=base.N, kernel=getattr(_lib, "KERNEL_" + family), max_iter=5, rho_restart_iter=-1, max_contacts_per_step=2 if family == "COMPACT" else 0) as eng:
        batch = eng.solve(d["x0"][sel], d["x_ref"][sel], d["foot"][sel], d["contact"][sel], warm_u=WU[sel], warm_y=WY[sel], want_y=True)
        batch_name = eng.kernel_name()
    assert _same(again1, cold1) == [] and _same(again5, cold5) == [], "a use_warm=0 call read the stale staging arrays"
    assert not np.array_equal(one["u"], cold1["u"]) and not np.array_equal(five["u"], cold5["u"])
    for k in KEYS:
        assert np.array_equal(five[k][0], one[k][0]), k              # QP 0 alone and QP 0 of five
    _check_staged(f"(b) {cid} [{name}] staged B = 1, HIP launch", cid, one)
    _check_staged(f"(b) {cid} [{name}] staged B = 5", cid, five)
    diff = [k for k in KEYS if not np.array_equal(five[k], batch[k])]
    print(f"(b) {cid}: against the batch solve [{batch_name}]: differs in {diff}, max |du| {np.abs(five['u'] - batch['u']).max():.3e} N")
    assert batch_name == (name[:-4] if name.endswith("_lat") else name), batch_name
    assert np.array_equal(five["status"], batch["status"]) and np.array_equal(five["iters"], batch["iters"])
    if cid == "live_h7":
        assert diff == [], diff
    else:
        assert np.abs(five["u"] - batch["u"]).max() <= STAGED_VS_BATCH_N and np.abs(five["x"] - batch["x"]).max() <= ws.TOL_X
        assert np.abs(five["y"] - batch["y"]).max() <= 2 * ws.DUAL64 * max(1.0, np.abs(batch["y"]).max())


@by_staged
def test_staged_one_qp_on_the_librarys_own_queue(torch_first, built_lib, cid, name, family):
    """The same one staged QP through the library's own queue -- the inline-inputs kernel of the batch-1 headline path, whose inputs ride in the kernel-argument
    segment and whose start does not --: bit-identical to the HIP launch of the same kernel, and at the bars of (a).  Skipped where the handle has no queue."""
    from g1_locomotion_amd import BatchMPC
    base, d, sel, WU, WY, refs = _staged_case(cid)
    os.environ.pop("SRBDQP_NO_AQL", None)
    with BatchMPC(horizon=base.N, max_iter=5, rho_restart_iter=-1) as eng, BatchMPC(horizon=base.N, max_iter=5, rho_restart_iter=-1) as hip:
        cold = _staged(eng, cid, sel[:1], False)
        path = eng.batch1_launch_path()
        if path != "aql":
            pytest.skip("no queue for this handle (%s)" % path)
        one = _staged(eng, cid, sel[:1], True)
        assert eng.kernel_name() == name and eng.batch1_launch_path() == "aql", (eng.kernel_name(), eng.batch1_launch_path())
        again = _staged(eng, cid, sel[:1], False)
        ref = _staged(hip, cid, sel[:1], True, no_aql=True)
        assert hip.kernel_name() == name and hip.batch1_launch_path().startswith("hip: "), (hip.kernel_name(), hip.batch1_launch_path())
    assert _same(again, cold) == [] and not np.array_equal(one["u"], cold["u"])
    assert _same(one, ref) == [], "the queue and the HIP launch differ from the same start"
    _check_staged(f"(b) {cid} [{name}] staged B = 1, the library's own queue", cid, one)


# ---- (c) full solves from a foreign start ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["shifted", "neighbour"])
@pytest.mark.parametrize("cid", ws.FULL_CASES)
def test_full_solves_from_a_foreign_start(torch_first, built_lib, cid, start):
    case = ws.BY_ID[cid]
    B = ws.inputs(case)["x0"].shape[0]
    rst = _restarts(case)
    W = [ws.full_start(case, start, b) for b in range(B)]
    WU, WY = np.stack([w[0] for w in W]), np.stack([w[1] for w in W])
    with _engine(case, full=True, restart=rst) as eng:
        out = _solve(torch_first, case, eng, WU, WY)
        assert eng.kernel_name() == case.name, eng.kernel_name()
    refs = ws.full_twins(case, start, rst)
    ms = [ws.measure(out, b, refs[b]) for b in range(B)]
    ws.report(f"(c) {cid} [{case.name}] from the {start} start", ms)
    print(f"(c) {cid}: iters {out['iters'].tolist()}, twin {[r['iters'] for r in refs]}")
    for b in range(B):
        ws.check(case, out, b, refs[b], ws.params(case, b, full=True, restart=rst), exact=True)


# (id, twin path, N, kernel, the batch seed -- chosen on the twin: QPs past the first restart mark from the neighbour's start)
RESTART = (("compact_n10_s4", "dense", 10, "AUTO", 9210), ("wrench_f64_n20", "wrench_f64", 20, "WRENCH", 9820))


@pytest.mark.parametrize("rid,path,N,kernel,seed", RESTART, ids=[r[0] for r in RESTART])
def test_restart_passes_from_the_callers_start(torch_first, built_lib, rid, path, N, kernel, seed):
    """The default rho restart, B = 48 mixed: the first pass starts from the caller's (u, y) -- the neighbour's solution --, the later ones from their own; against
    the twin run the same way on the QPs past the first mark and on four that are not (tests/test_gpu_parity.py::test_restart_in_place_from_a_warm_start)."""
    from g1_locomotion_amd import BatchMPC, _lib
    B = 48
    x0, xr, ft, ct = si.batch(B, N, seed, "mixed")
    mark = orc.default_restart(N)[0]
    p = orc.default_params(N)
    with BatchMPC(horizon=N, kernel=getattr(_lib, "KERNEL_" + kernel)) as eng:
        first = eng.solve(x0, xr, ft, ct, want_y=True)
        wu, wy = np.roll(first["u"].reshape(B, -1), -1, axis=0), np.roll(first["y"], -1, axis=0)
        out = eng.solve(x0, xr, ft, ct, warm_u=wu, warm_y=wy, want_y=True)
        name = eng.kernel_name()
    assert name == ("compact_f64_n10_s4" if N == 10 else "wrench_f64_n20"), name
    slow = np.where(out["iters"] > mark)[0]
    case = ws.Case(rid, path, N, "mixed", seed, name)
    past, ms = 0, []
    for b in list(slow[:6]) + list(np.where(out["iters"] <= mark)[0][:4]):
        ref = ws.twin(path, p, dict(x0=x0[b], x_ref=xr[b], foot=ft[b], contact=ct[b]), (wu[b], wy[b]))
        past += ref["iters"] > mark
        ms.append(ws.check(case, out, b, ref, p))
    ws.report(f"(c) {rid} [{name}] default restart, {len(slow)} of {B} QPs past iteration {mark}", ms)
    assert past >= 3, (past, out["iters"].tolist())


# ---- (d) the own solution ---------------------------------------------------------------------------------------------------------------------------
@by_case
def test_own_solution_is_held_to_the_twin(torch_first, built_lib, case):
    B = ws.inputs(case)["x0"].shape[0]
    rst = _restarts(case)
    with _engine(case, full=True, restart=rst) as eng:
        own = _solve(torch_first, case, eng, None, None)
        u0, y0 = np.asarray(own["u"], np.float64).reshape(B, -1), np.asarray(own["y"], np.float64)
        out = _solve(torch_first, case, eng, u0, y0)
        assert eng.kernel_name() == case.name, eng.kernel_name()
    refs = [ws.twin(case.path, ws.params(case, b, full=True, restart=rst), ws.qp_of(case, b), (u0[b], y0[b])) for b in range(B)]
    ms = [ws.measure(out, b, refs[b]) for b in range(B)]
    ws.report(f"(d) {case.id} [{case.name}] from its own solution", ms)
    print(f"(d) {case.id}: cold iters {own['iters'].tolist()}, again {out['iters'].tolist()}, twin {[r['iters'] for r in refs]}")
    for b in range(B):
        p = ws.params(case, b, full=True, restart=rst)
        assert int(out["status"][b]) == refs[b]["status"], (b, out["status"][b], refs[b]["status"])
        assert abs(ms[b][4]) <= p.check_every, (b, out["iters"][b], refs[b]["iters"])
        ws.check(case, out, b, refs[b], p)


# ---- (e) ragged fleets ------------------------------------------------------------------------------------------------------------------------------
RAGGED_HZ, RAGGED_B, RAGGED_SEED = (8, 12, 20), 30, 9130
_ragged = {}


def _fleet(hz=RAGGED_HZ, seed=RAGGED_SEED, robots=False):
    """The fleet, its shifted starts packed as (sum N, 12) / (sum N, 20), and the records where asked; computed once."""
    key = (hz, seed, robots)
    if key not in _ragged:
        Nq, x0, xr, ft, ct = si.ragged_inputs(RAGGED_B, hz, seed)
        off = np.concatenate([[0], np.cumsum(Nq)])
        rob = si.draw_robots(RAGGED_B, seed + 1) if robots else None
        WU, WY = np.empty((off[-1], 12)), np.empty((off[-1], 20))
        for b in range(RAGGED_B):
            r = slice(off[b], off[b + 1])
            p = si.params(int(Nq[b]), rob[b] if robots else None)
            p = replace(p, rho_restart_iter=0)
            wu, wy = ws.shifted_start(p, x0[b], xr[r], ft[r], ct[r], orc.update)
            WU[r], WY[r] = wu.reshape(-1, 12), wy.reshape(-1, 20)
        _ragged[key] = (Nq, x0, xr, ft, ct, off, WU, WY, rob)
    return _ragged[key]


def _ragged_twins(key, path, one_interval, restart=True):
    k = ("twins", key, path, one_interval, restart)
    if k not in _ragged:
        Nq, x0, xr, ft, ct, off, WU, WY, rob = _fleet(*key)
        out = []
        for b in range(RAGGED_B):
            N, r = int(Nq[b]), slice(off[b], off[b + 1])
            kw = dict(max_iter=5, rho_restart_iter=0) if one_interval else ({} if restart else dict(rho_restart_iter=0))
            p = si.params(N, rob[b] if rob is not None else None)
            if path != "wrench_f64" and path != "side":
                kw.update(eps_abs=2e-6, eps_rel=2e-6)
            p = replace(p, **kw)
            out.append((p, ws.twin(path, p, dict(x0=x0[b], x_ref=xr[r], foot=ft[r], contact=ct[r]), (WU[r].reshape(-1), WY[r].reshape(-1)))))
        _ragged[k] = out
    return _ragged[k]


def _ragged_solve(torch, rg, fleet, f32, flush=True):
    Nq, x0, xr, ft, ct, off, WU, WY, _ = fleet
    B, rows = len(Nq), int(off[-1])
    ft_, tt = (np.float32, torch.float32) if f32 else (np.float64, torch.float64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, ft_)).cuda()
    t = [dev(x0), dev(xr), dev(ft), torch.from_numpy(np.ascontiguousarray(ct, np.uint8)).cuda(), dev(WU), dev(WY)]
    u = torch.zeros((rows, 12), dtype=tt, device="cuda"); x = torch.zeros((rows + B, 13), dtype=tt, device="cuda"); y = torch.zeros((rows, 20), dtype=tt, device="cuda")
    st = torch.full((B,), -77, dtype=torch.int32, device="cuda"); it = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    rg.solve_device(B, Nq, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), u.data_ptr(), x.data_ptr(), st.data_ptr(), it.data_ptr(), stream=s,
                    f32=f32, warm_u=t[4].data_ptr(), warm_y=t[5].data_ptr(), y_out=y.data_ptr())
    if flush:
        rg.flush(s)
    torch.cuda.synchronize()
    return dict(u=u.cpu().numpy(), x=x.cpu().numpy(), y=y.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy())


def _per_qp(out, off, b):
    """QP b of a packed ragged result as a one-QP batch result."""
    return dict(u=out["u"][off[b]:off[b + 1]][None], x=out["x"][off[b] + b:off[b + 1] + b + 1][None], y=out["y"][off[b]:off[b + 1]].reshape(1, -1),
                status=out["status"][b:b + 1], iters=out["iters"][b:b + 1])


def _check_ragged(title, out, fleet, twins, f32):
    Nq, off = fleet[0], fleet[5]
    ms = []
    for b, (p, ref) in enumerate(twins):
        case = ws.Case(f"ragged qp {b} N={int(Nq[b])}", "wrench_f32" if f32 else "wrench_f64", int(Nq[b]), "", 0, "")
        ms.append(ws.check(case, _per_qp(out, off, b), 0, ref, p))
    ws.report(title, ms)
    return ms


@pytest.mark.parametrize("defer", [False, True], ids=["plain", "defer_tail"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_ragged_warm_entry_points(torch_first, built_lib, f32, defer):
    """srbdqp_solve_ragged_warm_device_f64 / _f32 with the default rho restart, with and without SRBDQP_FLAG_DEFER_TAIL (and the flush): every QP bit-equal to the
    per-horizon BatchMPC(kernel=KERNEL_WRENCH) solve from the same start (fp32: on fp64 tiles, as a ragged fp32 solve runs) and within the bars of its twin."""
    from g1_locomotion_amd import BatchMPC, RaggedMPC, _lib
    torch = torch_first
    fleet = _fleet()
    Nq, x0, xr, ft, ct, off, WU, WY, _ = fleet
    rg = RaggedMPC(horizons=RAGGED_HZ, flags=_lib.FLAG_DEFER_TAIL if defer else 0)
    try:
        out = _ragged_solve(torch, rg, fleet, f32)
    finally:
        rg.close()
    dt_ = np.float32 if f32 else np.float64
    for N in RAGGED_HZ:
        idx = np.where(Nq == N)[0]
        st = lambda a, w: np.stack([a[off[i]:off[i + 1]] for i in idx]).reshape(len(idx), *w)
        with BatchMPC(horizon=int(N), kernel=_lib.KERNEL_WRENCH, flags=_lib.FLAG_F64_TILES if f32 else 0) as one:
            ref = one.solve(x0[idx], st(xr, (N, 13)), st(ft, (N, 12)), st(ct, (N, 4)), warm_u=st(WU, (12 * N,)), warm_y=st(WY, (20 * N,)), want_y=True, dtype=dt_)
        for j, i in enumerate(idx):
            got = _per_qp(out, off, i)
            for k in KEYS:
                assert np.array_equal(np.asarray(got[k][0]).reshape(-1), np.asarray(ref[k][j]).reshape(-1)), (N, i, k)
    _check_ragged(f"(e) ragged {'f32' if f32 else 'f64'}{' defer_tail' if defer else ''}, horizons {RAGGED_HZ}", out, fleet,
                  _ragged_twins((RAGGED_HZ, RAGGED_SEED, False), "wrench_f32" if f32 else "wrench_f64", False), f32)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_ragged_one_interval_from_the_callers_start(torch_first, built_lib, f32):
    """The one-interval form of (a) on the fleet: every QP at the equal-count bars from its own rows of the packed start, and the junk on swing-contact entries
    changes nothing."""
    from g1_locomotion_amd import RaggedMPC
    fleet = _fleet()
    JU, JY = ws.with_junk(fleet[6], fleet[7], fleet[4])
    rg = RaggedMPC(horizons=RAGGED_HZ, max_iter=5, rho_restart_iter=-1)
    try:
        out = _ragged_solve(torch_first, rg, fleet, f32)
        junk = _ragged_solve(torch_first, rg, fleet[:6] + (JU, JY, None), f32)
    finally:
        rg.close()
    ms = _check_ragged(f"(e) ragged {'f32' if f32 else 'f64'} one interval", out, fleet,
                       _ragged_twins((RAGGED_HZ, RAGGED_SEED, False), "wrench_f32" if f32 else "wrench_f64", True), f32)
    assert all(m[4] == 0 for m in ms) and (out["iters"] == 5).all()
    assert _same(junk, out) == []


def test_ragged_live_bucket_and_robot_records(torch_first, built_lib):
    """A ragged object with live buckets (6, 9, 15) through the fp64 warm call, and set_robots on (8, 12, 16): record b and start b both follow the caller's order."""
    from g1_locomotion_amd import RaggedMPC
    for hz, robots in (((6, 9, 15), False), (si.RAGGED_HORIZONS, True)):
        key = (hz, RAGGED_SEED + 1, robots)
        fleet = _fleet(*key)
        rg = RaggedMPC(horizons=hz, max_iter=5, rho_restart_iter=-1)
        try:
            if robots:
                rg.set_robots(fleet[8])
            out = _ragged_solve(torch_first, rg, fleet, False)
        finally:
            rg.close()
        ms = _check_ragged(f"(e) ragged f64 one interval, horizons {hz}{' with robot records' if robots else ''}", out, fleet,
                           _ragged_twins(key, "side" if robots else "wrench_f64", True), False)
        assert all(m[4] == 0 for m in ms)
