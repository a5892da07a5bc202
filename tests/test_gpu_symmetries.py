"""Every QP kernel held to the QP's exact symmetries on turning scenes (tests/symmetries.py): the world turned by 90 degrees, mirrored, heel and toe
relabelled, the feet's lanes swapped, the scene moved 1000 m from the origin.  Each maps a scene to OTHER input numbers whose solution is known exactly from
the base scene's, so a kernel is compared with ITSELF -- no twin arithmetic, and a convention the kernel shares with its twin cannot hide.

One solve call per case: the B base scenes followed by their images, block by block (batch order is pinned bitwise elsewhere, so one launch is enough); the
staged batch-1 paths make one call per scene.  Bars, stated once:
  every fp64 scene, base and image alike, against ITS OWN twin by the existing per-QP bars: status equal, iterations within one check interval, forces
    TOL_TWIN_N = 2e-3 N, roll-out 1e-5 (staged: 1e-4, as tests/test_gpu_turning.py), swing forces exactly 0 -- new input coverage by itself: 1000 m from
    the origin, a yaw beyond pi, every label order;
  every pair: status equal outright; where the two runs stop at the SAME iteration, forces [N] and states within pair_bar(N) = 100 D_N of each other, D_N
    the largest deviation the twin itself shows over the cases of that horizon and the five transformations, computed from the twin inside this run
    (8e-10 at N = 4, <= 8e-8 at N = 10, <= 5e-7 at N = 24; at N = 10 under a wrench 9e-7, on contact frames 5e-8: each side input has its own D); where they stop a check interval apart, TOL_TWIN_N only
    -- and at most one pair in eight of a case may be of that kind;
  fp32: rounding to float32 after the transformation breaks the pairing, so every image is held on its own to the fp32 bars of tests/test_gpu_wrench.py:
    status SOLVED, TOL32_TWIN_N = 2e-2 N against orc.update_split(float32), two check intervals, TOL32_EXACT_N = 1e-1 N against the exact optimum of the
    rounded QP, states 1e-3.  The fp32 shift is (1000, -700, 0) m.
tests/test_symmetries_cpu.py holds the twin to all of this first and decides which transformations a side input keeps (tilted normals: not rot90).
The measured ratios (kernel deviation / D_N, per path and transformation) are printed at the end of a run with -s; profiles/r34_symmetries.txt keeps them."""
import numpy as np
import pytest

import srbd_oracle as orc
import symmetries as sy
from gpu_helpers import torch_first  # noqa: F401  (the fixture)
from test_gpu_wrench import TOL32_EXACT_N, TOL32_TWIN_N, TOL_TWIN_N

pytestmark = pytest.mark.gpu

_rows = []      # (case label, transformation, pairs, pairs at unequal counts, worst deviation at equal counts, D_N, worst deviation at unequal counts)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nkernel deviation across a pair / D_N of the twin (pairs at equal iteration counts; bar 100)")
    print(f"  {'case':44s} {'transformation':9s} pairs unequal   worst [N]       D_N     ratio   worst at unequal counts [N]")
    for label, name, n, uneq, worst, d, worst_uneq in _rows:
        print(f"  {label:44s} {name:9s} {n:5d} {uneq:7d}   {worst:.3e}  {d:.2e}  {worst / d:8.2f}   {worst_uneq:.3e}")


def _case(path, N):
    """(engine keywords, what kernel_name() must say) of a path."""
    from g1_locomotion_amd import _lib
    off = dict(rho_restart_iter=-1)       # off unless the path is about it (as tests/test_gpu_wrench.py::_engine)
    return {"wave": (dict(off, kernel=_lib.KERNEL_WAVE), lambda s: s.startswith("wave_")),
            "wave_restart": (dict(sy.WAVE_RESTART, max_contacts_per_step=2), lambda s: s.startswith("wave_")),
            "compact": (dict(off, kernel=_lib.KERNEL_COMPACT), lambda s: s.startswith("compact_")),
            "compact_auto": (off, lambda s: s.startswith("compact_")),
            "wrench": (dict(off, kernel=_lib.KERNEL_WRENCH), lambda s: s == f"wrench_f64_n{N}"),
            "staged_compact": (off, lambda s: s == f"compact_f64_n{N}_s2_lat"),
            "staged_wrench": (off, lambda s: s == f"wrench_f64_n{N}_lat"),
            "any_horizon": ({}, lambda s: s == f"wrench_f64_n{min(n for n in _lib.HORIZONS if n >= N)}_h{N}"),
            "ew": ({}, lambda s: s == f"wrench_f64_n{N}_ew"), "staged_ew": ({}, lambda s: s == f"wrench_f64_n{N}_lat_ew"),
            "cn": ({}, lambda s: s == f"wrench_f64_n{N}_cn")}[path]


def _solve(path, N, x0, xr, ft, ct, pc, side):
    """The stacked batch through the path's kernel -> per-QP dicts(u, x, status, iters)."""
    from g1_locomotion_amd import BatchMPC
    kw, named = _case(path, N)
    n = len(x0)
    with BatchMPC(horizon=N, **kw) as eng:
        if path.startswith("staged"):
            st, res = eng.stage(), []
            for b in range(n):                                       # every scene and every image is a call of its own
                st["x0"][0], st["x_ref"][0], st["foot"][0], st["contact"][0], st["pcom"][0] = x0[b], xr[b], ft[b], ct[b], pc[b]
                if path == "staged_ew":
                    eng.stage_ext_wrench()[0] = side[b]
                    eng.solve_staged_wrench(1, use_pcom=True, want_x=True)
                else:
                    eng.solve_staged(1, use_pcom=True, want_x=True)
                assert named(eng.kernel_name()), eng.kernel_name()
                res.append(dict(u=st["u"][0].copy(), x=st["x"][0].copy(), status=int(st["status"][0]), iters=int(st["iters"][0])))
            return res
        if path == "ew":
            eng.set_external_wrench(side)
        if path == "cn":
            eng.set_contact_normals(side)
        out = eng.solve(x0, xr, ft, ct, pcom=pc)
        assert named(eng.kernel_name()), eng.kernel_name()
    return [dict(u=out["u"][b], x=out["x"][b], status=int(out["status"][b]), iters=int(out["iters"][b])) for b in range(n)]


def _hold_to_twin(label, b, r, ref, contact, check_every, x_tol=1e-5):
    """One fp64 scene against its own twin: the per-QP bars of the existing suites."""
    assert r["status"] == ref["status"] and ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER), (label, b, r["status"], ref["status"])
    assert abs(r["iters"] - ref["iters"]) <= check_every, (label, b, r["iters"], ref["iters"])
    du, dx = np.abs(r["u"] - ref["u"]).max(), np.abs(r["x"] - ref["x"]).max()
    assert du <= TOL_TWIN_N, (label, b, du)
    assert dx <= x_tol, (label, b, dx)
    assert np.all(r["u"].reshape(-1, 4, 3)[np.asarray(contact).reshape(-1, 4) == 0] == 0.0), (label, b)      # swing contacts carry exactly zero force


def _hold_pairs(label, res, backs, nb, bar_of, d_of):
    """Every base QP of `res` (nb of them, then their images block by block) against each of its images, by the pair bars of the docstring.  Every pair
    is measured before anything is asserted, so a run that fails still reports every figure."""
    findings, unequal, pairs = [], 0, 0
    for j, (name, back) in enumerate(backs):
        worst, uneq, worst_uneq = (0.0, 0.0, d_of(0)), 0, 0.0             # (ratio, deviation, D) of the worst pair at equal counts
        for b in range(nb):
            du, dx, same_status, same_iters = sy.pair_deviation(res, b, j, nb, back)
            i = (j + 1) * nb + b
            print(f"{label} {name} qp {b}: iters {res[b]['iters']}/{res[i]['iters']} |du| {du:.2e} N |dx| {dx:.2e}  bar {bar_of(b):.2e}")
            if not same_status:
                findings.append(f"{name} qp {b}: status {res[b]['status']} / {res[i]['status']}")
            elif same_iters:
                worst = max(worst, (max(du, dx) / d_of(b), max(du, dx), d_of(b)))
                if not max(du, dx) <= bar_of(b):                           # a finding (a NaN too): which transformation, which force components
                    comp = np.abs(back(res[i]["u"], res[i]["x"])[0] - res[b]["u"]).reshape(-1, 4, 3).max(axis=0)
                    findings.append(f"{name} qp {b}: |du| {du:.3e} N |dx| {dx:.3e} > pair bar {bar_of(b):.3e} at equal counts ({res[b]['iters']}); "
                                    f"worst per contact (rows) and axis (columns) [N]: {np.array2string(comp, precision=2)}")
            else:
                uneq += 1
                worst_uneq = max(worst_uneq, du)
                if not du <= TOL_TWIN_N:
                    findings.append(f"{name} qp {b}: |du| {du:.3e} N > {TOL_TWIN_N} at iteration counts {res[b]['iters']} / {res[i]['iters']}")
        _rows.append((label, name, nb, uneq, worst[1], worst[2], worst_uneq))
        unequal += uneq
        pairs += nb
    assert not findings, label + ":\n  " + "\n  ".join(findings)
    assert unequal <= sy.MAX_UNEQUAL_SHARE * pairs, (label, unequal, pairs)       # above one pair in eight the test fails instead of thinning itself out


@pytest.mark.parametrize("path,N,schedule,yaw,B", sy.CASES)
def test_kernel_holds_the_symmetries(torch_first, built_lib, path, N, schedule, yaw, B):
    x0, xr, ft, ct, pc, side, backs = sy.stacked(path, N, schedule, yaw, B)
    assert len(x0) == (1 + len(backs)) * B
    res = _solve(path, N, x0, xr, ft, ct, pc, side)
    refs = sy.twins(path, N, schedule, yaw, B)
    p = sy.twin_params(path, N)
    label = f"{path} N={N} {schedule} {yaw}"
    for b in range(len(x0)):
        _hold_to_twin(label, b, res[b], refs[b], ct[b], p.check_every, x_tol=1e-4 if path.startswith("staged") else 1e-5)
    if path == "wave_restart":
        assert sy.restarted(res, B) >= sy.RESTARTED_MIN, [r["iters"] for r in res]       # the case must exercise the second pass, on the kernel itself
    side_kind = sy.SIDE_OF.get(path)
    _hold_pairs(label, res, backs, B, lambda b: sy.pair_bar(N, side_kind), lambda b: sy.twin_d(N, side_kind))


def test_ragged_fleet_holds_the_symmetries(torch_first, built_lib):
    """One ragged fleet, horizons (8, 12, 16, 24), two QPs per horizon; the images are further QPs of the same call."""
    from g1_locomotion_amd import RaggedMPC
    problems, Nq, backs, refs, nb = sy.ragged_fleet()
    eng = RaggedMPC(horizons=sy.RAGGED_HORIZONS, rho_restart_iter=-1)
    try:
        res = eng.solve(problems)
    finally:
        eng.close()
    for b, (pr, r) in enumerate(zip(problems, res)):
        assert r["u"].shape == pr["foot"].shape and r["x"].shape == (Nq[b] + 1, 13)
        _hold_to_twin("ragged", b, r, refs[b], pr["contact"], orc.params_for(Nq[b]).check_every)
    _hold_pairs("ragged (8, 12, 16, 24)", res, backs, nb, lambda b: sy.pair_bar(Nq[b]), lambda b: sy.twin_d(Nq[b]))


@pytest.mark.parametrize("path,N,schedule,yaw,B", sy.F32_CASES)
def test_fp32_path_holds_every_image_on_its_own(torch_first, built_lib, path, N, schedule, yaw, B):
    """The fp32 iterations 1000 m from the origin, at a yaw beyond pi and in every label order: each scene by the fp32 bars of tests/test_gpu_wrench.py."""
    from g1_locomotion_amd import BatchMPC, _lib
    x0, xr, ft, ct, pc, _, backs = sy.stacked(path, N, schedule, yaw, B, f32=True)
    flags = _lib.FLAG_F32_TILES if path == "f32_tiles" else _lib.FLAG_F64_TILES if schedule == "mixed" else 0
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH, rho_restart_iter=-1, flags=flags) as eng:
        out = eng.solve(x0, xr, ft, ct, pcom=pc, dtype=np.float32)           # (the wrapper rounds to float32: after the transformation)
        assert eng.kernel_name() == f"wrench_f32_n{N}", eng.kernel_name()
    assert out["u"].dtype == np.float32 and out["x"].dtype == np.float32
    if path == "f32_tiles":
        assert all(orc.fp32_tiles_ok(c) for c in ct)                         # the case exercises what its name says
    refs, p = sy.twins32(path, N, schedule, yaw, B)
    names = ["base"] + [n for n, _ in backs]
    worst, failed = {}, []
    for b, ref in enumerate(refs):
        name = names[b // B]
        du, dx = np.abs(out["u"][b] - ref["u"]).max(), np.abs(out["x"][b] - ref["x"]).max()
        de = np.abs(out["u"][b].reshape(-1).astype(np.float64) - ref["xs"] * p.force_scale).max()
        print(f"{path} N={N} {name} qp {b % B}: status {out['status'][b]}/{ref['status']} iters {out['iters'][b]}/{ref['iters']} twin {du:.2e} N x {dx:.2e} exact {de:.2e} N")
        w = worst.setdefault(name, [0.0, 0.0, 0.0])
        w[:] = max(w[0], du), max(w[1], dx), max(w[2], de)
        ok = dict(status=out["status"][b] == ref["status"] == orc.STATUS_SOLVED, iters=abs(int(out["iters"][b]) - ref["iters"]) <= 2 * p.check_every,
                  twin=du <= TOL32_TWIN_N, x=dx <= 1e-3, exact=de <= TOL32_EXACT_N, swing=np.all(out["u"][b].reshape(-1, 4, 3)[ct[b] == 0] == 0.0))
        if not all(ok.values()):
            failed.append((name, b % B, [k for k, v in ok.items() if not v], int(out["status"][b]), int(out["iters"][b]), ref["iters"], float(du), float(dx), float(de)))
    for name, (du, dx, de) in worst.items():
        print(f"fp32 {path} N={N} {schedule} {name:9s} worst: twin {du:.2e} / {TOL32_TWIN_N:.0e} N, x {dx:.2e} / 1e-3, exact {de:.2e} / {TOL32_EXACT_N:.0e} N")
    assert not failed, failed          # (scene, QP, the bars missed, status, iterations kernel / twin, |u - twin| [N], |x - twin|, |u - exact| [N])
