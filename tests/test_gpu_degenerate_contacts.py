"""Nearly collinear stance contacts on the general kernel (srbdqp_wrench.hpp), on every path that runs it.

A step whose stance contact points lie on one line -- feet in tandem, point feet -- makes E = Y D^-1 Y' of that step singular while the QP stays well posed
(the dense kernels solve every rung, test_dense_kernels_answer_every_rung).  The kernel's conditioning guard compares every pivot of the step's 3 x 3 Schur
complement with the diagonal entry of E it came from and rejects the QP below kGuardRatioF64 = 2.5e-7 (fp64 iterations) or kGuardRatioF32 = 3e-5 (fp32
iterations).  The contract, for every QP on every path (tests/degenerate_twin.py::check_contract): ANSWERED -- SOLVED or MAX_ITER, forces within 5e-2 N
(fp64) / 1e-1 N (fp32) of the exact optimum, KKT residuals at the suite's bounds when SOLVED, swing entries exactly 0 -- or REJECTED -- SRBDQP_NUMERICAL,
u, y, iters exactly 0, x the finite roll-out of zero forces.  A must-answer QP (the twin WITHOUT the guard is SOLVED within a fifth of the bound, and the
pivot ratio is above the threshold) has to be answered, with the guarded twin's status.  Every second QP of a batch is an undeformed one; those come back
bit-identical to a solve of them alone on the same handle.

Pivot ratio against the outcome of the algorithm WITHOUT the guard (CPU twin, largest |u - exact| in newtons; tandem ratio = 0.34 eps^2, point feet 2.6 eps^2):

    ratio      fp64 twin                                 fp32 twin (fp64 tiles / fp32 tiles)
    >= 1e-4    <= 2e-3, SOLVED                           <= 7e-3, SOLVED or MAX_ITER
    3e-5       <= 1e-3                                   4e-3 / 2.6e-2          (N = 20: 9e-2 / 0.34: the one known rung above the threshold that is wrong)
    2.3e-5     <= 2e-3                                   3e-3 / 5e-2
    3e-6       <= 1e-3                                   5e-2, MAX_ITER / 0.27  <- largest wrong fp32 ratio on the committed ladders
    2.6e-6     <= 2e-3                                   2e-2 / 0.44
    3.4e-7     1e-3  (N = 20: 7e-3)                      0.25 / 4.3
    2.6e-8     2e-2  (N = 20: 0.12, SOLVED)              96 / NaN               <- largest wrong fp64 ratio (N = 20, every step)
    3.4e-9     2.6e-2 (N = 20: 0.22, SOLVED)             1.5e3 / NaN
    3.4e-11    4.2, SOLVED                               NaN
    <= 1e-12   8e2 ... 1e21, NaN, LinAlgError            NaN
Thresholds = largest wrong ratio x 10.  No committed rung lies within a factor 4 of its threshold: tandem 1e-3 and 1e-2 and point-feet 3e-3 did and were
moved to 3e-4, 2.2e-2 and 1.5e-3 (degenerate_twin.MOVED).  The guard sees one step's geometry; at equal ratio the error grows with the horizon and the number
of degenerate steps, so up to three rungs per batch that the unguarded twin answers well are rejected (test_degenerate_contacts_cpu.py pins them).
"""
import numpy as np
import pytest

import srbd_oracle as orc
import scenarios as sc
import degenerate_twin as dt
import side_inputs as si
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
KEYS = ("u", "x", "y", "status", "iters")


def _host(eng, x0, xr, ft, ct, dtype=np.float64):
    return eng.solve(x0, xr, ft, ct, want_y=True, dtype=dtype)


def run_batch(name, mode, engine, solve=_host, restart=False, kernel=None, prepare=None):
    """The interleaved batch of `name` through `engine()` and `solve`, then its healthy half alone on the same handle.
    Returns (records, healthy_identical): records = one (tag, u, x, y, status, iters, ref, contact, params, mode, x0) per deformed QP."""
    x0, xr, ft, ct = dt.interleaved(name)
    refs, p = dt.reference(name, mode, restart)
    with engine() as eng:
        if prepare:
            prepare(eng, x0.shape[0])
        out = solve(eng, x0, xr, ft, ct)
        kname = eng.kernel_name()
        if prepare:
            prepare(eng, x0.shape[0] // 2)
        alone = solve(eng, x0[1::2], xr[1::2], ft[1::2], ct[1::2])
    assert kernel is None or kname == kernel, kname
    same = all(np.array_equal(out[k][1::2], alone[k]) for k in KEYS)
    healthy_ok = bool(np.all(np.isin(alone["status"], (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER))) and np.all(np.isfinite(alone["u"])))
    x0k = x0 if mode == "f64" else np.asarray(x0, np.float32).astype(np.float64)
    recs = [((name, mode, b, r["eps"]), out["u"][2 * b], out["x"][2 * b], out["y"][2 * b], int(out["status"][2 * b]), int(out["iters"][2 * b]), r, ct[2 * b], p, mode, x0k[2 * b])
            for b, r in enumerate(refs)]
    return recs, same and healthy_ok


def assert_contract(recs, healthy_identical=True):
    kinds = [dt.check_contract(*r) for r in recs]
    assert healthy_identical, "the healthy QPs beside the ladder differ from a solve of them alone"
    assert "answered" in kinds and "rejected" in kinds, kinds          # the batch exercises both outcomes
    return kinds


def _wrench(N, **kw):
    from g1_locomotion_amd import BatchMPC, _lib
    kw.setdefault("kernel", _lib.KERNEL_WRENCH)
    kw.setdefault("rho_restart_iter", -1)
    return lambda: BatchMPC(horizon=N, **kw)


# ---- the paths (name -> records, healthy QPs identical): also what a build without the guard was measured with ----
def path_f64_n4(torch):
    return run_batch("n4_double", "f64", _wrench(4), kernel="wrench_f64_n4")


def path_f64_n10_mixed(torch):
    return run_batch("n10_mixed", "f64", _wrench(10), kernel="wrench_f64_n10")


def path_f64_n10_three(torch):
    return run_batch("n10_three", "f64", _wrench(10), kernel="wrench_f64_n10")


def path_restart(torch):
    return run_batch("n10_mixed", "f64", _wrench(10, rho_restart_iter=0), restart=True, kernel="wrench_f64_n10")


def _device_solve(torch, flush):
    def solve(eng, x0, xr, ft, ct):
        dev = torch.device("cuda", 0)
        B, N = x0.shape[0], xr.shape[1]
        d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (x0, xr, ft, ct)]
        u = torch.zeros((B, N, 12), dtype=torch.float64, device=dev); x = torch.zeros((B, N + 1, 13), dtype=torch.float64, device=dev)
        y = torch.zeros((B, 20 * N), dtype=torch.float64, device=dev)
        st = torch.full((B,), -77, dtype=torch.int32, device=dev); it = torch.full((B,), -77, dtype=torch.int32, device=dev)
        eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), x_out=x.data_ptr(), y_out=y.data_ptr(),
                         status=st.data_ptr(), iters=it.data_ptr())
        if flush:
            eng.flush()
        eng.synchronize()
        torch.cuda.synchronize(dev)
        return dict(u=u.cpu().numpy(), x=x.cpu().numpy(), y=y.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy())
    return solve


def path_defer_tail(torch):
    from g1_locomotion_amd import _lib
    return run_batch("n10_mixed", "f64", _wrench(10, rho_restart_iter=0, flags=_lib.FLAG_DEFER_TAIL), solve=_device_solve(torch, True), restart=True, kernel="wrench_f64_n10")


def path_f32_n10(torch):
    return run_batch("n10_double", "f32", _wrench(10), solve=lambda e, *a: _host(e, *a, dtype=np.float32), kernel="wrench_f32_n10")


def path_f32_tiles_n4(torch):
    from g1_locomotion_amd import _lib
    return run_batch("n4_double", "f32t", _wrench(4, flags=_lib.FLAG_F32_TILES), solve=lambda e, *a: _host(e, *a, dtype=np.float32), kernel="wrench_f32_n4")


def path_f32_tiles_n20(torch):
    from g1_locomotion_amd import _lib
    return run_batch("n20_double", "f32t", _wrench(20, flags=_lib.FLAG_F32_TILES), solve=lambda e, *a: _host(e, *a, dtype=np.float32), kernel="wrench_f32_n20")


def path_robots(torch):
    from g1_locomotion_amd.mpc import robots_array
    return run_batch("n10_mixed", "f64", _wrench(10), prepare=lambda eng, B: eng.set_robots(robots_array(B)), kernel="wrench_f64_n10_rb")


def path_live_horizon(torch):
    return run_batch("n7_mixed", "f64", _wrench(7), kernel="wrench_f64_n8_h7")


def path_cn_flat(torch):
    return run_batch("n10_three", "f64", _wrench(10), prepare=lambda eng, B: eng.set_contact_normals(si.flat_normals(B, 10)), kernel="wrench_f64_n10_cn")


LAT_RUNGS = (1e-1, 1e-2, 1e-3, 1e-5, 1e-8, 0.0)


def path_staged_lat(torch):
    """wrench_f64_n10_lat through srbdqp_solve_staged_f64, one QP per call: six rungs of the tandem ladder of n10_double."""
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct, meta = dt.inputs("n10_double")
    refs, p = dt.reference("n10_double", "f64")
    recs = []
    with BatchMPC(horizon=10, rho_restart_iter=-1) as eng:
        st = eng.stage()
        for b, (g, eps) in enumerate(meta):
            if g != 0 or eps not in LAT_RUNGS:
                continue
            st["x0"][0] = x0[b]; st["x_ref"][0] = xr[b]; st["foot"][0] = ft[b]; st["contact"][0] = ct[b]
            eng.solve_staged(1, want_x=True, want_y=True)
            assert eng.kernel_name() == "wrench_f64_n10_lat", eng.kernel_name()
            recs.append((("lat", b, eps), st["u"][0].copy(), st["x"][0].copy(), st["y"][0].copy(), int(st["status"][0]), int(st["iters"][0]), refs[b], ct[b], p, "f64", x0[b]))
    return recs, True


PATHS = dict(f64_n4=path_f64_n4, f64_n10_mixed=path_f64_n10_mixed, f64_n10_three=path_f64_n10_three, restart=path_restart, defer_tail=path_defer_tail,
             f32_n10=path_f32_n10, f32_tiles_n4=path_f32_tiles_n4, f32_tiles_n20=path_f32_tiles_n20, robots=path_robots, live_horizon=path_live_horizon,
             cn_flat=path_cn_flat, staged_lat=path_staged_lat)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_qp_is_answered_or_rejected(torch_first, built_lib, path):
    recs, healthy_identical = PATHS[path](torch_first)
    assert_contract(recs, healthy_identical)


def test_mpc_update_raises_on_a_rejected_rung(torch_first, built_lib):
    """MPC(strict=True).update() on the staged low-latency instantiation: SrbdqpError on a rejected rung, the right forces on an answered one."""
    from g1_locomotion_amd import MPC, SrbdqpError
    x0, xr, ft, ct, meta = dt.inputs("n10_double")
    refs, p = dt.reference("n10_double", "f64")
    M = MPC(dt=0.04, horizon=10, strict=True, rho_restart_iter=-1)
    seen = set()
    try:
        for b, (g, eps) in enumerate(meta):
            if g != 0 or eps not in LAT_RUNGS:
                continue
            M.x_ref_hor = xr[b].copy()
            r = refs[b]
            if r["guarded"]["status"] == orc.STATUS_NUMERICAL:
                with pytest.raises(SrbdqpError):
                    M.update(ct[b], ft[b], None, x_current=x0[b].reshape(13, 1))
                assert M.status == orc.STATUS_NUMERICAL
                seen.add("rejected")
            elif r["must_answer"]:
                u0, x1 = M.update(ct[b], ft[b], None, x_current=x0[b].reshape(13, 1))
                assert M._engine.kernel_name() == "wrench_f64_n10_lat", M._engine.kernel_name()
                assert M.status == r["guarded"]["status"] == orc.STATUS_SOLVED
                assert np.abs(np.asarray(u0).reshape(12) - r["us"][0]).max() <= dt.BOUND["f64"]
                assert np.abs(M.u_opt - r["us"]).max() <= dt.BOUND["f64"]
                seen.add("answered")
    finally:
        M.close()
    assert seen == {"answered", "rejected"}


def test_tilted_normals(torch_first, built_lib):
    """wrench_f64_n10_cn with every normal tilted by 10 degrees: the G block is full there and has its own pivots.  The exact optimum is that of the QP in the
    contacts' own frames (side_inputs.frames_matrix); a rung is must-answer here when its flat-ground ratio is 16 x above the threshold (the tilt turns the frames, not
    the contact points: the ratio moves by a factor near one)."""
    from g1_locomotion_amd import BatchMPC, _lib
    name, N = "n10_three", 10
    x0, xr, ft, ct = dt.interleaved(name)
    refs, p = dt.reference(name, "f64")
    B = x0.shape[0]
    a = np.deg2rad(10.0)
    nr = si.foot_normals(B, N, (np.sin(a), 0.0, np.cos(a)), (np.sin(a), 0.0, np.cos(a)))
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH, rho_restart_iter=-1) as eng:
        eng.set_contact_normals(nr)
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == "wrench_f64_n10_cn", eng.kernel_name()
        eng.set_contact_normals(nr[1::2])
        alone = eng.solve(x0[1::2], xr[1::2], ft[1::2], ct[1::2], want_y=True)
    assert all(np.array_equal(out[k][1::2], alone[k]) for k in KEYS)
    assert np.all(alone["status"] == orc.STATUS_SOLVED)
    T = si.frames_matrix(nr[0])
    kinds = set()
    for b, r in enumerate(refs):
        i = 2 * b
        qp = orc.build_qp(p, x0[i], xr[i], ft[i], ct[i])
        P = T.T @ qp["P"] @ T
        loc = dict(qp, P=0.5 * (P + P.T), q=T.T @ qp["q"])
        xs, _ = orc.solve_reference(p, loc)
        ref = dict(r, us=(p.force_scale * (T @ xs)).reshape(N, 12), qp=loc, must_answer=bool(r["free_ok"] and r["ratio"] > 16 * orc.GUARD_RATIO_F64))
        kinds.add(dt.check_contract(("cn 10 deg", b, r["eps"]), out["u"][i], out["x"][i], out["y"][i], int(out["status"][i]), int(out["iters"][i]), ref, ct[i], p, "f64", x0[i],
                                    must_status=False, frames=T, world_qp=qp))
    assert kinds == {"answered", "rejected"}


def test_ragged_buckets(torch_first, built_lib):
    """One ragged call over the buckets {8, 12}: the ladders of n8_mixed and n12_mixed interleaved with their healthy QPs, shuffled into one fleet."""
    from g1_locomotion_amd import RaggedMPC
    parts = []
    for name in ("n8_mixed", "n12_mixed"):
        x0, xr, ft, ct = dt.interleaved(name)
        refs, p = dt.reference(name, "f64")
        parts += [(name, b, x0[b], xr[b], ft[b], ct[b], refs[b // 2] if b % 2 == 0 else None, p) for b in range(x0.shape[0])]
    order = np.random.default_rng(5).permutation(len(parts))
    fleet = [parts[i] for i in order]

    def solve(eng, qps):
        Nq = [q[3].shape[0] for q in qps]
        return eng.solve_packed(Nq, np.stack([q[2] for q in qps]), np.concatenate([q[3] for q in qps]), np.concatenate([q[4] for q in qps]), np.concatenate([q[5] for q in qps]))
    eng = RaggedMPC(horizons=(8, 12), rho_restart_iter=-1)
    try:
        out = solve(eng, fleet)
        sound = [q for q in fleet if q[6] is None]
        alone = solve(eng, sound)
    finally:
        eng.close()
    kinds, j = set(), 0
    for i, q in enumerate(fleet):
        N = q[3].shape[0]
        u, x = out["u"][out["off"][i]:out["off"][i + 1]], out["x"][out["off"][i] + i:out["off"][i + 1] + i + 1]
        if q[6] is None:
            assert np.array_equal(u, alone["u"][alone["off"][j]:alone["off"][j + 1]]) and np.array_equal(x, alone["x"][alone["off"][j] + j:alone["off"][j + 1] + j + 1])
            assert out["status"][i] == alone["status"][j] == orc.STATUS_SOLVED and out["iters"][i] == alone["iters"][j]
            j += 1
        else:
            kinds.add(dt.check_contract(("ragged", q[0], q[1]), u, x, None, int(out["status"][i]), int(out["iters"][i]), q[6], q[5], q[7], "f64", q[2]))
    assert kinds == {"answered", "rejected"}


def test_assembly_marks_a_rejected_qp(torch_first, built_lib):
    """srbdqp_assemble_wrench_f64 on the n10_three batch: a QP the guard rejects has goff[N] = -1 (the kernel's ub_out[N] marker, include/srbdqp.h) and
    nothing else of it is defined; every other QP has goff[N] = n_g, and a must-answer one keeps the assembly bounds of tests/test_gpu_wrench.py (1e-11 on T,
    V, Bd, 1e-8 on the operator) against the oracle, scaled by the oracle's own distance from a longdouble reference where that is larger."""
    name, N = "n10_three", 10
    x0, xr, ft, ct = dt.interleaved(name)
    refs, p = dt.reference(name, "f64")
    with _wrench(N)() as eng:
        d = eng.assemble_wrench(x0, xr, ft, ct)
    marked = 0
    for i in range(x0.shape[0]):
        r = refs[i // 2] if i % 2 == 0 else None
        with np.errstate(all="ignore"):
            wr = orc.wrench_reduce(p, xr[i], ft[i], ct[i])
        if r is not None and not r["ratio"] > orc.GUARD_RATIO_F64:
            assert d["goff"][i][N] == -1, (i, r["eps"], d["goff"][i])
            marked += 1
            continue
        np.testing.assert_array_equal(d["goff"][i], wr["goff"])
        if r is not None and not r["must_answer"]:
            continue
        eV, eB, cond = sc.wrench_blocks_reference_error(p, xr[i], ft[i], ct[i])
        ng, vi, goff = wr["n_g"], wr["vi"], wr["goff"]
        T = d["T"][i]
        scale = max(1.0, 4 * max(eV, eB) / 1e-11)            # (E^-1 enters T as it enters V and Bd: where the float64 oracle is worse than 1e-11, its own error)
        assert np.abs(T[:ng, :ng] - wr["T"]).max() <= 1e-11 * scale * np.abs(wr["T"]).max(), (i, r and r["eps"], np.abs(T[:ng, :ng] - wr["T"]).max() / np.abs(wr["T"]).max(), scale)
        nu = len(vi)
        V = np.zeros((ng, nu)); Bd = np.zeros((nu, nu))
        for idx, v in enumerate(vi):
            k = v // 12
            same = [j for j, vv in enumerate(vi) if vv // 12 == k]
            Bd[idx, same] = d["Bd"][i][v][[vi[j] % 12 for j in same]]
            V[goff[k]:goff[k + 1], idx] = d["Vcol"][i][v][:goff[k + 1] - goff[k]]
        assert np.abs(V - wr["V"]).max() <= 1e-11 * scale * np.abs(wr["V"]).max(), (i, r and r["eps"], scale)
        assert np.abs(Bd - wr["Bd"]).max() <= 1e-11 * scale * max(np.abs(wr["Bd"]).max(), 1e-3), (i, r and r["eps"], scale)
        qp = orc.build_qp(p, x0[i], xr[i], ft[i], ct[i])
        red, _, _ = orc.presolve(qp, ct[i])
        Kinv, _ = sc.refined_inverse(sc.dense_k(p, red))
        Kw = Bd + V.T @ np.linalg.solve(T[:ng, :ng], V)
        assert np.abs(Kw - Kinv).max() <= 1e-8 * scale * np.abs(Kinv).max(), (i, r and r["eps"], np.abs(Kw - Kinv).max() / np.abs(Kinv).max(), scale)
    assert marked >= 6, marked


@pytest.mark.parametrize("kernel,schedule", [("compact", "double"), ("wave", "single"), ("split", "single")])
def test_dense_kernels_answer_every_rung(torch_first, built_lib, kernel, schedule):
    """The control: the dense kernels at N = 10 answer EVERY rung, eps = 0 included, at the normal bounds -- the weakness is the wrench coordinates alone.
    "single": heel and toe of the stance foot brought together (point feet on every step; two contacts are always collinear)."""
    from g1_locomotion_amd import BatchMPC, _lib
    N = 10
    mc = 4 if schedule == "double" else 2
    kid = dict(compact=_lib.KERNEL_COMPACT, wave=_lib.KERNEL_WAVE, split=_lib.KERNEL_SPLIT)[kernel]
    if schedule == "double":
        x0, xr, ft, ct, meta = dt.inputs("n10_double")
    else:
        b0 = orc.synthetic_batch(1, N, 11, "single")
        ft = np.stack([sc.collinear_contacts(b0[2][0], b0[3][0], e, "point", range(N)) for e in sc.EPS_LADDER])
        x0, xr, ct = (np.repeat(v, len(sc.EPS_LADDER), 0) for v in (b0[0], b0[1], b0[3]))
    p = orc.params_for(N)
    with BatchMPC(horizon=N, kernel=kid, max_contacts_per_step=mc, rho_restart_iter=-1) as eng:
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"{kernel}_f64_n{N}_s{mc}", eng.kernel_name()
    for b in range(x0.shape[0]):
        ref = orc.update(p, x0[b], xr[b], ft[b], ct[b])
        xs, _ = orc.solve_reference(p, ref["qp"])
        assert ref["status"] == orc.STATUS_SOLVED and out["status"][b] == orc.STATUS_SOLVED, (b, out["status"][b])
        assert abs(int(out["iters"][b]) - ref["iters"]) <= p.check_every
        assert np.abs(out["u"][b] - ref["u"]).max() <= 2e-3 and np.abs(out["u"][b].reshape(-1) - xs * p.force_scale).max() <= 5e-2, b
        red, vi, ri = orc.presolve(ref["qp"], ct[b])
        kr = orc.kkt_residuals(red["P"], red["q"], red["A"], red["l"], red["u"], out["u"][b].reshape(-1)[vi] / p.force_scale, out["y"][b][ri])
        assert kr["primal"] <= 1e-4 and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(ref["qp"]["q"]).max()), (b, kr)
        assert np.all(out["u"][b].reshape(-1)[np.setdiff1d(np.arange(12 * N), vi)] == 0.0)
