"""GPU tests of what is particular to contact normals (include/srbdqp.h srbdqp_set_contact_normals / _device): friction pyramids on sloped ground, on the
general kernel's MODE = 4 instantiation (wrench_f64_n<N>_cn).  What the normals share with the other per-QP side inputs -- parity per QP on drawn normals, flat
normals, bad device values -- is in tests/test_gpu_side_inputs.py.

The reference is the twin of tests/side_inputs.py -- orc.build_qp's QP in the local force variables of every contact's frame, through the presolve and the
restarted ADMM orc.update runs -- with its per-QP bars (si.check_qp) applied to that local QP: the KKT bars on T' u / s and y_out."""
import numpy as np
import pytest

import side_inputs as si
import srbd_oracle as orc
from gpu_helpers import device_solve as _device_solve, to_dev as _to_dev, torch_first  # noqa: F401  (torch_first: the fixture)
from test_gpu_side_inputs import NEUTRAL_CASES, check_neutral, check_parity

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("schedule", si.SCHEDULES)
@pytest.mark.parametrize("N", si.HORIZONS)
def test_tilted_pyramids_match_the_twin(torch_first, built_lib, N, schedule):
    check_parity(si.NORMALS, N, schedule)


@pytest.mark.parametrize("N,schedule", NEUTRAL_CASES)
def test_flat_normals_change_nothing(torch_first, built_lib, N, schedule):
    """Every normal e_z against a KERNEL_WRENCH solve without normals: 1e-6 and one check interval (the general 3 x 3 inverse of G rounds differently from
    the flat kernel's reciprocals: ~1e-8 N expected)."""
    check_neutral(si.NORMALS, N, schedule)


def _parity(out, N, x0, xr, ft, ct, nr):
    """check_qp for every QP of the batch against its twin; returns the twins."""
    p = si.params(N)
    refs = [si.twin(p, x0[b], xr[b], ft[b], ct[b], normals=nr[b]) for b in range(len(x0))]
    for b, ref in enumerate(refs):
        si.check_qp(out, b, N, p, ref, ct[b])
    return p, refs


def test_the_normals_move_the_solutions(torch_first, built_lib):
    """Over the N >= 10 cases of the parity test at least a quarter of the QPs move by > 1 N from the flat-ground solve of the same inputs."""
    from g1_locomotion_amd import BatchMPC
    B, moved, total = 16, 0, 0
    for N in (10, 12, 16, 20):
        with BatchMPC(horizon=N) as eng:
            for schedule in si.SCHEDULES:
                x0, xr, ft, ct, nr = si.NORMALS.case(B, N, schedule)
                flat = eng.solve(x0, xr, ft, ct)
                out = eng.solve(x0, xr, ft, ct, normals=nr)
                assert eng.kernel_name() == f"wrench_f64_n{N}_cn"
                moved += int((np.abs(out["u"] - flat["u"]).reshape(B, -1).max(1) > 1.0).sum())
                total += B
    print(f"moved by > 1 N: {moved} of {total}")
    assert 4 * moved >= total, (moved, total)


@pytest.mark.parametrize("N", [10, 16])
def test_the_cone_reaches_the_kernel_on_a_ridge(torch_first, built_lib, N):
    """Double support either side of a 0.6 rad ridge (the twin: 16 / 16 solved, a friction row active in 16 / 16, the flat optimum outside the tilted pyramid by
    > 0.5 N in 16 (N = 10) and 15 (N = 16) of 16): parity, every solved QP's forces inside the tilted pyramid to 1e-4 (scaled), a friction row active in >= 12."""
    from g1_locomotion_amd import BatchMPC
    B = 16
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=5100 + N, schedule="double")
    nr = si.ridge_normals(B, N)
    with BatchMPC(horizon=N) as eng:
        out = eng.solve(x0, xr, ft, ct, want_y=True, normals=nr)
        assert eng.kernel_name() == f"wrench_f64_n{N}_cn"
    p, refs = _parity(out, N, x0, xr, ft, ct, nr)
    assert all(r["status"] == orc.STATUS_SOLVED for r in refs)
    active = 0
    for b, ref in enumerate(refs):
        viol = si.cone_violation(p, ref["qp"], ref["T"], out["u"][b])
        assert viol <= 1e-4, (b, viol)
        active += int(si.friction_row_active(p, ref["T"], out["u"][b], ct[b]))
    assert active >= 12, active


@pytest.mark.parametrize("schedule", ["double", "mixed"])
def test_wedge_parity(torch_first, built_lib, schedule):
    """Normals leaning inward by 0.3 rad (all 16 QPs solve in the twin)."""
    from g1_locomotion_amd import BatchMPC
    B, N = 16, 10
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=5100 + N, schedule=schedule)
    nr = si.wedge_normals(B, N)
    with BatchMPC(horizon=N) as eng:
        out = eng.solve(x0, xr, ft, ct, want_y=True, normals=nr)
    _, refs = _parity(out, N, x0, xr, ft, ct, nr)
    assert all(r["status"] == orc.STATUS_SOLVED for r in refs)


def test_block_b_belongs_to_qp_b_under_a_hint_and_a_deferred_tail(torch_first, built_lib):
    """Every QP with its own normals: the device-buffer solve under a schedule hint that reorders, and with SRBDQP_FLAG_DEFER_TAIL + flush, equals the plain one."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    B, N = 256, 10
    x0, xr, ft, ct = si.batch(B, N, 31, "mixed")
    nr = si.drawn_normals(B, N, np.random.default_rng(33), per_step=True)
    t = _to_dev(torch, x0, xr, ft, ct)
    dnr = torch.from_numpy(nr).cuda()
    with BatchMPC(horizon=N) as eng:
        eng.set_contact_normals(dnr)                                  # (the device setter: read in place)
        plain = _device_solve(torch, eng, t, B)
        torch.cuda.synchronize()
        assert eng.kernel_name() == f"wrench_f64_n{N}_cn"
        hint = torch.from_numpy(np.random.default_rng(5).integers(0, 250, B).astype(np.int32)).cuda()
        eng.set_schedule_hint(hint.data_ptr(), B)
        hinted = _device_solve(torch, eng, t, B)
        torch.cuda.synchronize()
        eng.set_schedule_hint(0, 0)
        host = eng.solve(x0, xr, ft, ct, normals=nr)                  # (the host setter, and back to the device array afterwards)
        again = _device_solve(torch, eng, t, B)
        torch.cuda.synchronize()
    assert int((plain["status"] == _lib.MAX_ITER).sum()) + int((plain["status"] == _lib.SOLVED).sum()) == B
    for k in ("u", "x", "status", "iters"):
        assert torch.equal(plain[k], hinted[k]), k
        assert torch.equal(plain[k], again[k]), k
        assert np.array_equal(plain[k].cpu().numpy(), host[k]), k
    with BatchMPC(horizon=N, flags=_lib.FLAG_DEFER_TAIL) as eng:
        eng.set_contact_normals(dnr)
        deferred = _device_solve(torch, eng, t, B)
        eng.flush(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert eng.kernel_name() == f"wrench_f64_n{N}_cn"
    for k in ("u", "x", "status", "iters"):
        assert torch.equal(plain[k], deferred[k]), k


def test_refusals(torch_first, built_lib):
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, SrbdqpError, _lib
    from g1_locomotion_amd.mpc import robots_array
    B, N = 16, 10
    x0, xr, ft, ct = si.batch(B, N, 51, "double")
    nr = si.wedge_normals(B, N)
    setter = "srbdqp_set_contact_normals"
    with BatchMPC(horizon=N) as eng:
        eng.set_contact_normals(nr[:B - 1])
        with pytest.raises(SrbdqpError, match=f"contact normals for {B - 1} set"):             # B > length: nothing launches
            eng.solve(x0, xr, ft, ct)
        eng.solve(x0[:B - 1], xr[:B - 1], ft[:B - 1], ct[:B - 1])
        eng.set_contact_normals(nr)
        with pytest.raises(SrbdqpError, match=f"srbdqp_solve_batch_f32: refused.*{setter}"):
            eng.solve(x0, xr, ft, ct, dtype=np.float32)
        with pytest.raises(SrbdqpError, match=f"srbdqp_assemble_wrench_f64: refused.*{setter}"):
            eng.assemble_wrench(x0, xr, ft, ct)
        with pytest.raises(SrbdqpError, match=f"srbdqp_assemble_f64: refused.*{setter}"):
            eng.assemble(x0, xr, ft, ct)
        with pytest.raises(SrbdqpError, match=f"srbdqp_solve_staged_f64: refused.*{setter}"):
            eng.solve_staged(1)
        with pytest.raises(SrbdqpError, match=f"srbdqp_prepare_staged_f64: refused.*{setter}"):
            eng.prepare_staged(1)
        with pytest.raises(SrbdqpError, match=f"srbdqp_solve_prepared_f64: refused.*{setter}"):
            eng.solve_prepared(1)
        raw = _lib.load()
        u0 = np.zeros(12)
        assert raw.srbdqp_update_f64(eng._h, x0[0].ctypes.data, xr[0].ctypes.data, ft[0].ctypes.data, ct[0].astype(np.uint8).ctypes.data, None,
                                     u0.ctypes.data, None, None, None, None) == _lib.E_INVALID
        assert f"srbdqp_update_f64: refused" in raw.srbdqp_last_error(eng._h).decode() and setter in raw.srbdqp_last_error(eng._h).decode()
        t = _to_dev(torch, x0, xr, ft, ct)
        o = torch.empty((B, N, 12), dtype=torch.float32, device="cuda")
        with pytest.raises(SrbdqpError, match=f"srbdqp_solve_batch_device_f32: refused.*{setter}"):
            eng.solve_device(B, t["x0"].data_ptr(), t["xr"].data_ptr(), t["ft"].data_ptr(), t["ct"].data_ptr(), o.data_ptr(), f32=True)
        with pytest.raises(SrbdqpError, match=f"srbdqp_set_robots: refused.*{setter}"):        # no instantiation reads records and normals
            eng.set_robots(robots_array(B))
        with pytest.raises(SrbdqpError, match=f"srbdqp_set_robots_device: refused.*{setter}"):
            eng.set_robots(torch.from_numpy(robots_array(B)).cuda())
        eng.set_contact_normals(None)
        eng.set_robots(robots_array(B))
        with pytest.raises(SrbdqpError, match="srbdqp_set_contact_normals: refused while per-QP robot records are set"):
            eng.set_contact_normals(nr)
        with pytest.raises(SrbdqpError, match="srbdqp_set_contact_normals_device: refused while per-QP robot records are set"):
            eng.set_contact_normals(torch.from_numpy(nr).cuda())
        eng.set_robots(None)
        eng.set_contact_normals(nr)
        eng.solve(x0, xr, ft, ct)
    for kern in (_lib.KERNEL_COMPACT, _lib.KERNEL_SPLIT, _lib.KERNEL_WAVE):
        with BatchMPC(horizon=N, kernel=kern) as eng:
            eng.set_contact_normals(nr)
            with pytest.raises(SrbdqpError, match="general kernel only"):
                eng.solve(x0, xr, ft, ct)
    with BatchMPC(horizon=24) as eng:
        n24 = si.flat_normals(2, 24)
        with pytest.raises(SrbdqpError, match="srbdqp_set_contact_normals: contact normals: not at N = 24"):
            eng.set_contact_normals(n24)
        with pytest.raises(SrbdqpError, match="srbdqp_set_contact_normals_device: contact normals: not at N = 24"):
            eng.set_contact_normals(torch.from_numpy(n24).cuda())
        eng.set_contact_normals(None)
    with BatchMPC(horizon=7) as eng:                                  # a live horizon (SRBDQP_FLAG_ANY_HORIZON)
        n7 = si.flat_normals(2, 7)
        with pytest.raises(SrbdqpError, match="srbdqp_set_contact_normals: refused on a handle whose horizon 7"):
            eng.set_contact_normals(n7)
        with pytest.raises(SrbdqpError, match="srbdqp_set_contact_normals_device: refused on a handle whose horizon 7"):
            eng.set_contact_normals(torch.from_numpy(n7).cuda())
    with BatchMPC(horizon=N) as eng:
        with pytest.raises(ValueError, match="expected shape"):
            eng.set_contact_normals(np.zeros((B, N + 1, 12)))


def test_mpc_update_with_contact_normals_equals_the_batch_solve(torch_first, built_lib):
    from g1_locomotion_amd import BatchMPC, MPC
    N = 10
    x0, xr, ft, ct = orc.synthetic_batch(1, N, seed=5100 + N, schedule="double")
    nr = si.ridge_normals(1, N)
    with BatchMPC(horizon=N) as eng:
        ref = eng.solve(x0, xr, ft, ct, normals=nr)
        flat = eng.solve(x0, xr, ft, ct)
    m = MPC(dt=0.04, horizon=N)
    m.init_matrices()
    try:
        m.x_ref_hor[:] = xr[0]
        u0, x1 = m.update(ct[0], ft[0], None, x_current=x0[0], contact_normals=nr[0])
        assert m.status == ref["status"][0] and m.iters == ref["iters"][0]
        assert np.array_equal(u0.reshape(-1), ref["u"][0][0]) and np.array_equal(x1, ref["x"][0]) and np.array_equal(m.u_opt, ref["u"][0])
        u0l, _ = m.update([ct[0][k] for k in range(N)], [ft[0][k] for k in range(N)], None, x_current=x0[0],
                          contact_normals=[nr[0][k] for k in range(N)])                         # per-step lists
        assert np.array_equal(u0l, u0)
        u0f, _ = m.update(ct[0], ft[0], None, x_current=x0[0])                                   # and without: the staged batch-1 path, flat ground
        assert np.abs(u0f.reshape(-1) - flat["u"][0][0]).max() <= si.TOL_EXACT_N and np.abs(u0f - u0).max() > 0.25
    finally:
        m.close()
