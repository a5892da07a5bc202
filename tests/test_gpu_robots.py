"""GPU tests of what is particular to the per-QP robot records (include/srbdqp.h srbdqp_robot, srbdqp_set_robots / _device, srbdqp_ragged_set_robots / _device):
every QP of a batch with its own mass, inertia, friction coefficient and normal-force bounds, on the general kernel's MODE = 2 instantiation.  What the
records share with the other per-QP side inputs -- parity per QP, the neutral records, the schedule hint, the ragged order, bad device records -- is in
tests/test_gpu_side_inputs.py; the bars, the draw and the seeds are described in tests/side_inputs.py."""
import numpy as np
import pytest

from gpu_helpers import torch_first  # noqa: F401  (the fixture)
import side_inputs as si
from side_inputs import batch as _batch, draw_robots as _draw, ragged_inputs as _ragged_inputs
from test_gpu_side_inputs import NEUTRAL_CASES, check_neutral, check_parity

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("schedule", si.SCHEDULES)
@pytest.mark.parametrize("N", si.HORIZONS)
def test_per_qp_records_match_the_oracle(torch_first, built_lib, N, schedule):
    check_parity(si.ROBOTS, N, schedule)


@pytest.mark.parametrize("N,schedule", NEUTRAL_CASES)
def test_uniform_records_equal_the_config(torch_first, built_lib, N, schedule):
    """Every record = the handle's config: the same QPs as a KERNEL_WRENCH solve without records, bit for bit."""
    check_neutral(si.ROBOTS, N, schedule)


def _bound_active(u, ct, rec, tol=0.05):
    """A stance contact of some step on a friction-pyramid row (|f_x| or |f_y| = mu f_z) or on fz_max."""
    f = u.reshape(-1, 4, 3)
    st = ct.reshape(-1, 4) != 0
    fz = f[..., 2]
    fric = (np.maximum(np.abs(f[..., 0]), np.abs(f[..., 1])) >= rec[4] * fz - tol) & (fz > tol)
    top = fz >= rec[6] - tol
    return bool(np.any(st & (fric | top)))


def test_records_reach_the_kernel_through_the_bounds(torch_first, built_lib):
    """In at least a quarter of the QPs the solution moves by > 1 N from the nominal robot's AND a friction-pyramid or fz_max row of the QP's own record is
    active in it (N = 4 alone has few of those: its short horizon rarely pushes a force to a bound; 4 - 8 of 32 QPs in the oracle)."""
    from g1_locomotion_amd import BatchMPC
    B, moved, total = 32, 0, 0
    for N in (8, 10, 12, 16):
        for schedule in ("double", "mixed"):
            x0, xr, ft, ct = _batch(B, N, 900 + N, schedule)
            rec = _draw(B, 1900 + N)
            with BatchMPC(horizon=N) as eng:
                out0 = eng.solve(x0, xr, ft, ct)
                eng.set_robots(rec)
                out = eng.solve(x0, xr, ft, ct)
            for b in range(B):
                total += 1
                moved += int(np.abs(out["u"][b] - out0["u"][b]).max() > 1.0 and _bound_active(out["u"][b], ct[b], rec[b]))
    assert moved >= total // 4, (moved, total)


def test_refusals_and_clearing(torch_first, built_lib):
    from g1_locomotion_amd import BatchMPC, RaggedMPC, SrbdqpError, _lib
    from g1_locomotion_amd.mpc import robots_array
    B, N = 16, 10
    x0, xr, ft, ct = _batch(B, N, 51, "double")
    rec = _draw(B, 52)
    with BatchMPC(horizon=N) as fresh:
        ref = fresh.solve(x0, xr, ft, ct, want_y=True)
        ref_name = fresh.kernel_name()
    with BatchMPC(horizon=N) as eng:
        eng.set_robots(rec[:B - 1])
        with pytest.raises(SrbdqpError, match="robot records"):          # B > length
            eng.solve(x0, xr, ft, ct)
        bad = rec.copy()
        bad[5, 1] = -1.0
        with pytest.raises(SrbdqpError, match="record 5 is invalid"):
            eng.set_robots(bad)
        eng.solve(x0[:B - 1], xr[:B - 1], ft[:B - 1], ct[:B - 1])         # the previous setting was kept
        eng.set_robots(rec)
        with pytest.raises(SrbdqpError, match="refused"):
            eng.solve(x0, xr, ft, ct, dtype=np.float32)
        with pytest.raises(SrbdqpError, match="refused"):
            eng.assemble_wrench(x0, xr, ft, ct)
        with pytest.raises(SrbdqpError, match="refused"):
            eng.solve_staged(1)
        with pytest.raises(SrbdqpError, match="refused"):
            eng.prepare_staged(1)
        st = eng.stage()
        assert st is not None
        raw = _lib.load()
        u0 = np.zeros(12)
        assert raw.srbdqp_update_f64(eng._h, x0[0].ctypes.data, xr[0].ctypes.data, ft[0].ctypes.data, ct[0].astype(np.uint8).ctypes.data, None,
                                     u0.ctypes.data, None, None, None, None) == _lib.E_INVALID
        eng.set_robots(None)
        out = eng.solve(x0, xr, ft, ct, want_y=True)                      # after clearing: exactly as a fresh handle
        assert eng.kernel_name() == ref_name
        for k in ("u", "x", "y", "status", "iters"):
            assert np.array_equal(out[k], ref[k]), k
    with BatchMPC(horizon=N) as eng:
        with pytest.raises(SrbdqpError, match="refused"):
            eng.set_robots(rec)
            eng.assemble(x0, xr, ft, ct)
    for kern in (_lib.KERNEL_COMPACT, _lib.KERNEL_SPLIT, _lib.KERNEL_WAVE):
        with BatchMPC(horizon=N, kernel=kern) as eng:
            eng.set_robots(rec)
            with pytest.raises(SrbdqpError, match="general kernel only"):
                eng.solve(x0, xr, ft, ct)
    rg = RaggedMPC(horizons=(8, 12))
    try:
        Nq, rx0, rxr, rft, rct = _ragged_inputs(6, (8, 12), 53)
        rg.set_robots(robots_array(5))
        with pytest.raises(SrbdqpError, match="robot records"):
            rg.solve_packed(Nq, rx0, rxr, rft, rct)
        rg.set_robots(robots_array(6))
        with pytest.raises(SrbdqpError, match="refused"):
            rg.solve_packed(Nq, rx0, rxr, rft, rct, dtype=np.float32)
        bad = robots_array(6)
        bad[2, 7] = 1.0
        with pytest.raises(SrbdqpError, match="record 2 is invalid"):
            rg.set_robots(bad)
        rg.set_robots(None)
        rg.solve_packed(Nq, rx0, rxr, rft, rct, dtype=np.float32)
    finally:
        rg.close()


def test_wbid_reference_uses_each_robots_mass_and_inertia(torch_first, built_lib):
    import cascade_oracle as co
    from g1_locomotion_amd import BatchMPC
    B = 24
    rng = np.random.default_rng(61)
    x = rng.normal(size=(B, 13)); x[:, 12] = -9.81
    u = rng.uniform(-50, 300, size=(B, 12)); f = rng.normal(size=(B, 12))
    rec = _draw(B, 62)
    with BatchMPC(horizon=10) as eng:
        eng.set_robots(rec)
        got = eng.wbid_reference(x, u, f)
    for b in range(B):
        ref = co.wbid_reference(x[b], u[b], f[b].reshape(4, 3), rec[b, 0], tuple(rec[b, 1:4]))
        for k in ("R", "base_vel", "base_acc", "com_acc"):
            np.testing.assert_allclose(got[k][b].reshape(ref[k].shape), ref[k], rtol=1e-12, atol=1e-12, err_msg=f"{k} of robot {b}")


def test_n24_is_refused(torch_first, built_lib):
    """No instantiation of the general kernel reads records at N = 24 without scratch memory: the setters refuse an N = 24 handle and a ragged object
    with an N = 24 bucket, and nothing changes on either."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, RaggedMPC, SrbdqpError
    from g1_locomotion_amd.mpc import robots_array
    rec = robots_array(4)
    with BatchMPC(horizon=24) as eng:
        with pytest.raises(SrbdqpError, match="N = 24"):
            eng.set_robots(rec)
        with pytest.raises(SrbdqpError, match="N = 24"):
            eng.set_robots(torch.from_numpy(rec).cuda())
        eng.set_robots(None)
        x0, xr, ft, ct = _batch(4, 24, 3, "mixed")
        assert eng.solve(x0, xr, ft, ct)["status"].shape == (4,)
        assert eng.kernel_name() == "wrench_f64_n24"
    rg = RaggedMPC(horizons=(8, 24))
    try:
        with pytest.raises(SrbdqpError, match="N=24"):
            rg.set_robots(rec)
    finally:
        rg.close()
