"""Rank-aware wrench steps (SRBDQP_FLAG_RANK_AWARE; srbdqp_wrench.hpp, MODE = 5) on the general kernel: the ladders of nearly collinear stance contacts that an
unflagged handle rejects below the conditioning guard (tests/test_gpu_degenerate_contacts.py) are ANSWERED here, every rung of them -- feet in tandem and point
feet down to exactly collinear contact points.

A batch = the rungs of a ladder pair interleaved with as many healthy QPs (degenerate_twin.interleaved: 40 QPs, 16 for the 4-rung ladders of N = 20).  Every
deformed QP has to come back under degenerate_twin.check_contract as a must-answer QP: forces within 5e-2 N of the exact optimum, KKT residuals at the suite's
bounds when SOLVED, swing entries exactly 0, the status of the rank-aware twin (tests/rank_aware_twin.py); no QP is rejected.  (The KKT bound is what makes
the kernel normalise more steps than the guard refuses: on E^-1, the 20 double-support steps of n20_double's 1 mm point feet -- ratio 2.5e-6, ten times
above the guard -- left a stationarity residual of 227 against the bound 49; rank_aware_twin.SELECT_RATIO.)  The healthy half is bit-identical
to a solve of it alone on the same handle and within the suite's bounds of its own exact optimum.  On the parent of this change the flag's bit is ignored and 11
rungs per batch of 40 come back SRBDQP_NUMERICAL.
"""
import functools

import numpy as np
import pytest

import srbd_oracle as orc
import degenerate_twin as dt
import rank_aware_twin as rt
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
KEYS = ("u", "x", "y", "status", "iters")


@functools.lru_cache(maxsize=None)
def references(name, restart=False):
    """Per deformed QP: degenerate_twin.reference's record as a must-answer one, `guarded` = the rank-aware twin's result; and the parameters."""
    refs, p = dt.reference(name, "f64", restart)
    x0, xr, ft, ct, meta = dt.inputs(name)
    out = []
    for b, r in enumerate(refs):
        tw = rt.update_rank_aware(p, x0[b], xr[b], ft[b], ct[b])
        assert tw["status"] == orc.STATUS_SOLVED and np.abs(tw["u"] - r["us"]).max() <= dt.BOUND["f64"] / 5, (name, b, r["eps"])
        out.append(dict(r, must_answer=True, guarded=tw))
    return out, p


def _engine(N, **kw):
    from g1_locomotion_amd import BatchMPC, _lib
    kw.setdefault("kernel", _lib.KERNEL_WRENCH)
    kw.setdefault("rho_restart_iter", -1)
    return BatchMPC(horizon=N, rank_aware=True, **kw)


def _host(eng, x0, xr, ft, ct):
    return eng.solve(x0, xr, ft, ct, want_y=True)


def _run(name, eng, solve=_host, restart=False):
    N = dt.BATCHES[name]["N"]
    x0, xr, ft, ct = dt.interleaved(name)
    refs, p = references(name, restart)
    with eng:
        out = solve(eng, x0, xr, ft, ct)
        kname = eng.kernel_name()
        alone = solve(eng, x0[1::2], xr[1::2], ft[1::2], ct[1::2])
    assert kname == f"wrench_f64_n{N}_ra", kname
    assert not np.any(out["status"] == orc.STATUS_NUMERICAL), out["status"]
    below = 0
    for b, r in enumerate(refs):
        i = 2 * b
        kind = dt.check_contract((name, b, r["eps"]), out["u"][i], out["x"][i], out["y"][i], int(out["status"][i]), int(out["iters"][i]), r, ct[i], p, "f64", x0[i])
        assert kind == "answered"
        below += not r["ratio"] > orc.GUARD_RATIO_F64
    assert below >= 2, below                                        # the batch does reach below the guard
    # the healthy half: untouched by its neighbours, and right
    assert all(np.array_equal(out[k][1::2], alone[k]) for k in KEYS), "the healthy QPs beside the ladder differ from a solve of them alone"
    hx0, hxr, hft, hct = dt.healthy(name)
    for b in range(hx0.shape[0]):
        qp = orc.build_qp(p, hx0[b], hxr[b], hft[b], hct[b])
        xs, _ = orc.solve_reference(p, qp)
        href = dict(us=(xs * p.force_scale).reshape(N, 12), qp=qp, must_answer=False, ratio=np.inf)
        assert dt.check_contract((name, "healthy", b), alone["u"][b], alone["x"][b], alone["y"][b], int(alone["status"][b]), int(alone["iters"][b]), href, hct[b], p, "f64",
                                 hx0[b]) == "answered"


@pytest.mark.parametrize("name", ["n4_double", "n8_mixed", "n10_mixed", "n10_three", "n12_mixed", "n20_double"])
def test_every_rung_is_answered(torch_first, built_lib, name):
    _run(name, _engine(dt.BATCHES[name]["N"]))


def test_restart_passes_on_the_tail_stream(torch_first, built_lib):
    """n10_mixed with the automatic rho restart, device buffers, SRBDQP_FLAG_DEFER_TAIL plus flush: every pass launches the rank-aware instantiation."""
    from g1_locomotion_amd import _lib
    torch = torch_first

    def solve(eng, x0, xr, ft, ct):
        dev = torch.device("cuda", 0)
        B, N = x0.shape[0], xr.shape[1]
        d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (x0, xr, ft, ct)]
        u = torch.zeros((B, N, 12), dtype=torch.float64, device=dev); x = torch.zeros((B, N + 1, 13), dtype=torch.float64, device=dev)
        y = torch.zeros((B, 20 * N), dtype=torch.float64, device=dev)
        st = torch.full((B,), -77, dtype=torch.int32, device=dev); it = torch.full((B,), -77, dtype=torch.int32, device=dev)
        eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), x_out=x.data_ptr(), y_out=y.data_ptr(),
                         status=st.data_ptr(), iters=it.data_ptr())
        eng.flush()
        eng.synchronize()
        torch.cuda.synchronize(dev)
        return dict(u=u.cpu().numpy(), x=x.cpu().numpy(), y=y.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy())

    _run("n10_mixed", _engine(10, rho_restart_iter=0, flags=_lib.FLAG_DEFER_TAIL), solve=solve, restart=True)


def test_mpc_update_on_feet_in_tandem(torch_first, built_lib):
    """MPC(rank_aware=True).update() on the exactly collinear tandem rung with double support on every step: an answer through the HIP launch of the batch
    instantiation; without the keyword the same call ends with status -1."""
    from g1_locomotion_amd import MPC
    x0, xr, ft, ct, meta = dt.inputs("n10_double")
    refs, p = dt.reference("n10_double", "f64")
    b = [i for i, (g, eps) in enumerate(meta) if g == 0 and eps == 0.0][0]
    assert np.all(ct[b] != 0) and not refs[b]["ratio"] > orc.GUARD_RATIO_F64
    M = MPC(dt=0.04, horizon=10, strict=False, rank_aware=True, rho_restart_iter=-1)
    try:
        M.x_ref_hor = xr[b].copy()
        u0, x1 = M.update(ct[b], ft[b], None, x_current=x0[b].reshape(13, 1))
        assert M._engine.kernel_name() == "wrench_f64_n10_ra", M._engine.kernel_name()
        assert M._engine.batch1_launch_path().startswith("hip: ") and "SRBDQP_FLAG_RANK_AWARE" in M._engine.batch1_launch_path()
        assert M.status == orc.STATUS_SOLVED
        assert np.abs(np.asarray(u0).reshape(12) - refs[b]["us"][0]).max() <= dt.BOUND["f64"]
        assert np.abs(M.u_opt - refs[b]["us"]).max() <= dt.BOUND["f64"]
    finally:
        M.close()
    M = MPC(dt=0.04, horizon=10, strict=False, rho_restart_iter=-1)
    try:
        M.x_ref_hor = xr[b].copy()
        M.update(ct[b], ft[b], None, x_current=x0[b].reshape(13, 1))
        assert M.status == orc.STATUS_NUMERICAL
    finally:
        M.close()


def test_calls_without_a_rank_aware_form_are_refused(torch_first, built_lib):
    from g1_locomotion_amd import BatchMPC, RaggedMPC, SrbdqpError, _lib
    from g1_locomotion_amd.mpc import robots_array
    import side_inputs as si
    x0, xr, ft, ct = orc.synthetic_batch(2, 10, seed=3, schedule="double")
    flag = "SRBDQP_FLAG_RANK_AWARE"
    with _engine(10) as eng:
        with pytest.raises(SrbdqpError, match=flag):
            eng.solve(x0, xr, ft, ct, dtype=np.float32)
        with pytest.raises(SrbdqpError, match=flag):
            eng.assemble_wrench(x0, xr, ft, ct)
        with pytest.raises(SrbdqpError, match=flag):
            eng.set_robots(robots_array(2))
        with pytest.raises(SrbdqpError, match=flag):
            eng.set_contact_normals(si.flat_normals(2, 10))
        eng.set_robots(None); eng.set_contact_normals(None)         # clearing what was never set stays allowed
        out = eng.solve(x0, xr, ft, ct)                             # ... and the handle still solves
        assert np.all(out["status"] == orc.STATUS_SOLVED) and eng.kernel_name() == "wrench_f64_n10_ra"
    for kw in (dict(horizon=24), dict(horizon=7), dict(horizon=24, kernel=_lib.KERNEL_AUTO)):
        with pytest.raises(SrbdqpError, match=flag):
            BatchMPC(rank_aware=True, **kw)
    with pytest.raises(SrbdqpError, match=flag):
        RaggedMPC(horizons=(8, 12), flags=_lib.FLAG_RANK_AWARE)
    # AUTO: what it sends to the dense kernels is unchanged, what it sends to the general kernel runs the rank-aware instantiation
    with BatchMPC(horizon=10, rank_aware=True) as eng:
        xs, xrs, fts, cts = orc.synthetic_batch(4, 10, seed=4, schedule="single")
        eng.solve(xs, xrs, fts, cts)
        assert eng.kernel_name().startswith("wave_"), eng.kernel_name()
    with BatchMPC(horizon=12, rank_aware=True) as eng:
        xs, xrs, fts, cts = orc.synthetic_batch(4, 12, seed=4, schedule="double")
        eng.solve(xs, xrs, fts, cts)
        assert eng.kernel_name() == "wrench_f64_n12_ra", eng.kernel_name()
