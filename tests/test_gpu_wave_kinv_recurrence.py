"""The one-wave kernels form K^-1 by block recurrence from the Cholesky factor (csrc/srbdqp_setup1.hpp, phases F and I: P_j = W_jj' W_jj and V_lj = U_jl' W_jj
on the way out of F, then X_jb = delta_jb P_j - sum_{l>j} V_lj' X_lb block column by block column, the blocks below a column's diagonal read back transposed
from the staging tiles; tests/test_kinv_recurrence_cpu.py restates the scheme and holds its accuracy to the scheme it replaced).  Here the kernels themselves, on
the batches of tests/test_gpu_wave_front_end.py (64 QPs; QPs 0 - 3 of the single-support ones have n_eff < KS) and on one more whose every QP has a swing step:

  n4 (NT = 2)   n4_four_contacts (MAXS = 4, NT = 3)   n8 (NT = 3, n_eff = 16 NT)   n10 (NT = 4)   n10_swing (NT = 4, n_eff = 54 < KS on every QP)

each through every instantiation that runs the phases -- the restart kernel, the deferred-tail kernel with a flush, the split pipeline's set-up (FUSED = false:
K^-1 stored to the workspace, both triangles), a caller's warm start and the two-phase prepared call (PHI) -- against the oracle: statuses and iteration
counts equal on every QP, forces within the twin bound of the parity tests.  Then the same with the rho restart after 20 iterations, so that nearly every QP runs
continued passes: K^-1 at a re-balanced rho (RP = 2 in place, RP = 3 in a workgroup of the flush)."""
import numpy as np
import pytest

import srbd_oracle as orc
import test_gpu_wave_front_end as fe
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TOL_TWIN_N = 2e-3
B = fe.B
CASES = {"n4": ("n4", 2), "n4_four_contacts": ("n4_four_contacts", 4), "n8": ("n8", 2), "n10": ("n10", 2), "n10_swing": ("n10", 2)}
EARLY = dict(rho_restart_iter=20, rho_restart_count=3)            # (a multiple of check_every; three re-balancings: all the kernel has copies of the body for)
NB = 8                                                           # QPs of the warm-start and two-phase runs: the four special shapes and four full ones

_REF = {}


def _inputs(case):
    base, maxs = CASES[case]
    x0, xr, ft, ct = fe._batch(base)
    N = fe.CASES[base][0]
    if case == "n10_swing":
        ct = ct.copy()
        ct[4:, N // 2, :] = 0                                    # (QPs 0 - 3 keep their shapes)
    return N, maxs, (x0, xr, ft, ct)


def _reference(case, early):
    """The batch and the oracle's solution with the engine's default restart or the early one: computed once, shared read-only."""
    if (case, early) not in _REF:
        import c_oracle
        N, maxs, inputs = _inputs(case)
        p = orc.params_for(N, **EARLY) if early else orc.default_params(N)
        ref = c_oracle.solve_batch(p, *inputs, nthreads=8)
        for v in list(inputs) + list(ref.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[case, early] = (N, maxs, inputs, p, ref)
    return _REF[case, early]


def test_the_batches_hold_the_shapes():
    for case in CASES:
        N, maxs, (x0, xr, ft, ct), p, ref = _reference(case, False)
        n_eff = 3 * ct.reshape(B, -1).sum(1)
        ks = 3 * maxs * N
        assert (n_eff <= ks).all() and n_eff.min() > 0
        if case == "n10_swing":
            assert (n_eff < ks).all() and (n_eff[4:] == ks - 6).all()
        elif maxs == 2:
            assert (n_eff[:4] < ks).all() and (n_eff[4:] == ks).all()
        else:
            assert (n_eff == ks).all()
    N, maxs, inputs, p, ref = _reference("n10", True)
    assert (ref["iters"] > EARLY["rho_restart_iter"]).mean() > 0.5      # the continued passes run


def _run(torch, case, early, kernel, flags):
    from g1_locomotion_amd import BatchMPC, _lib
    N, maxs, inputs, p, ref = _reference(case, early)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.array(v)).to(dev) for v in inputs]
    u = torch.zeros((B, N, 12), dtype=torch.float64, device=dev)
    st = torch.full((B,), -77, dtype=torch.int32, device=dev)
    it = torch.zeros(B, dtype=torch.int32, device=dev)
    with BatchMPC(horizon=N, max_contacts_per_step=maxs, kernel=kernel, flags=flags, **(EARLY if early else {})) as eng:
        eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), status=st.data_ptr(), iters=it.data_ptr())
        if flags & _lib.FLAG_DEFER_TAIL:
            eng.flush()
        eng.synchronize()
        torch.cuda.synchronize(dev)
        name = eng.kernel_name()
    return dict(u=u.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy()), name


@pytest.mark.parametrize("early", [False, True], ids=["default_restart", "restart_after_20"])
@pytest.mark.parametrize("path", ["restart", "defer", "split"])
@pytest.mark.parametrize("case", list(CASES))
def test_full_solves_against_the_oracle(torch_first, built_lib, case, path, early):
    from g1_locomotion_amd import _lib
    N, maxs, (x0, xr, ft, ct), p, ref = _reference(case, early)
    kernel = _lib.KERNEL_SPLIT if path == "split" else _lib.KERNEL_WAVE
    out, name = _run(torch_first, case, early, kernel, _lib.FLAG_DEFER_TAIL if path == "defer" else 0)
    assert name.startswith({"restart": "wave_f64", "defer": "wave_defer_f64", "split": "split_f64"}[path]), name
    d = np.abs(out["iters"].astype(int) - ref["iters"].astype(int))
    err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
    print(case, path, name, "restart", (p.rho_restart_iter, p.rho_restart_count), "QPs past the first mark", int((ref["iters"] > p.rho_restart_iter).sum()),
          " iteration counts that differ from the oracle's", int((d != 0).sum()), "max", d.max(), " max |u - oracle|", err.max(), "N")
    np.testing.assert_array_equal(out["status"], ref["status"])
    np.testing.assert_array_equal(out["iters"], ref["iters"])
    assert err.max() <= TOL_TWIN_N, err.max()
    assert np.all(out["u"].reshape(B, N, 4, 3)[ct == 0] == 0.0)


@pytest.mark.parametrize("case", list(CASES))
def test_a_callers_warm_start(torch_first, built_lib, case):
    """warm_u / warm_y from a solve that stopped early"""
    from g1_locomotion_amd import BatchMPC, _lib
    N, maxs, (x0, xr, ft, ct), p, ref = _reference(case, False)
    a = (x0[:NB], xr[:NB], ft[:NB], ct[:NB])
    with BatchMPC(horizon=N, max_contacts_per_step=maxs, kernel=_lib.KERNEL_WAVE, max_iter=10) as eng:
        rough = eng.solve(*a, want_y=True)
    with BatchMPC(horizon=N, max_contacts_per_step=maxs, kernel=_lib.KERNEL_WAVE) as eng:
        warm = eng.solve(*a, warm_u=rough["u"].reshape(NB, -1), warm_y=rough["y"])
        assert eng.kernel_name().startswith("wave_"), eng.kernel_name()
    for b in range(NB):
        o = orc.update(p, x0[b], xr[b], ft[b], ct[b], warm=(rough["u"][b].reshape(-1) / p.force_scale, rough["y"][b]))
        e = np.abs(warm["u"][b] - o["u"]).max()
        print(case, "warm start, QP", b, "iterations", int(warm["iters"][b]), "oracle", o["iters"], " |u - oracle|", e, "N")
        assert warm["status"][b] == o["status"] and warm["iters"][b] == o["iters"], (b, warm["status"][b], o["status"], warm["iters"][b], o["iters"])
        assert e <= TOL_TWIN_N


@pytest.mark.parametrize("case", list(CASES))
def test_the_two_phase_call(torch_first, built_lib, case):
    """srbdqp_prepare_staged_f64 (FUSED = false with dq / dx0: K^-1 through the workspace) + srbdqp_solve_prepared_f64, the set-up from a WRONG predicted
    state as in tests/test_gpu_wave_front_end.py"""
    from g1_locomotion_amd import BatchMPC
    N, maxs, (x0, xr, ft, ct), p, ref = _reference(case, False)
    pp = orc.params_for(N)                                      # (no rho restart on this path)
    with BatchMPC(horizon=N, max_contacts_per_step=maxs, rho_restart_iter=-1) as eng:
        st = eng.stage()
        assert st["capacity"] >= NB
        st["x_ref"][:NB] = xr[:NB]; st["foot"][:NB] = ft[:NB].reshape(NB, N, 12); st["contact"][:NB] = ct[:NB].reshape(NB, N, 4)
        rng = np.random.default_rng(9320)
        st["x0"][:NB] = x0[:NB] + rng.normal(size=x0[:NB].shape) * np.array([0.2] * 3 + [0.05] * 3 + [0.5] * 6 + [0.0])     # the prediction: off
        eng.prepare_staged(NB)
        assert eng.kernel_name().startswith("prepare_f64_n"), eng.kernel_name()
        st["x0"][:NB] = x0[:NB]                                                                                               # the measurement
        eng.solve_prepared(NB, want_x=True)
        u, status, iters = st["u"][:NB].copy(), st["status"][:NB].copy(), st["iters"][:NB].copy()
    twin = [orc.update(pp, x0[b], xr[b], ft[b], ct[b]) for b in range(NB)]
    err = max(np.abs(u[b] - twin[b]["u"]).max() for b in range(NB))
    print(case, "two-phase call: iterations", iters.tolist(), "oracle", [o["iters"] for o in twin], " max |u - oracle|", err, "N")
    assert status.tolist() == [o["status"] for o in twin]
    assert iters.tolist() == [o["iters"] for o in twin]
    assert err <= TOL_TWIN_N
