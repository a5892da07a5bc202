"""The one-wave kernels form their set-up tables on step PAIRS (csrc/srbdqp_setup1.hpp: a lane per pair (m, i >= m), lane m adds up its pairs in ascending i;
tests/test_wave_front_end_cpu.py restates the scheme).  Here the kernels themselves, on the shapes where a pair mapping can go wrong: per horizon N = 4, 8, 10
one batch of 64 single-support QPs of which

  QP 0  has its only stance step first,          QP 1  its only stance step last,
  QP 2  a flight step in the middle,             QP 3  one contact per step,

so that n_eff < KS on those four (the K^-1 row masks applied) and n_eff == KS on the other sixty; N = 4 also in double support (four contacts per step: the
MAXS = 4 instantiation of the one-wave kernel) and N = 10 in double support (four contacts per step at N = 10: beyond one wave, the 4-wave kernel).  The assembly
dump (srbdqp_assemble_f64) against closed_form_hessian_rank6 / closed_form_hessian_gradient to 1e-11 of the largest entry; full solves, a caller's warm start
(the second call of gt_tables) and the two-phase call (the PHI instantiation: thirteen more) against the oracle: statuses and iteration counts equal, forces
to the twin bound of the parity tests."""
import numpy as np
import pytest

import srbd_oracle as orc
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TOL_TWIN_N = 2e-3
B = 64
CASES = {"n4": (4, "single"), "n8": (8, "single"), "n10": (10, "single"), "n4_four_contacts": (4, "double"), "n10_four_contacts": (10, "double")}
ONE_WAVE = ("n4", "n8", "n10", "n4_four_contacts")


def _batch(case):
    N, schedule = CASES[case]
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=9300 + N + (100 if schedule == "double" else 0), schedule=schedule)
    ct = ct.reshape(B, N, 4).copy()
    if schedule == "single":
        ct[0, 1:, :] = 0                                   # only the first step in stance
        ct[1, :-1, :] = 0                                  # only the last
        ct[2, N // 2, :] = 0                               # a flight step in the middle
        for k in range(N):                                 # one contact per step
            on = np.flatnonzero(ct[3, k])
            ct[3, k, on[1:]] = 0
    return x0, xr, ft, ct


_REF = {}


def _reference(case):
    """The batch, the oracle's parameters and its solution: computed once per case, shared read-only."""
    if case not in _REF:
        import c_oracle
        inputs = _batch(case)
        p = orc.default_params(CASES[case][0])              # the twin of the engine's defaults (rho restart on)
        ref = c_oracle.solve_batch(p, *inputs, nthreads=8)
        for v in list(inputs) + list(ref.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[case] = (inputs, p, ref)
    return _REF[case]


def test_the_batches_hold_the_shapes():
    for case in ("n4", "n8", "n10"):
        (x0, xr, ft, ct), p, ref = _reference(case)
        N = CASES[case][0]
        per_step = ct.reshape(B, N, 4).sum(2)
        assert per_step[0].tolist() == [2] + [0] * (N - 1) and per_step[1].tolist() == [0] * (N - 1) + [2]
        assert per_step[2, N // 2] == 0 and (np.delete(per_step[2], N // 2) == 2).all()
        assert (per_step[3] == 1).all() and (per_step[4:] == 2).all()
        assert (3 * per_step[:4].sum(1) < 6 * N).all()            # n_eff < KS: the masked side of the branch
    for case in ("n4_four_contacts", "n10_four_contacts"):
        assert (_reference(case)[0][3].reshape(B, -1, 4).sum(2) == 4).all()


@pytest.mark.parametrize("case", ONE_WAVE)
def test_assembly_dump_against_the_closed_forms(torch_first, built_lib, case):
    from g1_locomotion_amd import BatchMPC, _lib
    (x0, xr, ft, ct), p, ref = _reference(case)
    N = CASES[case][0]
    nb = 8                                                      # the four special shapes and four full ones
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WAVE) as eng:
        got = eng.assemble(x0[:nb], xr[:nb], ft[:nb], ct[:nb])
        assert eng.kernel_name().startswith("wave_"), eng.kernel_name()
    worst_p = worst_q = 0.0
    for b in range(nb):
        P6 = orc.closed_form_hessian_rank6(p, xr[b], ft[b], ct[b])
        _, q, vi = orc.closed_form_hessian_gradient(p, x0[b], xr[b], ft[b], ct[b])
        ep = np.abs(got["P"][b][np.ix_(vi, vi)] - P6).max() / np.abs(P6).max()
        eq = np.abs(got["q"][b][vi] - q).max() / np.abs(q).max()
        worst_p, worst_q = max(worst_p, ep), max(worst_q, eq)
        assert ep <= 1e-11 and eq <= 1e-11, (case, b, ep, eq)
        off = np.setdiff1d(np.arange(12 * N), vi)
        assert np.all(got["P"][b][off, :] == 0.0) and np.all(got["P"][b][:, off] == 0.0) and np.all(got["q"][b][off] == 0.0)
    print(case, "max relative error of K", worst_p, " of q", worst_q)


def _run(torch, N, maxs, kernel, flags, inputs):
    from g1_locomotion_amd import BatchMPC, _lib
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.array(v)).to(dev) for v in inputs]
    u = torch.zeros((B, N, 12), dtype=torch.float64, device=dev)
    st = torch.full((B,), -77, dtype=torch.int32, device=dev)
    it = torch.zeros(B, dtype=torch.int32, device=dev)
    with BatchMPC(horizon=N, max_contacts_per_step=maxs, kernel=kernel, flags=flags) as eng:
        eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), status=st.data_ptr(), iters=it.data_ptr())
        if flags & _lib.FLAG_DEFER_TAIL:
            eng.flush()
        eng.synchronize()
        torch.cuda.synchronize(dev)
        name = eng.kernel_name()
    return dict(u=u.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy()), name


@pytest.mark.parametrize("handle", ["plain", "defer"])
@pytest.mark.parametrize("case", list(CASES))
def test_full_solves_against_the_oracle(torch_first, built_lib, case, handle):
    from g1_locomotion_amd import _lib
    (x0, xr, ft, ct), p, ref = _reference(case)
    N, schedule = CASES[case]
    out, name = _run(torch_first, N, 2 if schedule == "single" else 4, _lib.KERNEL_WAVE if case in ONE_WAVE else _lib.KERNEL_AUTO,
                     _lib.FLAG_DEFER_TAIL if handle == "defer" else 0, (x0, xr, ft, ct))
    if case in ONE_WAVE:
        assert name.startswith("wave_defer_f64" if handle == "defer" else "wave_f64"), name
    d = np.abs(out["iters"].astype(int) - ref["iters"].astype(int))
    err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
    print(case, handle, name, "QPs whose iteration count differs from the oracle's", int((d != 0).sum()), "max", d.max(), " max |u - oracle|", err.max(), "N")
    np.testing.assert_array_equal(out["status"], ref["status"])
    np.testing.assert_array_equal(out["iters"], ref["iters"])
    assert err.max() <= TOL_TWIN_N, err.max()
    assert np.all(out["u"].reshape(B, N, 4, 3)[ct == 0] == 0.0)


def test_a_callers_warm_start(torch_first, built_lib):
    """warm_u / warm_y from a solve that stopped early: P x^0 goes through gt_tables a second time"""
    from g1_locomotion_amd import BatchMPC, _lib
    (x0, xr, ft, ct), p, ref = _reference("n10")
    nb, N = 8, 10
    a = (x0[:nb], xr[:nb], ft[:nb], ct[:nb])
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WAVE, max_iter=10) as eng:
        rough = eng.solve(*a, want_y=True)
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WAVE) as eng:
        warm = eng.solve(*a, warm_u=rough["u"].reshape(nb, -1), warm_y=rough["y"])
        assert eng.kernel_name().startswith("wave_"), eng.kernel_name()
    for b in range(nb):
        o = orc.update(p, x0[b], xr[b], ft[b], ct[b], warm=(rough["u"][b].reshape(-1) / p.force_scale, rough["y"][b]))
        e = np.abs(warm["u"][b] - o["u"]).max()
        print("warm start, QP", b, "iterations", int(warm["iters"][b]), "oracle", o["iters"], " |u - oracle|", e, "N")
        assert warm["status"][b] == o["status"] and warm["iters"][b] == o["iters"], (b, warm["status"][b], o["status"], warm["iters"][b], o["iters"])
        assert e <= TOL_TWIN_N


def test_the_two_phase_call(torch_first, built_lib):
    """srbdqp_prepare_staged_f64 (the split pipeline's set-up with dq / dx0: gt_tables once per column) + srbdqp_solve_prepared_f64: the set-up
    sees a WRONG predicted state (the perturbation of test_gpu_parity.py's two-phase test), so the second phase patches q with phi (x0 - x0_pred) and a wrong column of
    phi moves the forces"""
    from g1_locomotion_amd import BatchMPC
    (x0, xr, ft, ct), p, ref = _reference("n10")
    nb, N = 8, 10
    pp = orc.params_for(N)                                      # (no rho restart on this path, as in test_gpu_parity.py's two-phase test)
    with BatchMPC(horizon=N, rho_restart_iter=-1) as eng:
        st = eng.stage()
        assert st["capacity"] >= nb
        st["x_ref"][:nb] = xr[:nb]; st["foot"][:nb] = ft[:nb].reshape(nb, N, 12); st["contact"][:nb] = ct[:nb].reshape(nb, N, 4)
        rng = np.random.default_rng(9310)
        st["x0"][:nb] = x0[:nb] + rng.normal(size=x0[:nb].shape) * np.array([0.2] * 3 + [0.05] * 3 + [0.5] * 6 + [0.0])     # the prediction: off
        eng.prepare_staged(nb)
        assert eng.kernel_name().startswith("prepare_f64_n"), eng.kernel_name()
        st["x0"][:nb] = x0[:nb]                                                                                               # the measurement
        eng.solve_prepared(nb, want_x=True)
        u, status, iters = st["u"][:nb].copy(), st["status"][:nb].copy(), st["iters"][:nb].copy()
    twin = [orc.update(pp, x0[b], xr[b], ft[b], ct[b]) for b in range(nb)]
    err = max(np.abs(u[b] - twin[b]["u"]).max() for b in range(nb))
    print("two-phase call: iterations", iters.tolist(), "oracle", [o["iters"] for o in twin], " max |u - oracle|", err, "N")
    assert status.tolist() == [o["status"] for o in twin]
    assert iters.tolist() == [o["iters"] for o in twin]
    assert err <= TOL_TWIN_N
