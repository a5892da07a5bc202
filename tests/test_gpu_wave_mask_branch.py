"""The one-wave kernels mask the lane's K^-1 row only when the QP has fewer presolved variables than the row has columns (n_eff < KS: a
wave-uniform branch in front of the ADMM).  Both sides of that branch in ONE batch of 64 QPs at N = 10: 32 single-support QPs (n_eff == KS = 60, the
masks skipped) and 32 whose contact flags are all zero on one or two steps (n_eff = 54 or 48, the masks applied), on a default handle (the restart in
place) and with SRBDQP_FLAG_DEFER_TAIL + flush() (the deferred-tail kernel), against the compiled oracle on the terms of
test_gpu_wave_setup_parity.py.  The two handles run the same passes with the same arithmetic: they agree bit for bit."""
import numpy as np
import pytest

import srbd_oracle as orc
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TOL_TWIN_N = 2e-3
B, N = 64, 10


def mask_branch_batch():
    """QPs 0..31: single support as drawn; 32..47: step b % N in flight; 48..63: steps b % N and (b + 3) % N in flight.  (The seed: the oracle solves
    all 64, and in each of the three groups at least one QP passes the first rho-restart mark, so the continued passes take the branch both ways too.)"""
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=9117, schedule="single")
    for b in range(32, B):
        ct[b, b % N, :] = 0
        if b >= 48:
            ct[b, (b + 3) % N, :] = 0
    return x0, xr, ft, ct


@pytest.fixture(scope="module")
def batch_and_reference():
    import c_oracle
    x0, xr, ft, ct = mask_branch_batch()
    p = orc.default_params(N)                       # the twin of the engine's defaults (rho restart on)
    ref = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=8)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return (x0, xr, ft, ct), p, ref


def _run(torch, flags, inputs):
    from g1_locomotion_amd import BatchMPC, _lib
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(v).to(dev) for v in inputs]
    u = torch.zeros((B, N, 12), dtype=torch.float64, device=dev)
    x = torch.zeros((B, N + 1, 13), dtype=torch.float64, device=dev)
    st = torch.full((B,), -77, dtype=torch.int32, device=dev)
    it = torch.zeros(B, dtype=torch.int32, device=dev)
    with BatchMPC(horizon=N, max_contacts_per_step=2, kernel=_lib.KERNEL_WAVE, flags=flags) as eng:
        eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), x_out=x.data_ptr(),
                         status=st.data_ptr(), iters=it.data_ptr())
        if flags & _lib.FLAG_DEFER_TAIL:
            eng.flush()
        eng.synchronize()
        torch.cuda.synchronize(dev)
        name = eng.kernel_name()
    return dict(u=u.cpu().numpy(), x=x.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy()), name


@pytest.fixture(scope="module")
def gpu_outputs(torch_first, built_lib, batch_and_reference):
    from g1_locomotion_amd import _lib
    inputs = batch_and_reference[0]
    plain, kp = _run(torch_first, 0, inputs)
    defer, kd = _run(torch_first, _lib.FLAG_DEFER_TAIL, inputs)
    assert kp.startswith("wave_f64"), kp
    assert kd.startswith("wave_defer_f64"), kd
    return dict(plain=plain, defer=defer)


def test_batch_takes_both_sides_of_the_branch(batch_and_reference):
    (x0, xr, ft, ct), p, ref = batch_and_reference
    n_eff = 3 * ct.reshape(B, -1).sum(1)
    assert np.all(n_eff[:32] == 60) and np.all(n_eff[32:48] == 54) and np.all(n_eff[48:] == 48)
    assert np.all(ref["status"] == orc.STATUS_SOLVED)            # the comparison below is on solved QPs throughout
    for g in (slice(0, 32), slice(32, 48), slice(48, 64)):
        assert (ref["iters"][g] > p.rho_restart_iter).any()      # a continued pass in every group


@pytest.mark.parametrize("handle", ["plain", "defer"])
def test_both_sides_against_the_oracle(gpu_outputs, batch_and_reference, handle):
    (x0, xr, ft, ct), p, ref = batch_and_reference
    out = gpu_outputs[handle]
    np.testing.assert_array_equal(out["status"], ref["status"])
    d = np.abs(out["iters"].astype(int) - ref["iters"].astype(int))
    err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
    print(handle, "max |iters - oracle|", d.max(), " max |u - oracle| full", err[:32].max(), "N  masked", err[32:].max(), "N")
    assert d.max() <= p.check_every
    assert err.max() <= TOL_TWIN_N, err.max()
    assert np.all(out["u"].reshape(B, N, 4, 3)[ct == 0] == 0.0)


def test_the_two_handles_agree_bit_for_bit(gpu_outputs):
    a, b = gpu_outputs["plain"], gpu_outputs["defer"]
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["iters"], b["iters"])
    assert np.array_equal(a["u"].view(np.uint64), b["u"].view(np.uint64))
    assert np.array_equal(a["x"].view(np.uint64), b["x"].view(np.uint64))
