"""The one-wave kernels factor K tile by tile and invert every 16 x 16 diagonal tile with the packed DPP elimination (srbdqp_mfma.hpp,
diag16_invert_dpp_packed).  Every tile count and padding the routine meets, in batches of 64 QPs through KERNEL_WAVE:

  N = 10  the batch of test_gpu_wave_mask_branch.py: n_eff = 60 / 54 / 48, four tiles, the last one partly padded (12, 6 or 0 real rows), and at least one
          continued pass in every group (a second and third factorisation with a re-balanced rho),
  N = 8   single support: n_eff = 48, exactly three full tiles,
  N = 4   single support: n_eff = 24, two tiles, the second half padded,

on a default handle (the restart in place) and with SRBDQP_FLAG_DEFER_TAIL + flush() (the deferred-tail kernel), against the compiled oracle on the terms of
test_gpu_wave_mask_branch.py.  The two handles run the same passes with the same arithmetic: they agree bit for bit.  The seeds were picked on the CPU so that
the oracle solves every QP; the CPU-only test below asserts that, and the continued passes of the N = 10 groups."""
import numpy as np
import pytest

import srbd_oracle as orc
from test_gpu_wave_mask_branch import B, TOL_TWIN_N, mask_branch_batch, torch_first  # noqa: F401  (one batch, one bound and one fixture for both files)

CASES = {"n10_masked": 10, "n8_three_full_tiles": 8, "n4_half_padded": 4}
SEED = 9200


def _batch(case):
    if case == "n10_masked":
        return mask_branch_batch()
    return orc.synthetic_batch(B, CASES[case], seed=SEED, schedule="single")


_REF = {}


def _reference(case):
    """The batch, the oracle's parameters and its solution: computed once per case, shared read-only."""
    if case not in _REF:
        import c_oracle
        inputs = _batch(case)
        p = orc.default_params(CASES[case])             # the twin of the engine's defaults (rho restart on)
        ref = c_oracle.solve_batch(p, *inputs, nthreads=8)
        for v in list(inputs) + list(ref.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[case] = (inputs, p, ref)
    return _REF[case]


@pytest.mark.parametrize("case", list(CASES))
def test_the_oracle_solves_every_qp_of_the_batches(case):
    (x0, xr, ft, ct), p, ref = _reference(case)
    n_eff = 3 * ct.reshape(B, -1).sum(1)
    if case == "n10_masked":
        assert np.all(n_eff[:32] == 60) and np.all(n_eff[32:48] == 54) and np.all(n_eff[48:] == 48)
        for g in (slice(0, 32), slice(32, 48), slice(48, 64)):
            assert (ref["iters"][g] > p.rho_restart_iter).any()      # a continued pass in every group
    else:
        assert np.all(n_eff == 6 * CASES[case])
    assert np.all(ref["status"] == orc.STATUS_SOLVED)


def _run(torch, N, flags, inputs):   # (test_gpu_wave_mask_branch.py's launcher, for any horizon)
    from g1_locomotion_amd import BatchMPC, _lib
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.array(v)).to(dev) for v in inputs]
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


@pytest.fixture(scope="module", params=list(CASES))
def gpu_outputs(request, torch_first, built_lib):
    from g1_locomotion_amd import _lib
    case = request.param
    inputs = _reference(case)[0]
    plain, kp = _run(torch_first, CASES[case], 0, inputs)
    defer, kd = _run(torch_first, CASES[case], _lib.FLAG_DEFER_TAIL, inputs)
    assert kp.startswith("wave_f64"), kp
    assert kd.startswith("wave_defer_f64"), kd
    return case, dict(plain=plain, defer=defer)


@pytest.mark.gpu
@pytest.mark.parametrize("handle", ["plain", "defer"])
def test_every_tile_shape_against_the_oracle(gpu_outputs, handle):
    case, outs = gpu_outputs
    (x0, xr, ft, ct), p, ref = _reference(case)
    N = CASES[case]
    out = outs[handle]
    d = np.abs(out["iters"].astype(int) - ref["iters"].astype(int))
    err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
    print(case, handle, "max |iters - oracle|", d.max(), " max |u - oracle|", err.max(), "N")
    np.testing.assert_array_equal(out["status"], ref["status"])
    assert d.max() <= p.check_every
    assert err.max() <= TOL_TWIN_N, err.max()
    assert np.all(out["u"].reshape(B, N, 4, 3)[ct == 0] == 0.0)


@pytest.mark.gpu
def test_the_two_handles_agree_bit_for_bit(gpu_outputs):
    case, outs = gpu_outputs
    a, b = outs["plain"], outs["defer"]
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["iters"], b["iters"])
    assert np.array_equal(a["u"].view(np.uint64), b["u"].view(np.uint64))
    assert np.array_equal(a["x"].view(np.uint64), b["x"].view(np.uint64))
