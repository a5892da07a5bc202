"""The one-wave kernel's set-up (register linearisation, per-step tables in registers, K^-1 from its upper triangle) on a full
configs[1]-sized batch: 4096 single-support QPs at N = 10 with the engine's default rho restart, against the compiled oracle, with
the committed golden QPs placed inside the batch."""
import os

import numpy as np
import pytest

import srbd_oracle as orc
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TOL_TWIN_N = 2e-3


def test_wave_kernel_4096_single_support_against_oracle_and_golden(torch_first, built_lib):
    import c_oracle
    from g1_locomotion_amd import BatchMPC, _lib
    B, N = 4096, 10
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=6100, schedule="single")
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "srbd_qp_golden.npz"))
    slots = {"n10_single_a": 0, "n10_single_b": B - 1}
    for name, b in slots.items():
        x0[b], xr[b], ft[b], ct[b] = (gold[f"{name}/{k}"] for k in ("x0", "x_ref", "foot", "contact"))
    p = orc.default_params(N)                       # the twin of the engine's defaults (rho restart on)
    ref = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=8)
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WAVE) as eng:
        out = eng.solve(x0, xr, ft, ct)
        assert eng.kernel_name().startswith("wave_"), eng.kernel_name()
    np.testing.assert_array_equal(out["status"], ref["status"])
    d = np.abs(out["iters"].astype(int) - ref["iters"].astype(int))
    assert d.max() <= p.check_every
    same = d == 0
    assert same.mean() > 0.97
    err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
    assert err[same].max() <= 1e-4 and err.max() <= TOL_TWIN_N, (err[same].max(), err.max())
    assert np.abs(out["x"] - ref["x"]).max() <= 1e-5
    assert np.all(out["u"].reshape(B, N, 4, 3)[ct == 0] == 0.0)
    for name, b in slots.items():                   # the golden QPs: exact optimum and frozen ADMM twin (test_gpu_parity.py's tolerances)
        assert out["status"][b] == orc.STATUS_SOLVED
        assert np.abs(out["u"][b] - gold[f"{name}/u_exact"]).max() <= 5e-2
        assert np.abs(out["x"][b] - gold[f"{name}/x_exact"]).max() <= 1e-4
