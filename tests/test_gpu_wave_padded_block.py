"""The one-wave kernels without the padding of their last block (csrc/srbdqp_setup1.hpp: PAD = 16 NT - KS rows and columns of the last tile are padding for every
QP, so the last diagonal tile's elimination runs 16 - PAD pivots and the products that contract over block row NT - 1 leave PAD / 4 k-steps out;
tests/test_wave_padded_block_cpu.py restates both forms and holds them to each other bit for bit).  Here the kernels themselves, 64 QPs a case against the oracle
as tests/test_gpu_wave_setup_diet.py runs them -- through the restart in place, the deferred tails with a flush and the split set-up (FUSED = false): statuses
and iteration counts equal to the oracle's and to each other, max |u - oracle| <= 2e-3 N -- on the smallest shapes at which the arm can go wrong:

  n4                 N = 4, MAXS = 2: KS = 24, NT = 2, PAD = 8 -- TWO k-steps and eight pivots left out (PAD >= 8 skips two: every row at or beyond KS is padding)
  n4_four_contacts   N = 4, MAXS = 4: KS = 48, NT = 3, PAD = 0 -- the arm compiles away
  n8                 N = 8, MAXS = 2: KS = 48, PAD = 0
  n10                N = 10, MAXS = 2: KS = 60, NT = 4, PAD = 4; QPs 4 .. 63 in full single support (n_eff = 60), QPs 0 .. 3 with n_eff < 60
  n10_swing          a swing step on every QP: n_eff = 54, real zero rows beside the padding, inside the live k-steps
  n10_flight         the n10 batch with QP 5 in flight over the whole horizon (n_eff = 0: the pass ends before F) and QP 6 in flight over its first half

then n4 and n10 with rho_restart_iter = 20, so that nearly every QP runs continued passes (the shortened F at a re-balanced rho: RP = 2 in place, RP = 3 in a
workgroup of the flush), and the n10 batch with a NaN in x_ref of one QP and an infinite stance-foot position in another: those two end SRBDQP_NUMERICAL with
forces exactly 0 (include/srbdqp.h), every other QP keeps the bits of the clean solve."""
import numpy as np
import pytest

import srbd_oracle as orc
import test_gpu_wave_front_end as fe
import test_gpu_wave_kinv_recurrence as kr
import test_gpu_wave_setup_diet as sd
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TOL_TWIN_N = 2e-3
B = kr.B
SHAPES = {"n4": (24, 2, 8), "n4_four_contacts": (48, 3, 0), "n8": (48, 3, 0), "n10": (60, 4, 4), "n10_swing": (60, 4, 4)}     # KS, NT, PAD


def test_the_cases_hold_the_shapes():
    for case, (ks, nt, pad) in SHAPES.items():
        N, maxs, (x0, xr, ft, ct), p, ref = kr._reference(case, False)
        assert 3 * maxs * N == ks and (ks + 15) // 16 == nt and 16 * nt - ks == pad
        n_eff = 3 * ct.reshape(B, -1).sum(1)
        if case == "n10":
            assert (n_eff[4:] == 60).all() and (n_eff[:4] < 60).all()
        if case == "n10_swing":
            assert (n_eff[4:] == 54).all()


@pytest.mark.parametrize("case", list(SHAPES))
def test_restart_defer_and_split_against_the_oracle(torch_first, built_lib, case):
    N, maxs, (x0, xr, ft, ct), p, ref = kr._reference(case, False)
    sd._three_paths(torch_first, lambda kernel, flags: kr._run(torch_first, case, False, kernel, flags), ref, ct, N, case)


_FLIGHT = {}


def _flight_batch():
    if not _FLIGHT:
        import c_oracle
        x0, xr, ft, ct = fe._batch("n10")
        ct = ct.copy()
        ct[5] = 0                                             # n_eff = 0
        ct[6, :5] = 0                                         # n_eff = 30: two whole tiles of K are padding-like beside the real padding
        ref = c_oracle.solve_batch(orc.default_params(10), x0, xr, ft, ct, nthreads=8)
        for v in [x0, xr, ft, ct] + list(ref.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FLIGHT["v"] = ((x0, xr, ft, ct), ref)
    return _FLIGHT["v"]


def test_a_flight_phase(torch_first, built_lib):
    inputs, ref = _flight_batch()
    ct = inputs[3]
    assert ct[5].sum() == 0 and 3 * ct[6].sum() == 30
    # (QP 5: status and iteration count equal to the oracle's, forces exactly 0 by the helper's ct == 0 check)
    sd._three_paths(torch_first, lambda kernel, flags: fe._run(torch_first, 10, 2, kernel, flags, inputs), ref, ct, 10, "n10_flight")


@pytest.mark.parametrize("path", ["restart", "defer", "split"])
@pytest.mark.parametrize("case", ["n4", "n10"])
def test_continued_passes_at_a_rebalanced_rho(torch_first, built_lib, case, path):
    """rho_restart_iter = 20: the shortened F and I again in every continued pass"""
    from g1_locomotion_amd import _lib
    N, maxs, (x0, xr, ft, ct), p, ref = kr._reference(case, True)
    assert p.rho_restart_iter == 20 and (ref["iters"] > 20).mean() > 0.5
    out, name = kr._run(torch_first, case, True, _lib.KERNEL_SPLIT if path == "split" else _lib.KERNEL_WAVE, _lib.FLAG_DEFER_TAIL if path == "defer" else 0)
    assert name.startswith(sd.PATHS[path]), name
    err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
    print(case, path, name, "QPs past the first mark", int((ref["iters"] > 20).sum()), " max |u - oracle|", err.max(), "N")
    np.testing.assert_array_equal(out["status"], ref["status"])
    np.testing.assert_array_equal(out["iters"], ref["iters"])
    assert err.max() <= TOL_TWIN_N, err.max()


@pytest.mark.parametrize("path", ["restart", "defer"])
def test_a_nan_in_x_ref_and_an_infinite_foot(torch_first, built_lib, path):
    from g1_locomotion_amd import _lib
    x0, xr, ft, ct = fe._batch("n10")
    flags = _lib.FLAG_DEFER_TAIL if path == "defer" else 0
    clean, name = fe._run(torch_first, 10, 2, _lib.KERNEL_WAVE, flags, (x0, xr, ft, ct))
    assert name.startswith(sd.PATHS[path]), name
    xr2, ft2 = xr.copy(), np.array(ft, copy=True)
    qn, qi = 7, 9
    xr2[qn, 9, 7] = np.nan                                    # an angular velocity of the last step's reference
    k = 5
    c = int(np.flatnonzero(ct[qi, k])[0])                     # a stance contact of step 5
    ft2.reshape(B, 10, 4, 3)[qi, k, c, 1] = np.inf
    out, _ = fe._run(torch_first, 10, 2, _lib.KERNEL_WAVE, flags, (x0, xr2, ft2, ct))
    assert np.isfinite(out["u"]).all()
    for b in range(B):
        if b in (qn, qi):
            assert out["status"][b] == orc.STATUS_NUMERICAL, (b, out["status"][b])
            assert np.all(out["u"][b] == 0.0)
            assert out["iters"][b] in (0, orc.default_params(10).check_every), out["iters"][b]
        else:
            assert out["status"][b] == clean["status"][b] and out["iters"][b] == clean["iters"][b]
            assert out["u"][b].tobytes() == clean["u"][b].tobytes(), b
