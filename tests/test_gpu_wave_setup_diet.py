"""The one-wave kernels' set-up with less non-arithmetic vector work (csrc/srbdqp_setup1.hpp, csrc/srbdqp_mfma.hpp): the prefix sums C_k as a chain over
neighbouring lanes (row_prev), the identity of the packed inversion read from an LDS tile beside S, the W tile with its rows at PkTile::wrow and every access
one lane base plus immediate offsets, and the lane-constant residues of the loads, of J and of the K assembly formed once.  None of it changes the arithmetic
(tests/test_wave_prefix_chain_cpu.py holds the chain to the serial loop bit for bit), so the kernels must do here what they did: on the batches of
tests/test_gpu_wave_kinv_recurrence.py (64 QPs, every tile count, both sides of n_eff < KS)

  n4 (NT = 2)   n4_four_contacts (MAXS = 4, NT = 3)   n8 (NT = 3)   n10 (NT = 4, n_eff = 60)   n10_swing (NT = 4, n_eff = 54)

through the restart in place, the deferred tails with a flush and the split pipeline's set-up (FUSED = false) -- statuses and iteration counts equal to the
oracle's AND to each other on every QP, forces within the twin bound 2e-3 N --, then the two-phase call and a caller's warm start, and three more N = 10
batches that aim at the chain: a first yaw of -0.0 (the chain's leading 0 + c_0), all yaws of a QP equal (every lane adds the same term; the synthetic
batches above are of this kind) and a turning reference with another yaw on every step (a lane that took the wrong neighbour's sum shows only here)."""
import numpy as np
import pytest

import srbd_oracle as orc
import test_gpu_wave_front_end as fe
import test_gpu_wave_kinv_recurrence as kr
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TOL_TWIN_N = kr.TOL_TWIN_N          # 2e-3 N
B = kr.B
PATHS = {"restart": "wave_f64", "defer": "wave_defer_f64", "split": "split_f64"}


def _three_paths(torch, run, ref, ct, N, what):
    """run(kernel, flags) -> (out, name) for the three pipelines; each against the oracle, then against each other"""
    from g1_locomotion_amd import _lib
    outs = {}
    for path, prefix in PATHS.items():
        out, name = run(_lib.KERNEL_SPLIT if path == "split" else _lib.KERNEL_WAVE, _lib.FLAG_DEFER_TAIL if path == "defer" else 0)
        assert name.startswith(prefix), name
        err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
        print(what, path, name, " QPs past the first restart mark", int((ref["iters"] > 55).sum()), " max |u - oracle|", err.max(), "N")
        np.testing.assert_array_equal(out["status"], ref["status"])
        np.testing.assert_array_equal(out["iters"], ref["iters"])
        assert err.max() <= TOL_TWIN_N, (path, err.max())
        assert np.all(out["u"].reshape(B, N, 4, 3)[ct == 0] == 0.0)
        outs[path] = out
    for path in ("defer", "split"):
        np.testing.assert_array_equal(outs[path]["status"], outs["restart"]["status"])
        np.testing.assert_array_equal(outs[path]["iters"], outs["restart"]["iters"])


@pytest.mark.parametrize("case", list(kr.CASES))
def test_restart_defer_and_split_against_the_oracle_and_each_other(torch_first, built_lib, case):
    N, maxs, (x0, xr, ft, ct), p, ref = kr._reference(case, False)
    _three_paths(torch_first, lambda kernel, flags: kr._run(torch_first, case, False, kernel, flags), ref, ct, N, case)


@pytest.mark.parametrize("case", list(kr.CASES))
def test_the_two_phase_call_and_a_callers_warm_start(torch_first, built_lib, case):
    """(the checks of tests/test_gpu_wave_kinv_recurrence.py on these two paths: eight QPs each against the oracle, statuses and iteration counts equal)"""
    kr.test_the_two_phase_call(torch_first, built_lib, case)
    kr.test_a_callers_warm_start(torch_first, built_lib, case)


_YAW = {}


def _yaw_batch(kind):
    """The n10 batch with the yaws of x_ref (entry 2 of a step) set; the oracle's solution once, shared read-only."""
    if kind not in _YAW:
        import c_oracle
        x0, xr, ft, ct = fe._batch("n10")
        xr = xr.copy()
        if kind == "first_yaw_minus_zero":
            xr[:, 0, 2] = -0.0
        elif kind == "turning_yaws":                      # a yaw of its own on every step: a lane that picked up a neighbour's term too early or too late shows
            xr[:, :, 2] = xr[:, :1, 2] + np.cumsum(np.random.default_rng(2330).normal(0.0, 0.15, xr.shape[:2]), axis=1)
        else:
            xr[:, :, 2] = xr[:, :1, 2]                    # every step the QP's first yaw (what the synthetic batches hold: said here, not assumed)
        p = orc.default_params(10)
        ref = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=8)
        for v in [x0, xr, ft, ct] + list(ref.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _YAW[kind] = ((x0, xr, ft, ct), ref)
    return _YAW[kind]


@pytest.mark.parametrize("kind", ["first_yaw_minus_zero", "all_yaws_equal", "turning_yaws"])
def test_the_yaws_the_prefix_chain_could_get_wrong(torch_first, built_lib, kind):
    inputs, ref = _yaw_batch(kind)
    xr, ct = inputs[1], inputs[3]
    if kind == "first_yaw_minus_zero":
        assert np.all(np.signbit(xr[:, 0, 2])) and np.all(xr[:, 0, 2] == 0.0)
    elif kind == "turning_yaws":
        assert np.all(np.abs(np.diff(xr[:, :, 2], axis=1)) > 0.0)
    else:
        assert np.all(xr[:, :, 2] == xr[:, :1, 2]) and np.ptp(xr[:, 0, 2]) > 0.0
    _three_paths(torch_first, lambda kernel, flags: fe._run(torch_first, 10, 2, kernel, flags, inputs), ref, ct, 10, kind)
