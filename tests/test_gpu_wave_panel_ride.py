"""The one-wave kernels with the first panel tile of every block row riding the diagonal tile's inversion (csrc/srbdqp_mfma.hpp, diag16_invert_dpp_packed<16, true>:
U_{j,j+1} = L_jj^-1 K_{j,j+1} by forward substitution in the DPP row that held an unread copy of R; csrc/srbdqp_setup1.hpp, F; tests/test_wave_panel_ride_cpu.py
restates the elimination and holds K^-1 to the high-precision inverse).  Here the kernels themselves, 64 QPs a case against the oracle -- the batches of
tests/test_gpu_wave_padded_block.py, every tile count the routine meets:

  n4                 N = 4, MAXS = 2: NT = 2, PAD = 8 -- ONE riding tile, in front of a last tile of eight pivots; the instantiation whose LDS the panel area may grow
  n4_four_contacts   N = 4, MAXS = 4: NT = 3, PAD = 0 -- riding tiles (0, 1) and (1, 2), one panel product left: (0, 2)
  n8                 N = 8, MAXS = 2: NT = 3
  n10                N = 10, MAXS = 2: NT = 4, PAD = 4; QPs 4 .. 63 in full single support (n_eff = 60), QPs 0 .. 3 with n_eff < 60
  n10_swing          a swing step on every QP: n_eff = 54
  n10_flight         the n10 batch with QP 5 in flight over the whole horizon (the pass ends before F) and QP 6 in flight over its first half

each through the restart in place, the deferred tails with a flush and the split set-up (FUSED = false): statuses and iteration counts equal to the oracle's and
to each other, max |u - oracle| <= 2e-3 N, the suite's bound.  Then every case again with rho_restart_iter = 20, so that nearly every QP runs continued passes:
the riding F at a re-balanced rho, RP = 2 in place and RP = 3 in a workgroup of the flush.  Then the n10 batch with a NaN in x_ref of one QP and an infinite
stance-foot position in another: those two end SRBDQP_NUMERICAL with forces exactly 0 (include/srbdqp.h), the other 62 keep the clean solve's bytes."""
import numpy as np
import pytest

import srbd_oracle as orc
import test_gpu_wave_front_end as fe
import test_gpu_wave_kinv_recurrence as kr
import test_gpu_wave_padded_block as pb
import test_gpu_wave_setup_diet as sd
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TOL_TWIN_N = 2e-3
B = kr.B
SHAPES = dict(pb.SHAPES)                                       # KS, NT, PAD
PATHS = ("restart", "defer", "split")


def test_the_cases_hold_the_tile_counts():
    assert {nt for _, nt, _ in SHAPES.values()} == {2, 3, 4}
    for case, (ks, nt, pad) in SHAPES.items():
        N, maxs, inputs, p, ref = kr._reference(case, False)
        assert 3 * maxs * N == ks and (ks + 15) // 16 == nt
    N, maxs, (x0, xr, ft, ct), p, ref = kr._reference("n10_swing", False)
    assert (3 * ct.reshape(B, -1).sum(1)[4:] == 54).all()


_FLIGHT_EARLY = {}


def _flight(early):
    """the flight batch of tests/test_gpu_wave_padded_block.py; early: with the oracle's solution at rho_restart_iter = 20, computed once"""
    if not early:
        return pb._flight_batch()
    if not _FLIGHT_EARLY:
        import c_oracle
        inputs, _ = pb._flight_batch()
        ref = c_oracle.solve_batch(orc.params_for(10, **kr.EARLY), *inputs, nthreads=8)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FLIGHT_EARLY["v"] = (inputs, ref)
    return _FLIGHT_EARLY["v"]


def _run_flight(torch, early, kernel, flags):
    from g1_locomotion_amd import BatchMPC, _lib
    inputs, _ = _flight(early)
    if not early:
        return fe._run(torch, 10, 2, kernel, flags, inputs)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.array(v)).to(dev) for v in inputs]
    u = torch.zeros((B, 10, 12), dtype=torch.float64, device=dev)
    st = torch.full((B,), -77, dtype=torch.int32, device=dev)
    it = torch.zeros(B, dtype=torch.int32, device=dev)
    with BatchMPC(horizon=10, max_contacts_per_step=2, kernel=kernel, flags=flags, **kr.EARLY) as eng:
        eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), status=st.data_ptr(), iters=it.data_ptr())
        if flags & _lib.FLAG_DEFER_TAIL:
            eng.flush()
        eng.synchronize()
        torch.cuda.synchronize(dev)
        name = eng.kernel_name()
    return dict(u=u.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy()), name


@pytest.mark.parametrize("early", [False, True], ids=["default_restart", "restart_after_20"])
@pytest.mark.parametrize("case", list(SHAPES) + ["n10_flight"])
def test_restart_defer_and_split_against_the_oracle_and_each_other(torch_first, built_lib, case, early):
    if case == "n10_flight":
        (x0, xr, ft, ct), ref = _flight(early)
        N = 10
        assert ct[5].sum() == 0 and 3 * ct[6].sum() == 30
        run = lambda kernel, flags: _run_flight(torch_first, early, kernel, flags)      # noqa: E731
    else:
        N, maxs, (x0, xr, ft, ct), p, ref = kr._reference(case, early)
        run = lambda kernel, flags: kr._run(torch_first, case, early, kernel, flags)     # noqa: E731
    if early:
        past = int((ref["iters"] > kr.EARLY["rho_restart_iter"]).sum())
        print(case, "QPs that run continued passes", past, "of", B)
        assert past > B // 2
    sd._three_paths(torch_first, run, ref, ct, N, case + (" restart after 20" if early else ""))


@pytest.mark.parametrize("path", ["restart", "defer"])
def test_a_nan_in_x_ref_and_an_infinite_foot(torch_first, built_lib, path):
    from g1_locomotion_amd import _lib
    x0, xr, ft, ct = fe._batch("n10")
    flags = _lib.FLAG_DEFER_TAIL if path == "defer" else 0
    clean, name = fe._run(torch_first, 10, 2, _lib.KERNEL_WAVE, flags, (x0, xr, ft, ct))
    assert name.startswith(sd.PATHS[path]), name
    xr2, ft2 = xr.copy(), np.array(ft, copy=True)
    qn, qi = 11, 13
    xr2[qn, 3, 4] = np.nan                                    # a position of the fourth step's reference
    k = 2
    c = int(np.flatnonzero(ct[qi, k])[0])                     # a stance contact of step 2: the entries of K it reaches lie in the first block rows, riding tiles included
    ft2.reshape(B, 10, 4, 3)[qi, k, c, 0] = np.inf
    out, _ = fe._run(torch_first, 10, 2, _lib.KERNEL_WAVE, flags, (x0, xr2, ft2, ct))
    assert np.isfinite(out["u"]).all()
    kept = 0
    for b in range(B):
        if b in (qn, qi):
            assert out["status"][b] == orc.STATUS_NUMERICAL, (b, out["status"][b])
            assert np.all(out["u"][b] == 0.0)
        else:
            assert out["status"][b] == clean["status"][b] and out["iters"][b] == clean["iters"][b]
            assert out["u"][b].tobytes() == clean["u"][b].tobytes(), b
            kept += 1
    assert kept == B - 2
