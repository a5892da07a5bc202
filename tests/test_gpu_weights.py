"""GPU tests of what is particular to the per-QP cost weights (include/srbdqp.h srbdqp_weights, srbdqp_set_weights / _device, srbdqp_ragged_set_weights /
_device; the general kernel's MODE = 6 instantiation, srbdqp_wrench_wt_kernel): their own refusals.  What the weights share with the other per-QP side inputs
-- parity per QP, the neutral records, the combination with robot records, the schedule hint, the ragged order, bad device records, the shared bound -- is in
tests/test_gpu_side_inputs.py; the bars, the draw and the seeds are described in tests/side_inputs.py."""
import numpy as np
import pytest

import side_inputs as si
import srbd_oracle as orc
from gpu_helpers import refusal as _refusal, torch_first  # noqa: F401  (torch_first: the fixture)
from test_gpu_side_inputs import NEUTRAL_CASES, check_neutral, check_parity

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("schedule", si.SCHEDULES)
@pytest.mark.parametrize("N", si.HORIZONS)
def test_per_qp_weights_match_the_oracle(torch_first, built_lib, N, schedule):
    check_parity(si.WEIGHTS, N, schedule)


@pytest.mark.parametrize("N,schedule", NEUTRAL_CASES)
def test_uniform_weights_equal_the_config(torch_first, built_lib, N, schedule):
    """Every record = the handle's config: the same QPs as a KERNEL_WRENCH solve without weights, bit for bit."""
    check_neutral(si.WEIGHTS, N, schedule)


def test_ragged_objects_that_refuse_weights(torch_first, built_lib):
    from g1_locomotion_amd import RaggedMPC, SrbdqpError
    from g1_locomotion_amd.mpc import weights_array
    rec = weights_array(4)
    for horizons, text in (((8, 24), "bucket N=24: per-QP cost weights: not at N = 24"), ((3, 4), "SRBDQP_FLAG_ANY_HORIZON")):
        rg = RaggedMPC(horizons=horizons)
        try:
            for arg in (rec, torch_first.from_numpy(rec).cuda()):
                with pytest.raises(SrbdqpError, match=text):
                    rg.set_weights(arg)
            rg.set_weights(None)
        finally:
            rg.close()


def test_ragged_solves_that_weights_refuse(torch_first, built_lib):
    """While weights are set on a ragged object: the fp32 solves and a solve of B > length QPs return SRBDQP_E_INVALID with a message (nothing is launched);
    a solve of B <= length and, after clearing, the fp32 solve are accepted."""
    from g1_locomotion_amd import RaggedMPC, _lib
    Nq, x0, xr, ft, ct, rec, off, refs, _ = si.ragged_case(si.WEIGHTS)
    B, E = 6, f"srbdqp error {_lib.E_INVALID}: "
    rows = int(off[B])
    q = (Nq[:B], x0[:B], xr[:rows], ft[:rows], ct[:rows])
    rg = RaggedMPC(horizons=si.RAGGED_HORIZONS)
    try:
        rg.set_weights(rec[:B])
        f32 = E + "fp32 ragged solve: refused while per-QP cost weights are set (srbdqp_ragged_set_weights): only the fp64 solves read them"
        assert _refusal(lambda: rg.solve_packed(*q, dtype=np.float32)) == f32
        rg.set_weights(rec[:B - 1])
        assert _refusal(lambda: rg.solve_packed(*q)) == E + f"ragged solve of {B} QPs with {B - 1} weight records set: every QP needs its record"
        assert _refusal(lambda: rg.solve_packed(*q, dtype=np.float32)) == f32
        short = rg.solve_packed(Nq[:B - 1], x0[:B - 1], xr[:off[B - 1]], ft[:off[B - 1]], ct[:off[B - 1]])       # B <= length
        assert np.array_equal(short["status"], [refs[b]["status"] for b in range(B - 1)])
        rg.set_weights(None)
        assert _refusal(lambda: rg.solve_packed(*q, dtype=np.float32)) is None
    finally:
        rg.close()


def test_what_the_refusal_table_does_not_say_about_weights(torch_first, built_lib):
    """The weights column and rows of the table are in tests/test_gpu_variant_refusals.py; here, with its calls (B = 2, N = 4, full double support), what a
    table of (call, variant) cannot express."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    from g1_locomotion_amd.mpc import weights_array
    from test_gpu_variant_refusals import TAIL as VT, _calls
    B, N = 2, 4
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=610 + N, schedule="double")
    wr = weights_array(B, r_diag=[1e-4, 3e-4])
    wr_dev = torch.from_numpy(wr).cuda()
    E = f"srbdqp error {_lib.E_INVALID}: "
    with BatchMPC(horizon=N) as eng:
        calls = _calls(torch, eng, N)
        eng.set_weights(wr)
        assert _refusal(calls["srbdqp_solve_batch_f64"]) is None and eng.kernel_name() == "wrench_f64_n4_wt"
        # B > length
        eng.set_weights(wr[:1])
        msg = _refusal(calls["srbdqp_solve_batch_f64"])
        assert msg == E + "solve of 2 QPs with 1 weight records set (srbdqp_set_weights): every QP needs its record", msg
        assert _refusal(calls["srbdqp_solve_batch_device_f64"]) == msg
        # the clearing calls, host and device form: a plain handle again
        eng.set_weights(wr_dev)
        eng.set_weights(None)
        eng.set_weights(wr)
        eng.set_weights(torch.empty((0, 16), dtype=torch.float64, device="cuda"))
        for name in ("srbdqp_solve_staged_f64", "srbdqp_solve_batch_f32", "srbdqp_assemble_wrench_f64", "srbdqp_set_contact_normals"):
            assert _refusal(calls[name]) is None, name
        # with normals set (the line above), the weight setters are refused in the normals' words
        for fn, arg in (("srbdqp_set_weights", wr), ("srbdqp_set_weights_device", wr_dev)):
            assert _refusal(lambda: eng.set_weights(arg)) == E + f"{fn}: {VT['normals']}"
        eng.set_weights(None)                                        # (clearing is accepted in every state)
    # an explicit presolved kernel
    for kern in (_lib.KERNEL_COMPACT, _lib.KERNEL_SPLIT, _lib.KERNEL_WAVE):
        with BatchMPC(horizon=N, kernel=kern) as eng:
            eng.set_weights(wr)
            msg = _refusal(lambda: eng.solve(x0, xr, ft, ct))
            assert msg is not None and "per-QP cost weights (srbdqp_set_weights) are read by the general kernel only" in msg, msg
    # a live horizon, rank-aware steps, N = 24
    with BatchMPC(horizon=3) as eng:
        for fn, arg in (("srbdqp_set_weights", wr), ("srbdqp_set_weights_device", wr_dev)):
            assert _refusal(lambda: eng.set_weights(arg)) == E + f"{fn}: {VT['live']}"
    with BatchMPC(horizon=N, rank_aware=True) as eng:
        for fn, arg in (("srbdqp_set_weights", wr), ("srbdqp_set_weights_device", wr_dev)):
            assert _refusal(lambda: eng.set_weights(arg)) == E + f"{fn}: {VT['rank_aware']}"
    with BatchMPC(horizon=24) as eng:
        for arg in (wr, wr_dev):
            msg = _refusal(lambda: eng.set_weights(arg))
            assert msg is not None and msg.startswith(E + "per-QP cost weights: not at N = 24"), msg
        eng.set_weights(None)
