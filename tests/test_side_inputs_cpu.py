"""CPU-side test of what the suites of the per-QP side inputs share (tests/side_inputs.py): the one twin against the oracle."""
import numpy as np
import pytest

import side_inputs as si
import srbd_oracle as orc

NEUTRAL = dict(none=lambda N: {}, flat_normals=lambda N: dict(normals=si.flat_normals(1, N)[0]), zero_wrench=lambda N: dict(ext_wrench=np.zeros((N, 6))),
               both=lambda N: dict(normals=si.flat_normals(1, N)[0], ext_wrench=np.zeros((N, 6))))
NEUTRAL_CASES = [(4, "double"), (10, "mixed"), (20, "single")]


def check_neutral_twin(neutral, N, schedule):
    """Without normals and wrench, with every normal (0, 0, 1) (T is the identity), under a zero wrench (D = 0), or both: orc.update bit for bit, so the bars
    of si.check_qp against the twin are, for a handle without those inputs, the bars against the oracle."""
    B = 3
    x0, xr, ft, ct = si.batch(B, N, 4200 + N, schedule)
    p = si.params(N)
    for b in range(B):
        ref = orc.update(p, x0[b], xr[b], ft[b], ct[b])
        tw = si.twin(p, x0[b], xr[b], ft[b], ct[b], **NEUTRAL[neutral](N))
        assert tw["status"] == ref["status"] and tw["iters"] == ref["iters"]
        assert np.array_equal(tw["u"], ref["u"]) and np.array_equal(tw["x"], ref["x"]) and np.array_equal(tw["y"], ref["y"])
        assert tw["u_hat"] is tw["u_loc"] and (tw["T"] is None) == ("normals" not in NEUTRAL[neutral](N))


@pytest.mark.parametrize("N,schedule", NEUTRAL_CASES)
@pytest.mark.parametrize("neutral", [k for k in NEUTRAL if k != "flat_normals"])
def test_the_twin_with_neutral_inputs_is_the_oracle_update(neutral, N, schedule):
    """(Flat normals alone: tests/test_contact_normals_cpu.py::test_the_twin_with_flat_normals_is_the_oracle_update, the same body.)"""
    check_neutral_twin(neutral, N, schedule)
