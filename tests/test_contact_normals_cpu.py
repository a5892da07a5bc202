"""CPU-side tests of contact normals (include/srbdqp.h srbdqp_set_contact_normals): the host mirror of the frame convention (contact_frames), the oracle twin
the GPU tests compare against (tests/side_inputs.py; with flat normals it is the oracle: tests/test_side_inputs_cpu.py), and the library's exports.

No refusal of the two setters can be reached without a device -- every one of them needs a handle, and srbdqp_create returns SRBDQP_E_NO_DEVICE here (as the
other CPU C-ABI tests find) -- except the null handle; tests/test_gpu_contact_normals.py covers them all."""
import numpy as np
import pytest

import side_inputs as si
import srbd_oracle as orc
from g1_locomotion_amd import contact_frames
from test_side_inputs_cpu import NEUTRAL_CASES, check_neutral_twin


def test_contact_frames_follow_the_convention():
    assert np.array_equal(contact_frames([0.0, 0.0, 1.0]), np.eye(3))
    assert np.array_equal(contact_frames(np.tile([0.0, 0.0, 1.0], (3, 5, 1))), np.broadcast_to(np.eye(3), (3, 5, 3, 3)))
    rng = np.random.default_rng(3)
    tilt, az = rng.uniform(0.0, np.pi / 3, 500), rng.uniform(-np.pi, np.pi, 500)            # slopes to 60 degrees
    n = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], -1) * rng.uniform(0.5, 2.0, (500, 1))
    R = contact_frames(n)
    assert R.shape == (500, 3, 3)
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() <= 1e-14
    assert np.abs(np.linalg.det(R) - 1.0).max() <= 1e-14
    assert np.abs(R[:, :, 2] - n / np.linalg.norm(n, axis=1, keepdims=True)).max() <= 1e-15
    assert np.all(R[:, 0, 0] > 0.0) and np.abs((R[:, :, 0] * R[:, :, 2]).sum(-1)).max() <= 1e-14      # t1: e_x projected onto the surface
    assert np.abs(np.cross(R[:, :, 2], R[:, :, 0]) - R[:, :, 1]).max() <= 1e-15              # t2 = n x t1
    with pytest.raises(ValueError):
        contact_frames(np.zeros((4, 2)))


@pytest.mark.parametrize("N,schedule", NEUTRAL_CASES)
def test_the_twin_with_flat_normals_is_the_oracle_update(N, schedule):
    check_neutral_twin("flat_normals", N, schedule)


def test_the_twin_on_a_ridge_respects_the_tilted_pyramid():
    """Double support either side of a 0.6 rad ridge, N = 10: the twin's forces lie inside the tilted pyramids (1e-4, scaled) and agree with the exact optimum of
    the local QP (5e-2 N); a friction row of the tilted pyramid is active, and the flat-ground optimum of the same inputs leaves that pyramid by more than 0.5 N."""
    B, N = 4, 10
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=5100 + N, schedule="double")
    p = si.params(N)
    nr = si.ridge_normals(B, N)
    for b in range(B):
        tw = si.twin(p, x0[b], xr[b], ft[b], ct[b], normals=nr[b])
        assert tw["status"] == orc.STATUS_SOLVED
        assert si.cone_violation(p, tw["qp"], tw["T"], tw["u"]) <= 1e-4
        xs, _ = orc.solve_reference(p, tw["qp_loc"])
        assert np.abs(tw["u_loc"] - xs).max() * p.force_scale <= 5e-2
        assert si.friction_row_active(p, tw["T"], tw["u"], ct[b])
        flat = orc.update(p, x0[b], xr[b], ft[b], ct[b])
        assert si.cone_violation(p, tw["qp"], tw["T"], flat["u"]) * p.force_scale > 0.5, b


def test_library_exports_and_binds_both_setters(built_lib):
    from g1_locomotion_amd import _lib
    for name in ("srbdqp_set_contact_normals", "srbdqp_set_contact_normals_device"):
        assert name in _lib.EXPORTS
        fn = getattr(built_lib, name)
        assert fn.restype is not None and len(fn.argtypes) == 3
        assert fn(None, None, 0) == _lib.E_INVALID                                           # (no handle: the one refusal that needs no device)
