"""CPU side of the fleet roll-out (include/srbdqp_cascade.h srbdqp_fleet_*): the library exports the calls and the binding lists them,
refusals that need no device, and the NumPy twin the GPU tests compare against (tests/fleet_twin.py) -- held against the one closed loop the tree had
(tests/test_msgs_closed_loop.py) and against itself on the two CPU oracles."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import srbd_oracle as orc
import fleet_twin as ft

CALLS = ("srbdqp_fleet_default_settings", "srbdqp_fleet_advance_f64", "srbdqp_fleet_advance_device_f64", "srbdqp_fleet_rollout_device_f64",
         "srbdqp_fleet_rollout_f64")
T = 50


def test_the_library_exports_the_fleet_calls_and_the_binding_lists_them(built_lib):
    from g1_locomotion_amd import _lib, BatchMPC
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in CALLS:
        assert f" T {name}\n" in syms, name
        assert name in _lib.SIGNATURES and getattr(built_lib, name).restype is C.c_int
    for method in ("fleet_advance", "fleet_advance_device", "rollout", "rollout_device", "fleet_settings"):
        assert callable(getattr(BatchMPC, method))


def test_settings_struct_defaults_and_refusals_without_a_device(built_lib):
    from g1_locomotion_amd import _lib
    s = _lib.FleetSettings()
    assert C.sizeof(_lib.FleetSettings) == 32 + C.sizeof(_lib.Gait)
    s.struct_size = C.sizeof(_lib.FleetSettings)
    assert built_lib.srbdqp_fleet_default_settings(C.byref(s)) == _lib.OK
    assert (s.substeps, s.foot_half_length, s.z_min, s.tilt_max) == (10, 0.085, 0.3, 1.0)
    assert s.gait.struct_size == C.sizeof(_lib.Gait) and (s.gait.period_steps, s.gait.double_support_steps, s.gait.hip_offset_y) == (6, 1, 0.0645)
    # a struct of another size is refused before anything is written into it
    buf = (C.c_char * (C.sizeof(_lib.FleetSettings) + 32))()
    C.memset(buf, 0x5A, len(buf))
    p = C.cast(buf, C.POINTER(_lib.FleetSettings))
    for claimed in (0, C.sizeof(_lib.FleetSettings) - 8, C.sizeof(_lib.FleetSettings) + 8):
        p.contents.struct_size = claimed
        assert built_lib.srbdqp_fleet_default_settings(p) == _lib.E_INVALID
        assert bytes(buf)[4:] == b"\x5a" * (len(buf) - 4)
    assert built_lib.srbdqp_fleet_default_settings(None) == _lib.E_INVALID
    # a null handle is refused, not dereferenced
    assert built_lib.srbdqp_fleet_advance_f64(None, 1, None, None, None, None, 12, None, None, None, None, C.byref(s)) == _lib.E_INVALID
    assert built_lib.srbdqp_fleet_advance_device_f64(None, 1, None, None, None, None, 12, None, None, None, None, C.byref(s), None) == _lib.E_INVALID
    assert built_lib.srbdqp_fleet_rollout_f64(None, 1, 1, *([None] * 6), C.byref(s), *([None] * 6)) == _lib.E_INVALID
    assert built_lib.srbdqp_fleet_rollout_device_f64(None, 1, 1, *([None] * 6), C.byref(s), *([None] * 7)) == _lib.E_INVALID


def test_twin_reproduces_the_single_robot_closed_loop_bit_for_bit():
    """B = 1, standing, no push, the NumPy oracle behind it: the twin is the loop of tests/test_msgs_closed_loop.py.  That loop hands the MPC its state through
    the message types, where gravity is a float32 (msgs.state_to_vec) while the plant keeps the double: mpc_view is that round trip."""
    import test_msgs_closed_loop as cl
    from g1_locomotion_amd import msgs
    from srbd_plant import OracleMPC
    ref = cl._run(OracleMPC(), 30, standing=True)
    x = np.zeros((1, 13)); x[0, 3:6] = cl.COM + np.array([0.01, -0.01, -0.01]); x[0, 0] = 0.03; x[0, 12] = -9.80665
    view = lambda xs: np.stack([msgs.state_to_vec(msgs.vec_to_state(v)) for v in xs])
    r = ft.rollout(orc.SrbdParams(dt=0.04), x, cl.FEET.reshape(1, 12), np.zeros(1), np.zeros((1, 2)), 30, cl.COM, standing=np.ones(1), solver="numpy",
                   mpc_view=view)
    assert np.array_equal(r["x"][1:, 0], ref)
    assert np.array_equal(r["feet"][-1, 0], cl.FEET.reshape(12)) and r["alive"][0] == 1 and abs(r["stamp"][0] - 1.2) < 1e-12


@pytest.fixture(scope="module")
def fleet_c():
    f = ft.fleet()
    return ft.rollout(orc.default_params(10), f["x"], f["feet"], f["stamp"], f["v_ref"], T, ft.COM, standing=f["standing"], push=ft.fleet_push(T, 6), solver="c")


def test_twin_keeps_the_fleet_up_and_every_solve_solved(fleet_c):
    r = fleet_c
    assert r["alive"].tolist() == [1] * 6 and np.all(r["status"] == 1)
    assert r["x"][:, :, 5].min() > 0.55 and np.abs(r["x"][:, :, 0:2]).max() < 0.1
    assert np.all(r["x"][-1, 2:4, 3] - r["x"][0, 2:4, 3] > 0.2) and r["x"][-1, 4, 4] - r["x"][0, 4, 4] > 0.1    # the walkers walk where they are told
    assert np.abs(r["stamp"] - (0.04 * np.arange(6) + 0.04 * T)).max() < 1e-9


def test_c_and_numpy_oracle_rollouts_agree(fleet_c):
    f = ft.fleet()
    rn = ft.rollout(orc.default_params(10), f["x"], f["feet"], f["stamp"], f["v_ref"], T, ft.COM, standing=f["standing"], push=ft.fleet_push(T, 6), solver="numpy")
    assert np.array_equal(fleet_c["iters"], rn["iters"]) and np.array_equal(fleet_c["status"], rn["status"])
    worst = max(np.abs(fleet_c[k] - rn[k]).max() for k in ("x", "feet"))
    print("C against NumPy oracle over", T, "steps:", worst)
    assert worst < 1e-8, worst


def test_both_feet_of_a_walking_robot_have_moved_by_step_13(fleet_c):
    """The gait period is 12 steps: one touchdown of each foot lies in any 13.  The standing robot's feet never move."""
    feet = fleet_c["feet"].reshape(T + 1, 6, 4, 3)
    moved = np.abs(feet[13] - feet[0]).max(axis=2) > 1e-4                 # (robot, contact)
    assert not moved[0].any() and moved[1:].all(), moved
    # heel and toe of a foot that landed: foot_half_length either side of one point, on the ground
    assert np.abs((feet[13, 1:, 1::2, 0] - feet[13, 1:, 0::2, 0]) - 0.17).max() < 1e-12 and np.all(feet[13, :, :, 2] == 0.0)
    assert np.array_equal(feet[13, 1:, 0::2, 1], feet[13, 1:, 1::2, 1])
