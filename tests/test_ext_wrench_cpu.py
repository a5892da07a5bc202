"""CPU-side tests of the external wrench (include/srbdqp.h srbdqp_set_external_wrench): the twin of tests/side_inputs.py against a step-by-step
simulation and against two identities that need no wrench code at all (a vertical force is more gravity; a wrench without a yaw torque is a shifted
reference), the exported setters, the resources of the MODE = 7 instantiations of the general kernel (no scratch, occupancy no lower than the MODE = 6
twin), and the conditions the seeds of the GPU suite were fixed for."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import side_inputs as si
import srbd_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SETTERS = ("srbdqp_set_external_wrench", "srbdqp_set_external_wrench_device", "srbdqp_ragged_set_external_wrench", "srbdqp_ragged_set_external_wrench_device")


@pytest.mark.parametrize("N,schedule", [(4, "double"), (10, "mixed"), (20, "three")])
def test_the_condensed_response_is_the_step_by_step_simulation(N, schedule):
    """x_{k+1} = A_k x_k + B_k u_k + e_k simulated step by step with the twin's forces gives the twin's roll-out: A_qp x0 + B_qp u + D."""
    x0, xr, ft, ct = si.batch(2, N, si.wrench_batch_seed(N, schedule), schedule)
    w = si.draw_wrench(2, N, si.wrench_seed(N))
    p = si.params(N)
    for b in range(2):
        ref = si.twin(p, x0[b], xr[b], ft[b], ct[b], ext_wrench=w[b])
        e = si.affine(p, xr[b], w[b])
        x = np.asarray(x0[b], np.float64).copy()
        for k in range(N):
            A, Bm = orc.linearise(p, float(xr[b, k, 2]), ft[b, k].reshape(4, 3) - xr[b, k, 3:6])
            x = A @ x + Bm @ ref["u"][k] + e[k]
            assert np.abs(x - ref["x"][k + 1]).max() <= 1e-10 * max(1.0, np.abs(x).max()), (b, k)
        assert np.abs(si.response(p, xr[b], w[b]) - (ref["x"][1:] - orc.rollout(ref["qp"], x0[b], ref["u_hat"], p.force_scale)[1:])).max() <= 1e-12


@pytest.mark.parametrize("N,schedule", [(10, "mixed"), (16, "double")])
def test_a_constant_vertical_force_is_more_gravity(N, schedule):
    """A constant (0, 0, 0, 0, 0, F) gives the forces of orc.update with x0[12] + F / m.  Measured: 4e-11 N, the same iteration counts."""
    B = 4
    x0, xr, ft, ct = si.batch(B, N, si.wrench_batch_seed(N, schedule), schedule)
    p = si.params(N)
    worst = 0.0
    for b in range(B):
        F = 25.0 * (b + 1) * (-1.0) ** b
        w = np.zeros((N, 6)); w[:, 5] = F
        got = si.twin(p, x0[b], xr[b], ft[b], ct[b], ext_wrench=w)
        xg = x0[b].copy(); xg[12] += F / p.mass
        ref = orc.update(p, xg, xr[b], ft[b], ct[b])
        assert got["status"] == ref["status"] and got["iters"] == ref["iters"], (b, got["iters"], ref["iters"])
        worst = max(worst, float(np.abs(got["u"] - ref["u"]).max()))
        assert np.abs(got["x"][:, :12] - ref["x"][:, :12]).max() <= 1e-9
    print(f"N={N} {schedule}: max |du| {worst:.3e} N")
    assert worst <= 1e-8, worst


@pytest.mark.parametrize("N,schedule", [(10, "mixed"), (16, "double")])
def test_a_wrench_without_yaw_torque_is_a_shifted_reference(N, schedule):
    """For any wrench with tau_z = 0 the yaw column of D is exactly 0 -- the linearisation yaw is untouched --, and the solve equals orc.update on
    x_ref - D with pcom = x_ref[:, 3:6] passed explicitly.  Measured: 1e-9 N, the same iteration counts."""
    B = 4
    x0, xr, ft, ct = si.batch(B, N, si.wrench_batch_seed(N, schedule), schedule)
    w = si.draw_wrench(B, N, si.wrench_seed(N))
    w[:, :, 2] = 0.0
    p = si.params(N)
    worst = 0.0
    for b in range(B):
        D = si.response(p, xr[b], w[b])
        assert np.all(D[:, 2] == 0.0) and np.all(D[:, 12] == 0.0)
        got = si.twin(p, x0[b], xr[b], ft[b], ct[b], ext_wrench=w[b])
        ref = orc.update(p, x0[b], xr[b] - D, ft[b], ct[b], pcom_hor=xr[b][:, 3:6])
        assert got["status"] == ref["status"] and got["iters"] == ref["iters"], (b, got["iters"], ref["iters"])
        worst = max(worst, float(np.abs(got["u"] - ref["u"]).max()))
        assert np.abs(got["x"][1:] - (ref["x"][1:] + D)).max() <= 1e-5      # (the suite's bar for x: the two ADMM runs end 1e-9 N apart, and I_w^-1 (r x .) carries that into omega)
    print(f"N={N} {schedule}: max |du| {worst:.3e} N")
    assert worst <= 1e-7, worst


def test_a_yaw_torque_moves_the_plan_and_no_reference_shift_reproduces_it():
    """tau_z alone: the yaw column of D is not 0, the forces move, and the shifted reference x_ref - D -- which now turns the linearisation yaw too --
    gives another plan."""
    N = 10
    x0, xr, ft, ct = si.batch(1, N, si.wrench_batch_seed(N, "double"), "double")
    p = si.params(N)
    w = np.zeros((N, 6)); w[:, 2] = 4.0
    D = si.response(p, xr[0], w)
    assert np.abs(D[:, 2]).max() > 1e-3
    got = si.twin(p, x0[0], xr[0], ft[0], ct[0], ext_wrench=w)
    plain = orc.update(p, x0[0], xr[0], ft[0], ct[0])
    shifted = orc.update(p, x0[0], xr[0] - D, ft[0], ct[0], pcom_hor=xr[0][:, 3:6])
    assert np.abs(got["u"] - plain["u"]).max() > 1.0
    assert np.abs(got["u"] - shifted["u"]).max() > 1e-3


def test_the_setters_are_exported(built_lib):
    from g1_locomotion_amd import _lib
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in SETTERS:
        assert f" T {name}\n" in syms, name
        assert name in _lib.EXPORTS
        assert getattr(built_lib, name).restype is C.c_int
    # a null handle is refused, not dereferenced
    w = (C.c_double * 24)()
    assert built_lib.srbdqp_set_external_wrench(None, C.cast(w, C.c_void_p), 1) == _lib.E_INVALID
    assert built_lib.srbdqp_set_external_wrench_device(None, None, 0) == _lib.E_INVALID
    assert built_lib.srbdqp_ragged_set_external_wrench(None, C.cast(w, C.c_void_p), 4) == _lib.E_INVALID
    assert built_lib.srbdqp_ragged_set_external_wrench_device(None, None, 0) == _lib.E_INVALID
    hdr = open(os.path.join(ROOT, "include", "srbdqp.h")).read()
    assert re.search(r"#define SRBDQP_EXT_WRENCH_MAX 1\.0e6\b", hdr)


@pytest.fixture(scope="module")
def rows(built_lib):
    import resource_table
    log = os.path.join(os.environ.get("TMPDIR", "/tmp"), "srbdqp_build.log")
    src = os.path.join(ROOT, "g1_locomotion_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(src, f)) for f in os.listdir(src) if f.endswith((".hip", ".hpp")))
    if not (os.path.exists(log) and os.path.getmtime(log) >= newest and "Function Name" in open(log).read()):
        # no log of the current sources: compile the device code once more for its remarks (as tests/test_build_resources.py does)
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-c", "--cuda-device-only", "-o", os.devnull,
               os.path.join(src, "srbdqp.hip"), "-Rpass-analysis=kernel-resource-usage"]
        with open(log, "w") as lf:
            subprocess.check_call(cmd, stderr=lf)
    return resource_table.parse(log)


@pytest.mark.parametrize("N", si.HORIZONS)
def test_wrench_kernels_keep_nothing_in_scratch_and_their_occupancy(rows, N):
    """One srbdqp_wrench_ew_kernel per horizon the setters accept, with 0 bytes of scratch and at least the occupancy of its MODE = 6 twin."""
    by = {r["name"].strip(): r for r in rows}
    ek = [r for name, r in by.items() if name.startswith(f"srbdqp_wrench_ew_kernel<{N}, ")]
    assert len(ek) == 1, [r["name"] for r in ek]
    ek = ek[0]
    wps = int(re.match(rf"srbdqp_wrench_ew_kernel<{N}, (\d+)>", ek["name"].strip()).group(1))
    twin = by[f"srbdqp_wrench_wt_kernel<{N}, {wps}>"]
    assert ek["scratch"] == 0, (ek["name"], ek["scratch"])
    assert ek["occupancy"] >= twin["occupancy"], (ek["name"], ek["occupancy"], twin["occupancy"])


def test_no_wrench_kernel_at_n24(rows):
    assert [r for r in rows if r["name"].strip().startswith("srbdqp_wrench_ew_kernel<")]
    assert not [r for r in rows if r["name"].strip().startswith("srbdqp_wrench_ew_kernel<24, ")]


@pytest.mark.parametrize("schedule", si.SCHEDULES)
@pytest.mark.parametrize("N", si.HORIZONS)
def test_the_seeds_keep_their_conditions(N, schedule):
    """Every case of the GPU suite's twin comparison: at least 14 of 16 SOLVED, no SOLVED QP within check_every of the cap, every QP moved by more than 1 N
    against the solve without the wrench, and at N = 10 the slowest QP past the restart mark."""
    B = si.B16
    x0, xr, ft, ct = si.batch(B, N, si.wrench_batch_seed(N, schedule), schedule)
    w = si.draw_wrench(B, N, si.wrench_seed(N))
    p = si.params(N)
    solved, moved, most = 0, 0, 0
    for b in range(B):
        ref = si.twin(p, x0[b], xr[b], ft[b], ct[b], ext_wrench=w[b])
        plain = orc.update(p, x0[b], xr[b], ft[b], ct[b])
        solved += int(ref["status"] == orc.STATUS_SOLVED)
        moved += int(np.abs(ref["u"] - plain["u"]).max() > 1.0)
        most = max(most, int(ref["iters"]))
        assert not (ref["status"] == orc.STATUS_SOLVED and ref["iters"] > p.max_iter - p.check_every), (b, ref["iters"])
    assert solved >= 14, solved
    assert moved == B, moved
    if N == 10:
        assert most > orc.default_restart(N)[0], most
