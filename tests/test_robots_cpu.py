"""CPU-side tests of the per-QP robot records (include/srbdqp.h srbdqp_robot, srbdqp_set_robots): the record's layout on both sides of
the C-ABI, the exported setters, robots_array(), and the resources of the MODE = 2 instantiations of the general kernel that read the
records (no scratch, occupancy no lower than the MODE = 0 twin)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIELDS = ("mass", "inertia", "mu", "fz_min", "fz_max", "reserved")


def test_robot_struct_matches_the_header(tmp_path, built_lib):
    from g1_locomotion_amd import _lib
    assert C.sizeof(_lib.Robot) == 64 and _lib.ROBOT_DOUBLES * 8 == 64
    src = tmp_path / "robot.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srbdqp.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(srbdqp_robot));\n'
                   + "".join(f'    printf(" %zu", offsetof(srbdqp_robot, {f}));\n' for f in FIELDS) + "    return 0;\n}\n")
    exe = tmp_path / "robot"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.Robot)
    assert got[1:] == [getattr(_lib.Robot, f).offset for f in FIELDS]
    assert [getattr(_lib.Robot, f).offset // 8 for f in FIELDS] == [0, 1, 4, 5, 6, 7]   # the columns of robots_array()


def test_the_setters_are_exported(built_lib):
    from g1_locomotion_amd import _lib
    lib_path = _lib.LIB_PATH
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    for name in ("srbdqp_set_robots", "srbdqp_set_robots_device", "srbdqp_ragged_set_robots", "srbdqp_ragged_set_robots_device"):
        assert f" T {name}\n" in syms, name
        assert name in _lib.EXPORTS
        assert getattr(built_lib, name).restype is C.c_int
    # a null handle is refused, not dereferenced
    rec = (_lib.Robot * 1)()
    assert built_lib.srbdqp_set_robots(None, C.cast(rec, C.c_void_p), 1) == _lib.E_INVALID
    assert built_lib.srbdqp_ragged_set_robots_device(None, None, 0) == _lib.E_INVALID


def test_robots_array_broadcasts_and_fills_the_config(built_lib):
    from g1_locomotion_amd import _lib
    from g1_locomotion_amd.mpc import robots_array
    cfg = _lib.default_config()
    a = robots_array(3)
    assert a.shape == (3, 8) and a.dtype == np.float64
    assert np.all(a[:, 0] == cfg.mass) and np.all(a[:, 1:4] == np.array(list(cfg.inertia))) and np.all(a[:, 4] == cfg.mu)
    assert np.all(a[:, 5] == cfg.fz_min) and np.all(a[:, 6] == cfg.fz_max) and np.all(a[:, 7] == 0.0)
    m = np.array([30.0, 35.0, 40.0])
    a = robots_array(3, mass=m, mu=0.4, inertia=[0.1, 0.2, 0.03], fz_max=np.array([500.0, 600.0, 700.0]))
    assert np.array_equal(a[:, 0], m) and np.all(a[:, 4] == 0.4) and np.all(a[:, 1:4] == [0.1, 0.2, 0.03])
    assert np.array_equal(a[:, 6], [500.0, 600.0, 700.0]) and np.all(a[:, 5] == cfg.fz_min)
    inert = np.arange(1.0, 7.0).reshape(2, 3)
    assert np.array_equal(robots_array(2, inertia=inert)[:, 1:4], inert)
    assert np.all(robots_array(2, inertia=0.5)[:, 1:4] == 0.5)
    # another config's robot
    cfg.mass = 12.5
    cfg.fz_min = 3.0
    a = robots_array(2, cfg=cfg)
    assert np.all(a[:, 0] == 12.5) and np.all(a[:, 5] == 3.0)
    assert robots_array(0).shape == (0, 8)
    for bad in (dict(mass=np.ones(2)), dict(inertia=np.ones((3, 2))), dict(mu=np.ones((3, 1))), dict(inertia=np.ones(4))):
        with pytest.raises(ValueError):
            robots_array(3, **bad)
    # a record array is what Robot describes, row by row
    a = robots_array(2, mass=[20.0, 21.0], mu=[0.3, 0.9])
    recs = (_lib.Robot * 2).from_buffer_copy(a.tobytes())
    assert recs[1].mass == 21.0 and recs[1].mu == 0.9 and list(recs[0].inertia) == list(cfg.inertia) and recs[0].reserved == 0.0


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


@pytest.mark.parametrize("N", (4, 8, 10, 12, 16, 20))
def test_record_kernels_keep_nothing_in_scratch_and_their_occupancy(rows, N):
    """One MODE = 2 instantiation per horizon the setters accept, with 0 bytes of scratch and the occupancy of its MODE = 0 twin (the batch kernel of
    the same N and waves per SIMD)."""
    by = {r["name"].strip(): r for r in rows}
    rb = [r for name, r in by.items() if name.startswith(f"srbdqp_wrench_kernel<{N}, double, double, 2, ")]
    assert len(rb) == 1, [r["name"] for r in rb]
    rb = rb[0]
    wps = int(re.match(rf"srbdqp_wrench_kernel<{N}, double, double, 2, (\d+), double, 5, 0", rb["name"].strip()).group(1))
    twin = by[f"srbdqp_wrench_kernel<{N}, double, double, 0, {wps}, double, 5, 0>"]
    assert rb["scratch"] == 0, (rb["name"], rb["scratch"])
    assert rb["occupancy"] >= twin["occupancy"], (rb["name"], rb["occupancy"], twin["occupancy"])


def test_no_record_kernel_at_n24(rows):
    """N = 24 has no MODE = 2 instantiation (every configuration tried keeps bytes in scratch): the setters refuse it instead."""
    assert not [r for r in rows if r["name"].strip().startswith("srbdqp_wrench_kernel<24, double, double, 2, ")]
