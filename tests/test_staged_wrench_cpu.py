"""CPU-side tests of the external wrench of one call on the staged path (include/srbdqp.h srbdqp_stage_ext_wrench, srbdqp_solve_staged_wrench_f64,
srbdqp_update_wrench_f64): the three declarations against the binding's table and the library's exports, the resources of the low-latency MODE = 7
instantiations of the general kernel (no scratch), the route MPC.update(external_wrench=) takes with and without staged_wrench=True -- on a stub engine, no
GPU --, and the code object the new kernels live in: their own, behind the one that holds the plain call's batch-1 kernels."""
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

CALLS = ("srbdqp_stage_ext_wrench", "srbdqp_solve_staged_wrench_f64", "srbdqp_update_wrench_f64")


def test_the_header_declares_the_three_calls_and_the_table_holds_them():
    from g1_locomotion_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srbdqp.h")).read(), flags=re.S)
    params = {name: [p.strip() for p in " ".join(args.split()).split(",")]
              for name, args in re.findall(r"^int\s+(srbdqp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)}
    for name in CALLS:
        assert name in params and name in _lib.SIGNATURES and name in _lib.EXPORTS, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(params[name]), (name, params[name])
    assert params["srbdqp_stage_ext_wrench"] == ["srbdqp_handle* h", "double** out"]
    assert [p.split()[-1] for p in params["srbdqp_solve_staged_wrench_f64"]] == ["h", "B", "use_pcom", "use_warm", "want_x", "want_y"]
    # srbdqp_update_f64's parameters with the wrench behind pcom
    plain = [p.split()[-1] for p in params["srbdqp_update_f64"]]
    assert [p.split()[-1] for p in params["srbdqp_update_wrench_f64"]] == plain[:6] + ["ext_wrench"] + plain[6:]
    # srbdqp_stage keeps its layout: the wrench array is not a field of it
    body = re.search(r"typedef struct srbdqp_stage \{(.*?)\} srbdqp_stage;", hdr, flags=re.S).group(1)
    assert "wrench" not in body and len(re.findall(r"\*\s*\w+\s*;", body)) == 12


def test_the_library_exports_them(built_lib):
    from g1_locomotion_amd import _lib
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in CALLS:
        assert f" T {name}\n" in syms, name
        assert getattr(built_lib, name).restype is C.c_int
    # a null handle is refused, not dereferenced
    out = C.c_void_p()
    assert built_lib.srbdqp_stage_ext_wrench(None, C.byref(out)) == _lib.E_INVALID
    assert built_lib.srbdqp_solve_staged_wrench_f64(None, 1, 0, 0, 1, 0) == _lib.E_INVALID
    assert built_lib.srbdqp_update_wrench_f64(None, *([None] * 11)) == _lib.E_INVALID


@pytest.fixture(scope="module")
def rows(built_lib):
    import resource_table
    log = os.path.join(os.environ.get("TMPDIR", "/tmp"), "srbdqp_build.log")
    src = os.path.join(ROOT, "g1_locomotion_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(src, f)) for f in os.listdir(src) if f.endswith((".hip", ".hpp")))
    fresh = os.path.exists(log) and os.path.getmtime(log) >= newest and "Function Name" in open(log).read()
    if not fresh or "srbdqp_wrench_ew_lat_kernel" not in open(log).read():
        # no log of the current sources: compile the device code once more for its remarks (as tests/test_build_resources.py does).  A log that another test's
        # fixture wrote that way holds srbdqp.hip's kernels alone: the second translation unit's remarks are added to it
        with open(log, "a" if fresh else "w") as lf:
            for tu in (("srbdqp_wrench_lat_ew.hip",) if fresh else ("srbdqp.hip", "srbdqp_wrench_lat_ew.hip")):
                subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-c", "--cuda-device-only",
                                       "-o", os.devnull, os.path.join(src, tu), "-Rpass-analysis=kernel-resource-usage"], stderr=lf)
    return {r["name"].strip(): r for r in resource_table.parse(log)}


@pytest.mark.parametrize("N,XW", [(4, 1), (8, 2), (10, 2)])
def test_the_low_latency_wrench_kernels_keep_nothing_in_scratch(rows, N, XW):
    """A MODE 7 low-latency kernel per horizon of the staged path's low-latency form, and its twin with the inputs in the argument segment: 0 bytes of scratch,
    and no more registers than one workgroup alone on its CU has (512 per lane at one wave per SIMD)."""
    for name in (f"srbdqp_wrench_ew_lat_kernel<{N}, {XW}>", f"srbdqp_wrench_ew_lat_kernel_in<{N}, {XW}>"):
        assert name in rows, sorted(k for k in rows if "ew_lat" in k)
        assert rows[name]["scratch"] == 0 and rows[name]["vgprs"] + rows[name].get("agprs", 0) <= 512, rows[name]
    assert len([k for k in rows if k.startswith("srbdqp_wrench_ew_lat_kernel")]) == 6


class _StubEngine:
    """What MPC asks of its engine on the two routes of update(external_wrench=), recorded: NumPy staging arrays, the bound wrench call (which 'solves' by
    writing status 1), and the host-batch calls."""
    N, cap = 10, 2

    def __init__(self):
        N, cap = self.N, self.cap
        self.log = []
        self._h = C.c_void_p(1)
        self._st = dict(capacity=cap, x0=np.zeros((cap, 13)), x_ref=np.zeros((cap, N, 13)), foot=np.zeros((cap, N, 12)), contact=np.zeros((cap, N, 4), np.uint8),
                        pcom=np.zeros((cap, N, 3)), u=np.zeros((cap, N, 12)), x=np.zeros((cap, N + 1, 13)), status=np.zeros(cap, np.int32), iters=np.zeros(cap, np.int32))
        self._ew = np.zeros((cap, N, 6))

    def stage(self):
        return self._st

    def stage_ext_wrench(self):
        return self._ew

    def bind_update_wrench(self):
        def fn(*args):
            self.log.append(("srbdqp_update_wrench_f64", args[0], self._ew[0].copy()))
            self._st["status"][0], self._st["iters"][0] = 1, 35
            self._st["u"][0] = 7.0
            return 0
        return fn, ("with pcom",), ("without pcom",)

    def set_external_wrench(self, w):
        self.log.append(("set_external_wrench", None if w is None else np.array(w)))

    def solve(self, x0, x_ref, foot, contact, pcom=None, normals=None):
        self.log.append(("solve", normals))
        N = self.N
        return dict(u=np.full((1, N, 12), 3.0), x=np.zeros((1, N + 1, 13)), y=None, status=np.array([1], np.int32), iters=np.array([40], np.int32))

    def close(self):
        pass


def _mpc(staged_wrench):
    from g1_locomotion_amd import MPC
    mpc = MPC(horizon=_StubEngine.N) if staged_wrench is None else MPC(horizon=_StubEngine.N, staged_wrench=staged_wrench)
    mpc._engine = _StubEngine()
    return mpc, mpc._engine


def test_the_default_route_is_the_host_batch_solve():
    N = _StubEngine.N
    w = si.draw_wrench(1, N, 5)[0]
    for flag in (None, False):
        mpc, eng = _mpc(flag)
        assert mpc.staged_wrench is False
        u0, x1 = mpc.update(np.ones((N, 4)), np.zeros((N, 12)), None, external_wrench=w)
        assert [e[0] for e in eng.log] == ["set_external_wrench", "solve", "set_external_wrench"]
        assert np.array_equal(eng.log[0][1], w[None]) and eng.log[2][1] is None
        assert np.all(u0 == 3.0) and mpc.iters == 40


def test_staged_wrench_takes_the_new_call():
    N = _StubEngine.N
    w = si.draw_wrench(2, N, 6)
    mpc, eng = _mpc(True)
    u0, x1 = mpc.update(np.ones((N, 4)), np.full((N, 12), 0.25), None, external_wrench=w[0])
    assert [e[0] for e in eng.log] == ["srbdqp_update_wrench_f64"] and eng.log[0][1] == "without pcom" and np.array_equal(eng.log[0][2], w[0])
    assert np.all(eng.stage()["foot"][0] == 0.25) and np.all(eng.stage()["contact"][0] == 1)
    assert u0.shape == (12, 1) and np.all(u0 == 7.0) and x1.shape == (N + 1, 13) and mpc.status == 1 and mpc.iters == 35
    mpc.update(np.ones((N, 4)), np.zeros((N, 12)), np.zeros((N, 3)), external_wrench=w[1])       # bound once: the same call again, now with pcom
    assert [e[0] for e in eng.log] == ["srbdqp_update_wrench_f64"] * 2 and eng.log[1][1] == "with pcom" and np.array_equal(eng.log[1][2], w[1])
    with pytest.raises(ValueError, match="contact_normals and external_wrench together"):
        mpc.update(np.ones((N, 4)), np.zeros((N, 12)), None, external_wrench=w[0], contact_normals=np.tile([0.0, 0.0, 1.0], (N, 4)))
    assert len(eng.log) == 2


def test_the_new_kernels_have_a_code_object_of_their_own(built_lib):
    """The library's fat binary holds one offload bundle per translation unit.  The FIRST one is what the library's AQL loader reads (csrc/srbdqp_aql.hpp): it
    holds the plain call's batch-1 kernels and none of the low-latency wrench kernels, which would move them (csrc/srbdqp_wrench_lat_ew.hpp); a later one does."""
    import struct
    from g1_locomotion_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    def gfx950(at):
        """The gfx950 entry of the bundle at `at`, or None where the magic is not a bundle's (the loader's own copy of the string)."""
        (n,) = struct.unpack_from("<Q", blob, at + 24)
        pos = at + 32
        if not 1 <= n <= 16:
            return None
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, pos)
            if tl > 256 or at + off + size > len(blob):
                return None
            triple = blob[pos + 24:pos + 24 + tl]
            pos += 24 + tl
            if b"gfx950" in triple and size > 0:
                return blob[at + off:at + off + size]
        return None
    objs = [o for o in (gfx950(m.start()) for m in re.finditer(re.escape(magic), blob)) if o is not None]
    assert len(objs) == 2, len(objs)
    first, rest = objs[0], objs[1]
    assert b"srbdqp_wrench_kernel_inILi10ELi2E" in first and b"srbdqp_compact_kernel_inILi10ELi2E" in first
    assert b"srbdqp_wrench_ew_lat_kernel" not in first
    assert all(b"srbdqp_wrench_ew_lat_kernel_inILi%dE" % N in rest for N in (4, 8, 10))
    assert b"srbdqp_wrench_kernel_inILi10ELi2E" not in rest
