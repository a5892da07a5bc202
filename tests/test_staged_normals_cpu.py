"""CPU-side tests of the contact normals of one call on the staged path (include/srbdqp.h srbdqp_stage_contact_normals, srbdqp_solve_staged_normals_f64,
srbdqp_update_normals_f64): the three declarations against the binding's table and the library's exports, the resources of the low-latency MODE = 4
instantiations of the general kernel (no scratch), the code object they live in (the second one, with the low-latency wrench kernels), and the route
MPC.update(contact_normals=) takes with and without staged_normals=True -- on a stub engine, no GPU."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import side_inputs as si
from test_staged_wrench_cpu import rows  # noqa: F401  (the fixture: the build's resource remarks, both translation units)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("srbdqp_stage_contact_normals", "srbdqp_solve_staged_normals_f64", "srbdqp_update_normals_f64")


def test_the_header_declares_the_three_calls_and_the_table_holds_them():
    from g1_locomotion_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srbdqp.h")).read(), flags=re.S)
    params = {name: [p.strip() for p in " ".join(args.split()).split(",")]
              for name, args in re.findall(r"^int\s+(srbdqp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)}
    for name in CALLS:
        assert name in params and name in _lib.SIGNATURES and name in _lib.EXPORTS, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(params[name]), (name, params[name])
    assert params["srbdqp_stage_contact_normals"] == ["srbdqp_handle* h", "double** out"]
    assert [p.split()[-1] for p in params["srbdqp_solve_staged_normals_f64"]] == ["h", "B", "use_pcom", "use_warm", "want_x", "want_y"]
    # srbdqp_update_f64's parameters with the normals behind pcom
    plain = [p.split()[-1] for p in params["srbdqp_update_f64"]]
    assert [p.split()[-1] for p in params["srbdqp_update_normals_f64"]] == plain[:6] + ["normals"] + plain[6:]
    assert _lib.SIGNATURES["srbdqp_update_normals_f64"] == _lib.SIGNATURES["srbdqp_update_wrench_f64"]
    # srbdqp_stage keeps its layout: the normals array is not a field of it
    body = re.search(r"typedef struct srbdqp_stage \{(.*?)\} srbdqp_stage;", hdr, flags=re.S).group(1)
    assert "normal" not in body and len(re.findall(r"\*\s*\w+\s*;", body)) == 12


def test_the_library_exports_them(built_lib):
    from g1_locomotion_amd import _lib
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in CALLS:
        assert f" T {name}\n" in syms, name
        assert getattr(built_lib, name).restype is C.c_int
    # a null handle is refused, not dereferenced
    out = C.c_void_p()
    assert built_lib.srbdqp_stage_contact_normals(None, C.byref(out)) == _lib.E_INVALID
    assert built_lib.srbdqp_solve_staged_normals_f64(None, 1, 0, 0, 1, 0) == _lib.E_INVALID
    assert built_lib.srbdqp_update_normals_f64(None, *([None] * 11)) == _lib.E_INVALID


@pytest.mark.parametrize("N,XW", [(4, 1), (8, 2), (10, 2)])
def test_the_low_latency_normals_kernels_keep_nothing_in_scratch(rows, N, XW):  # noqa: F811
    """A MODE 4 low-latency kernel per horizon of the staged path's low-latency form, and its twin with the inputs in the argument segment: 0 bytes of scratch,
    and no more registers than one workgroup alone on its CU has (512 per lane at one wave per SIMD)."""
    for name in (f"srbdqp_wrench_cn_lat_kernel<{N}, {XW}>", f"srbdqp_wrench_cn_lat_kernel_in<{N}, {XW}>"):
        assert name in rows, sorted(k for k in rows if "cn_lat" in k)
        assert rows[name]["scratch"] == 0 and rows[name]["vgprs"] + rows[name].get("agprs", 0) <= 512, rows[name]
    assert len([k for k in rows if k.startswith("srbdqp_wrench_cn_lat_kernel")]) == 6


def _gfx950_objects(blob):
    """The gfx950 code objects of the offload bundles in a library's bytes, in file order."""
    def gfx950(at):
        (n,) = struct.unpack_from("<Q", blob, at + 24)
        pos = at + 32
        if not 1 <= n <= 16:                              # (the magic without a bundle behind it: the loader's own copy of the string)
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
    return [o for o in (gfx950(m.start()) for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)) if o is not None]


def test_the_new_kernels_live_in_the_second_code_object(built_lib):
    """Still two gfx950 code objects; the first -- what the library's AQL loader reads -- holds none of the low-latency normals kernels, the second all of them."""
    from g1_locomotion_amd import _lib
    objs = _gfx950_objects(open(_lib.LIB_PATH, "rb").read())
    assert len(objs) == 2, len(objs)
    first, second = objs
    assert b"srbdqp_wrench_cn_lat_kernel" not in first and b"srbdqp_wrench_kernel_inILi10ELi2E" in first
    assert all(b"srbdqp_wrench_cn_lat_kernel_inILi%dE" % N in second for N in (4, 8, 10))
    assert all(b"srbdqp_wrench_cn_lat_kernelILi%dE" % N in second for N in (4, 8, 10))


class _StubEngine:
    """What MPC asks of its engine on the two routes of update(contact_normals=), recorded: NumPy staging arrays, the bound normals call (which 'solves' by
    writing status 1), and the host-batch calls."""
    N, cap = 10, 2

    def __init__(self):
        N, cap = self.N, self.cap
        self.log = []
        self.binds = 0
        self._h = C.c_void_p(1)
        self._st = dict(capacity=cap, x0=np.zeros((cap, 13)), x_ref=np.zeros((cap, N, 13)), foot=np.zeros((cap, N, 12)), contact=np.zeros((cap, N, 4), np.uint8),
                        pcom=np.zeros((cap, N, 3)), u=np.zeros((cap, N, 12)), x=np.zeros((cap, N + 1, 13)), status=np.zeros(cap, np.int32), iters=np.zeros(cap, np.int32))
        self._cn = si.flat_normals(cap, N)

    def stage(self):
        return self._st

    def stage_contact_normals(self):
        return self._cn

    def bind_update_normals(self):
        self.binds += 1

        def fn(*args):
            self.log.append(("srbdqp_update_normals_f64", args[0], self._cn[0].copy(), self._cn[1].copy()))
            self._st["status"][0], self._st["iters"][0] = 1, 35
            self._st["u"][0] = 7.0
            return 0
        return fn, ("with pcom",), ("without pcom",)

    # the host-batch route: BatchMPC.solve(normals=) itself -- the setter, the solve, the setter again to restore the earlier state -- over the stub's two calls
    def set_contact_normals(self, n):
        self.log.append(("set_contact_normals", None if n is None else np.array(n)))

    def solve(self, x0, x_ref, foot, contact, pcom=None, *rest, normals=None):
        if normals is not None:
            from g1_locomotion_amd import BatchMPC
            return BatchMPC.solve(self, x0, x_ref, foot, contact, pcom, normals=normals)
        self.log.append(("solve",))
        N = self.N
        return dict(u=np.full((1, N, 12), 3.0), x=np.zeros((1, N + 1, 13)), y=None, status=np.array([1], np.int32), iters=np.array([40], np.int32))

    def close(self):
        pass


def _mpc(**kw):
    from g1_locomotion_amd import MPC
    mpc = MPC(horizon=_StubEngine.N, **kw)
    mpc._engine = _StubEngine()
    return mpc, mpc._engine


def test_the_default_route_is_the_host_batch_solve():
    N = _StubEngine.N
    nr = si.ridge_normals(1, N)[0]
    for kw in ({}, dict(staged_normals=False)):
        mpc, eng = _mpc(**kw)
        assert mpc.staged_normals is False
        u0, x1 = mpc.update(np.ones((N, 4)), np.zeros((N, 12)), None, contact_normals=nr)
        assert [e[0] for e in eng.log] == ["set_contact_normals", "solve", "set_contact_normals"]
        assert np.array_equal(eng.log[0][1], nr[None]) and eng.log[2][1] is None and eng.binds == 0
        assert np.all(u0 == 3.0) and mpc.iters == 40


@pytest.mark.parametrize("form", ["(N, 12)", "(N, 4, 3)", "list"])
def test_staged_normals_takes_the_new_call(form):
    N = _StubEngine.N
    nr = si.drawn_normals(2, N, np.random.default_rng(3), per_step=True)
    give = {"(N, 12)": lambda a: a, "(N, 4, 3)": lambda a: a.reshape(N, 4, 3), "list": lambda a: [row.reshape(4, 3) for row in a]}[form]
    mpc, eng = _mpc(staged_normals=True)
    flat = si.flat_normals(1, N)[0]
    u0, x1 = mpc.update(np.ones((N, 4)), np.full((N, 12), 0.25), None, contact_normals=give(nr[0]))
    assert [e[0] for e in eng.log] == ["srbdqp_update_normals_f64"] and eng.log[0][1] == "without pcom"
    assert np.array_equal(eng.log[0][2], nr[0]) and np.array_equal(eng.log[0][3], flat)           # row 0 of the staging array, and no other row
    assert np.all(eng.stage()["foot"][0] == 0.25) and np.all(eng.stage()["contact"][0] == 1)
    assert u0.shape == (12, 1) and np.all(u0 == 7.0) and x1.shape == (N + 1, 13) and mpc.status == 1 and mpc.iters == 35
    mpc.update(np.ones((N, 4)), np.zeros((N, 12)), np.zeros((N, 3)), contact_normals=give(nr[1]))   # bound once: the same call again, now with pcom
    assert [e[0] for e in eng.log] == ["srbdqp_update_normals_f64"] * 2 and eng.log[1][1] == "with pcom" and np.array_equal(eng.log[1][2], nr[1])
    assert eng.binds == 1
    with pytest.raises(ValueError, match="contact_normals and external_wrench together"):
        mpc.update(np.ones((N, 4)), np.zeros((N, 12)), None, external_wrench=np.zeros((N, 6)), contact_normals=give(nr[0]))
    assert len(eng.log) == 2
