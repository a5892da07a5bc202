"""CPU-side tests of the side input of one call on the staged path (include/srbdqp.h): an external wrench (srbdqp_stage_ext_wrench,
srbdqp_solve_staged_wrench_f64, srbdqp_update_wrench_f64) or contact normals (srbdqp_stage_contact_normals, srbdqp_solve_staged_normals_f64,
srbdqp_update_normals_f64).  Per kind: the three declarations against the binding's table and the library's exports, the resources of the low-latency
instantiations of the general kernel (MODE = 7 / MODE = 4: no scratch), the route MPC.update(external_wrench= / contact_normals=) takes with and without
staged_wrench=True / staged_normals=True -- on a stub engine, no GPU --, and the code object the kernels live in: their own, behind the one that holds the plain
call's batch-1 kernels."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import offload_bundles
import side_inputs as si

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


class Kind:
    """What differs between the two kinds on the CPU side."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


KINDS = {
    "wrench": Kind(
        calls=("srbdqp_stage_ext_wrench", "srbdqp_solve_staged_wrench_f64", "srbdqp_update_wrench_f64"), param="ext_wrench", word="wrench", tag="ew", mode=7,
        stage="stage_ext_wrench", bind="bind_update_wrench", setter="set_external_wrench", flag="staged_wrench", keyword="external_wrench",
        other=dict(contact_normals=np.tile([0.0, 0.0, 1.0], (10, 4))),
        neutral=lambda cap, N: np.zeros((cap, N, 6))),
    "normals": Kind(
        calls=("srbdqp_stage_contact_normals", "srbdqp_solve_staged_normals_f64", "srbdqp_update_normals_f64"), param="normals", word="normal", tag="cn", mode=4,
        stage="stage_contact_normals", bind="bind_update_normals", setter="set_contact_normals", flag="staged_normals", keyword="contact_normals",
        other=dict(external_wrench=np.zeros((10, 6))),
        neutral=si.flat_normals),
}


@pytest.fixture(params=list(KINDS))
def kind(request):
    return KINDS[request.param]


def test_the_header_declares_the_three_calls_and_the_table_holds_them(kind):
    from g1_locomotion_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srbdqp.h")).read(), flags=re.S)
    params = {name: [p.strip() for p in " ".join(args.split()).split(",")]
              for name, args in re.findall(r"^int\s+(srbdqp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)}
    stage, solve, update = kind.calls
    for name in kind.calls:
        assert name in params and name in _lib.SIGNATURES and name in _lib.EXPORTS, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(params[name]), (name, params[name])
    assert params[stage] == ["srbdqp_handle* h", "double** out"]
    assert [p.split()[-1] for p in params[solve]] == ["h", "B", "use_pcom", "use_warm", "want_x", "want_y"]
    # srbdqp_update_f64's parameters with the side input behind pcom
    plain = [p.split()[-1] for p in params["srbdqp_update_f64"]]
    assert [p.split()[-1] for p in params[update]] == plain[:6] + [kind.param] + plain[6:]
    assert _lib.SIGNATURES["srbdqp_update_normals_f64"] == _lib.SIGNATURES["srbdqp_update_wrench_f64"]
    # srbdqp_stage keeps its layout: the side input's array is not a field of it
    body = re.search(r"typedef struct srbdqp_stage \{(.*?)\} srbdqp_stage;", hdr, flags=re.S).group(1)
    assert kind.word not in body and len(re.findall(r"\*\s*\w+\s*;", body)) == 12


def test_the_library_exports_them(built_lib, kind):
    from g1_locomotion_amd import _lib
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    stage, solve, update = kind.calls
    for name in kind.calls:
        assert f" T {name}\n" in syms, name
        assert getattr(built_lib, name).restype is C.c_int
    # a null handle is refused, not dereferenced
    out = C.c_void_p()
    assert getattr(built_lib, stage)(None, C.byref(out)) == _lib.E_INVALID
    assert getattr(built_lib, solve)(None, 1, 0, 0, 1, 0) == _lib.E_INVALID
    assert getattr(built_lib, update)(None, *([None] * 11)) == _lib.E_INVALID


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
def test_the_low_latency_kernels_keep_nothing_in_scratch(rows, kind, N, XW):
    """A low-latency kernel of the kind's mode (7: wrench, 4: normals) per horizon of the staged path's low-latency form, and its twin with the inputs in the
    argument segment: 0 bytes of scratch, and no more registers than one workgroup alone on its CU has (512 per lane at one wave per SIMD)."""
    stem = f"srbdqp_wrench_{kind.tag}_lat_kernel"
    for name in (f"{stem}<{N}, {XW}>", f"{stem}_in<{N}, {XW}>"):
        assert name in rows, sorted(k for k in rows if f"{kind.tag}_lat" in k)
        assert rows[name]["scratch"] == 0 and rows[name]["vgprs"] + rows[name].get("agprs", 0) <= 512, rows[name]
    assert len([k for k in rows if k.startswith(stem)]) == 6


def test_the_kernels_have_a_code_object_of_their_own(built_lib, kind):
    """The library's fat binary holds one offload bundle per translation unit: two gfx950 code objects.  The FIRST one is what the library's AQL loader reads
    (csrc/srbdqp_aql.hpp): it holds the plain call's batch-1 kernels and none of the low-latency side-input kernels, which would move them
    (csrc/srbdqp_wrench_lat_ew.hpp); the second holds all of them."""
    from g1_locomotion_amd import _lib
    objs = offload_bundles.gfx950_objects(open(_lib.LIB_PATH, "rb").read())
    assert len(objs) == 2, len(objs)
    first, second = objs
    stem = b"srbdqp_wrench_%s_lat_kernel" % kind.tag.encode()
    assert b"srbdqp_wrench_kernel_inILi10ELi2E" in first and b"srbdqp_compact_kernel_inILi10ELi2E" in first
    assert stem not in first
    assert all(stem + b"_inILi%dE" % N in second for N in (4, 8, 10))
    assert all(stem + b"ILi%dE" % N in second for N in (4, 8, 10))
    assert b"srbdqp_wrench_kernel_inILi10ELi2E" not in second


class _StubEngine:
    """What MPC asks of its engine on the two routes of update() with a side input of `kind`, recorded: NumPy staging arrays, the bound call of the kind (which
    'solves' by writing status 1), and the host-batch calls.  It has the methods of its kind alone."""
    N, cap = 10, 2

    def __init__(self, kind):
        N, cap = self.N, self.cap
        self.kind = kind
        self.log = []
        self.binds = 0
        self._h = C.c_void_p(1)
        self._st = dict(capacity=cap, x0=np.zeros((cap, 13)), x_ref=np.zeros((cap, N, 13)), foot=np.zeros((cap, N, 12)), contact=np.zeros((cap, N, 4), np.uint8),
                        pcom=np.zeros((cap, N, 3)), u=np.zeros((cap, N, 12)), x=np.zeros((cap, N + 1, 13)), status=np.zeros(cap, np.int32), iters=np.zeros(cap, np.int32))
        self._side = kind.neutral(cap, N)
        setattr(self, kind.stage, lambda: self._side)
        setattr(self, kind.bind, self._bind)
        setattr(self, kind.setter, lambda v: self.log.append((kind.setter, None if v is None else np.array(v))))

    def stage(self):
        return self._st

    def _bind(self):
        self.binds += 1

        def fn(*args):
            self.log.append((self.kind.calls[2], args[0], self._side[0].copy(), self._side[1].copy()))
            self._st["status"][0], self._st["iters"][0] = 1, 35
            self._st["u"][0] = 7.0
            return 0
        return fn, ("with pcom",), ("without pcom",)

    # the host-batch route.  Normals: BatchMPC.solve(normals=) itself -- the setter, the solve, the setter again to restore the earlier state -- over the stub's
    # two calls; the wrench: MPC sets and clears it around the solve
    def solve(self, x0, x_ref, foot, contact, pcom=None, *rest, normals=None):
        if normals is not None:
            from g1_locomotion_amd import BatchMPC
            return BatchMPC.solve(self, x0, x_ref, foot, contact, pcom, normals=normals)
        self.log.append(("solve",))
        N = self.N
        return dict(u=np.full((1, N, 12), 3.0), x=np.zeros((1, N + 1, 13)), y=None, status=np.array([1], np.int32), iters=np.array([40], np.int32))

    def close(self):
        pass


def _mpc(kind, **kw):
    from g1_locomotion_amd import MPC
    mpc = MPC(horizon=_StubEngine.N, **kw)
    mpc._engine = _StubEngine(kind)
    return mpc, mpc._engine


def test_the_default_route_is_the_host_batch_solve(kind):
    N = _StubEngine.N
    v = si.draw_wrench(1, N, 5)[0] if kind.tag == "ew" else si.ridge_normals(1, N)[0]
    for kw in ({}, {kind.flag: False}):
        mpc, eng = _mpc(kind, **kw)
        assert getattr(mpc, kind.flag) is False
        u0, x1 = mpc.update(np.ones((N, 4)), np.zeros((N, 12)), None, **{kind.keyword: v})
        assert [e[0] for e in eng.log] == [kind.setter, "solve", kind.setter]
        assert np.array_equal(eng.log[0][1], v[None]) and eng.log[2][1] is None and eng.binds == 0
        assert np.all(u0 == 3.0) and mpc.iters == 40


# (the wrench comes as (N, 6); normals in the three forms set_contact_normals takes)
@pytest.mark.parametrize("name,form", [("wrench", "(N, 6)"), ("normals", "(N, 12)"), ("normals", "(N, 4, 3)"), ("normals", "list")])
def test_the_staged_flag_takes_the_new_call(name, form):
    kind, N = KINDS[name], _StubEngine.N
    v = si.draw_wrench(2, N, 6) if name == "wrench" else si.drawn_normals(2, N, np.random.default_rng(3), per_step=True)
    give = {"(N, 6)": lambda a: a, "(N, 12)": lambda a: a, "(N, 4, 3)": lambda a: a.reshape(N, 4, 3), "list": lambda a: [row.reshape(4, 3) for row in a]}[form]
    update = kind.calls[2]
    mpc, eng = _mpc(kind, **{kind.flag: True})
    neutral = kind.neutral(1, N)[0]
    u0, x1 = mpc.update(np.ones((N, 4)), np.full((N, 12), 0.25), None, **{kind.keyword: give(v[0])})
    assert [e[0] for e in eng.log] == [update] and eng.log[0][1] == "without pcom"
    assert np.array_equal(eng.log[0][2], v[0]) and np.array_equal(eng.log[0][3], neutral)         # row 0 of the staging array, and no other row
    assert np.all(eng.stage()["foot"][0] == 0.25) and np.all(eng.stage()["contact"][0] == 1)
    assert u0.shape == (12, 1) and np.all(u0 == 7.0) and x1.shape == (N + 1, 13) and mpc.status == 1 and mpc.iters == 35
    mpc.update(np.ones((N, 4)), np.zeros((N, 12)), np.zeros((N, 3)), **{kind.keyword: give(v[1])})   # bound once: the same call again, now with pcom
    assert [e[0] for e in eng.log] == [update] * 2 and eng.log[1][1] == "with pcom" and np.array_equal(eng.log[1][2], v[1])
    assert eng.binds == 1
    with pytest.raises(ValueError, match="contact_normals and external_wrench together"):
        mpc.update(np.ones((N, 4)), np.zeros((N, 12)), None, **{kind.keyword: give(v[0])}, **kind.other)
    assert len(eng.log) == 2
