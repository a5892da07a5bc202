"""CPU-side tests of SRBDQP_FLAG_ANY_HORIZON (include/srbdqp.h): what srbdqp_create admits with and without the flag, the flag's value on both sides of the
C-ABI, and the resources of the seven MODE = 3 (live-horizon) instantiations of the general kernel against their MODE = 0 twins -- with the rows of every
instantiation that existed before the flag pinned, since the flag must not move one of them."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TABULATED = (4, 8, 10, 12, 16, 20, 24)


def _create(lib, horizon, flags, kernel=None):
    from g1_locomotion_amd import _lib
    cfg = _lib.default_config()
    cfg.horizon = horizon
    cfg.flags = flags
    if kernel is not None:
        cfg.kernel = kernel
    h = C.c_void_p()
    rc = lib.srbdqp_create(C.byref(cfg), C.byref(h))
    if rc == _lib.OK:
        assert lib.srbdqp_destroy(h) == _lib.OK
    else:
        assert not h.value and lib.srbdqp_last_error(None)
    return rc


def test_the_flag_admits_every_horizon_from_1_to_24(built_lib):
    """With the flag a horizon without instantiations of its own passes srbdqp_create's checks: what is left to fail is the device (no GPU: E_NO_DEVICE).
    Horizons outside 1 ... 24 stay invalid, and so does an explicit kernel that has no live-horizon form."""
    import torch
    from g1_locomotion_amd import _lib
    want = _lib.OK if torch.cuda.is_available() else _lib.E_NO_DEVICE
    for n in range(1, 25):
        assert _create(built_lib, n, _lib.FLAG_ANY_HORIZON) == want, n
    assert _create(built_lib, 7, _lib.FLAG_ANY_HORIZON | _lib.FLAG_TIMING) == want
    assert _create(built_lib, 7, _lib.FLAG_ANY_HORIZON, _lib.KERNEL_WRENCH) == want
    for n in (0, 25, -3):
        assert _create(built_lib, n, _lib.FLAG_ANY_HORIZON) == _lib.E_INVALID, n
    for kern in (_lib.KERNEL_COMPACT, _lib.KERNEL_SPLIT, _lib.KERNEL_WAVE):
        assert _create(built_lib, 7, _lib.FLAG_ANY_HORIZON, kern) == _lib.E_INVALID
        assert b"SRBDQP_FLAG_ANY_HORIZON" in built_lib.srbdqp_last_error(None)
        assert _create(built_lib, 10, _lib.FLAG_ANY_HORIZON, kern) == want          # a tabulated horizon: the flag changes nothing


def test_without_the_flag_nothing_changes(built_lib):
    from g1_locomotion_amd import _lib
    for n in (7, 1, 15, 23, 0, 25, -3):
        assert _create(built_lib, n, 0) == _lib.E_INVALID, n
        assert _create(built_lib, n, _lib.FLAG_TIMING | _lib.FLAG_NO_LAT) == _lib.E_INVALID, n


def test_the_flag_is_128_on_both_sides(built_lib):
    from g1_locomotion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "srbdqp.h")).read()
    m = re.search(r"#define\s+SRBDQP_FLAG_ANY_HORIZON\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 128 == _lib.FLAG_ANY_HORIZON
    others = [int(v) for v in re.findall(r"#define\s+SRBDQP_FLAG_(?!ANY_HORIZON)\w+\s+(\d+)", hdr)]
    assert 128 not in others and all(v & 128 == 0 for v in others)
    assert _lib.HORIZONS == TABULATED


def test_the_python_wrappers_set_the_flag_themselves(built_lib, monkeypatch):
    """BatchMPC / RaggedMPC pass the flag exactly when a horizon needs it (seen through a recording srbdqp_create: no device needed)."""
    from g1_locomotion_amd import BatchMPC, RaggedMPC, SrbdqpError, _lib
    seen = []

    class Recording:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            return getattr(self._lib, name)

        def srbdqp_create(self, cfg, out):
            seen.append((cfg._obj.horizon, cfg._obj.flags))
            return _lib.E_NO_DEVICE

        def srbdqp_ragged_create(self, cfg, hz, n, out):
            seen.append(("ragged", cfg._obj.flags))
            return _lib.E_NO_DEVICE

    rec = Recording(built_lib)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    for n, flags in ((10, 0), (15, _lib.FLAG_ANY_HORIZON), (1, _lib.FLAG_ANY_HORIZON), (24, 0)):
        with pytest.raises(SrbdqpError):
            BatchMPC(horizon=n)
        assert seen[-1] == (n, flags)
    with pytest.raises(SrbdqpError):
        BatchMPC(horizon=7, timing=True)
    assert seen[-1] == (7, _lib.FLAG_ANY_HORIZON | _lib.FLAG_TIMING)
    for hz, flags in (((8, 12, 16, 24), 0), ((6, 9, 15, 22), _lib.FLAG_ANY_HORIZON), ((8, 11), _lib.FLAG_ANY_HORIZON)):
        with pytest.raises(SrbdqpError):
            RaggedMPC(horizons=hz)
        assert seen[-1] == ("ragged", flags)


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
    return {r["name"].strip(): r for r in resource_table.parse(log)}


# scratch bytes per lane a MODE = 3 kernel may keep BEYOND its twin's (measured) -- none
LIVE_SCRATCH_OVER_TWIN = {}


@pytest.mark.parametrize("N", TABULATED)
def test_live_horizon_kernels_cost_what_their_twins_cost(rows, N):
    """One MODE = 3 instantiation per tabulated horizon, in the shape of the batch kernel that ships for it (waves per SIMD, the three set-up helper waves at
    N = 24): no more scratch than that MODE = 0 twin, at its occupancy, within the register file."""
    live = [r for name, r in rows.items() if name.startswith(f"srbdqp_wrench_kernel<{N}, double, double, 3, ")]
    assert len(live) == 1, [r["name"] for r in live]
    live = live[0]
    m = re.match(rf"srbdqp_wrench_kernel<{N}, double, double, 3, (\d+), double, 5, (\d+)", live["name"].strip())
    wps, xw = int(m.group(1)), int(m.group(2))
    assert xw == (3 if N == 24 else 0)
    twin = rows[f"srbdqp_wrench_kernel<{N}, double, double, 0, {wps}, double, 5, {xw}>"]
    print(N, "live", {k: live[k] for k in ("vgprs", "sgprs", "scratch", "occupancy")}, "twin", {k: twin[k] for k in ("vgprs", "sgprs", "scratch", "occupancy")})
    assert live["scratch"] <= twin["scratch"] + LIVE_SCRATCH_OVER_TWIN.get(N, 0), (live["name"], live["scratch"], twin["scratch"])
    assert live["occupancy"] >= twin["occupancy"], (live["name"], live["occupancy"], twin["occupancy"])
    assert live["vgprs"] + live["agprs"] <= 512 // twin["occupancy"]


# (VGPRs, AGPRs, SGPRs, scratch bytes per lane, waves per SIMD) of every instantiation of the general kernel that existed before the flag
# (three entries re-pinned with the conditioning guard of phase E, which changed the kernels themselves: N = 16 fp32 on fp64 tiles 224 -> 216 bytes of scratch,
#  the N = 4 low-latency pair 174 -> 176 VGPRs; occupancy as before)
BEFORE = {
    "srbdqp_wrench_kernel<24, float, float, 0, 2, double, 5, 3>": (256, 0, 106, 92, 2),
    "srbdqp_wrench_kernel<24, float, float, 0, 3, float, 5, 0>": (168, 0, 106, 64, 3),
    "srbdqp_wrench_kernel<24, double, double, 1, 1, double, 5, 0>": (194, 0, 67, 0, 2),
    "srbdqp_wrench_kernel<24, double, double, 0, 1, double, 5, 3>": (256, 0, 106, 20, 2),
    "srbdqp_wrench_kernel<20, float, float, 0, 2, double, 5, 0>": (254, 0, 106, 0, 2),
    "srbdqp_wrench_kernel<20, float, float, 0, 3, float, 5, 0>": (168, 0, 106, 0, 3),
    "srbdqp_wrench_kernel<20, double, double, 1, 2, double, 5, 0>": (194, 0, 55, 0, 2),
    "srbdqp_wrench_kernel<20, double, double, 2, 2, double, 5, 0, void>": (256, 0, 106, 0, 2),
    "srbdqp_wrench_kernel<20, double, double, 0, 2, double, 5, 0>": (256, 0, 106, 0, 2),
    "srbdqp_wrench_kernel<16, float, float, 0, 3, double, 5, 0>": (168, 0, 106, 216, 3),
    "srbdqp_wrench_kernel<16, float, float, 0, 3, float, 5, 0>": (168, 0, 106, 0, 3),
    "srbdqp_wrench_kernel<16, double, double, 1, 2, double, 5, 0>": (158, 0, 53, 0, 3),
    "srbdqp_wrench_kernel<16, double, double, 2, 2, double, 5, 0, void>": (230, 0, 106, 0, 2),
    "srbdqp_wrench_kernel<16, double, double, 0, 2, double, 5, 0>": (230, 0, 106, 0, 2),
    "srbdqp_wrench_kernel<12, float, float, 0, 3, double, 5, 0>": (168, 0, 106, 116, 3),
    "srbdqp_wrench_kernel<12, float, float, 0, 3, float, 5, 0>": (168, 0, 106, 0, 3),
    "srbdqp_wrench_kernel<12, double, double, 1, 3, double, 5, 0>": (148, 0, 55, 0, 3),
    "srbdqp_wrench_kernel<12, double, double, 2, 3, double, 5, 0, void>": (165, 0, 106, 0, 3),
    "srbdqp_wrench_kernel<12, double, double, 0, 3, double, 5, 0>": (165, 0, 106, 0, 3),
    "srbdqp_wrench_kernel<10, float, float, 0, 3, double, 5, 0>": (165, 0, 106, 0, 3),
    "srbdqp_wrench_kernel<10, float, float, 0, 3, float, 5, 0>": (167, 0, 106, 20, 3),
    "srbdqp_wrench_kernel<10, double, double, 1, 3, double, 5, 0>": (148, 0, 51, 0, 3),
    "srbdqp_wrench_kernel<10, double, double, 2, 3, double, 5, 0, void>": (164, 0, 106, 0, 3),
    "srbdqp_wrench_kernel<10, double, double, 0, 1, double, 5, 2>": (227, 40, 106, 0, 1),
    "srbdqp_wrench_kernel_in<10, 2>": (227, 40, 106, 0, 1),
    "srbdqp_wrench_kernel<10, double, double, 0, 3, double, 5, 0>": (165, 0, 106, 0, 3),
    "srbdqp_wrench_kernel<8, float, float, 0, 3, double, 5, 0>": (167, 0, 106, 12, 3),
    "srbdqp_wrench_kernel<8, float, float, 0, 3, float, 5, 0>": (168, 0, 106, 0, 3),
    "srbdqp_wrench_kernel<8, double, double, 1, 3, double, 5, 0>": (130, 0, 55, 0, 3),
    "srbdqp_wrench_kernel<8, double, double, 2, 3, double, 5, 0, void>": (152, 0, 106, 0, 3),
    "srbdqp_wrench_kernel<8, double, double, 0, 1, double, 5, 2>": (202, 32, 106, 0, 2),
    "srbdqp_wrench_kernel_in<8, 2>": (202, 32, 101, 0, 2),
    "srbdqp_wrench_kernel<8, double, double, 0, 3, double, 5, 0>": (152, 0, 106, 0, 3),
    "srbdqp_wrench_kernel<4, float, float, 0, 3, double, 5, 0>": (158, 0, 104, 0, 3),
    "srbdqp_wrench_kernel<4, float, float, 0, 3, float, 5, 0>": (142, 0, 106, 0, 3),
    "srbdqp_wrench_kernel<4, double, double, 1, 3, double, 5, 0>": (124, 0, 61, 0, 4),
    "srbdqp_wrench_kernel<4, double, double, 2, 3, double, 5, 0, void>": (130, 0, 104, 0, 3),
    "srbdqp_wrench_kernel<4, double, double, 0, 1, double, 5, 1>": (176, 24, 94, 0, 2),
    "srbdqp_wrench_kernel_in<4, 1>": (176, 24, 90, 0, 2),
    "srbdqp_wrench_kernel<4, double, double, 0, 3, double, 5, 0>": (130, 0, 102, 0, 3),
}


def test_the_kernels_that_existed_before_are_allocated_as_before(rows):
    """MODE = 0 / 1 / 2 read (LH ? ... : ...) with LH a compile-time false: their registers, scratch and occupancy are what they were, kernel by kernel."""
    got = {k: tuple(rows[k][f] for f in ("vgprs", "agprs", "sgprs", "scratch", "occupancy")) for k in BEFORE if k in rows}
    assert got == BEFORE, {k: (got.get(k), BEFORE[k]) for k in BEFORE if got.get(k) != BEFORE[k]}
    # ... and the general kernel has no other instantiation than those and the seven live-horizon ones
    others = sorted(k for k in rows if k.startswith("srbdqp_wrench_kernel") and k not in BEFORE)
    assert [re.sub(r", \d+, double, 5, \d+, void>$", "", k) for k in others] == sorted(f"srbdqp_wrench_kernel<{N}, double, double, 3" for N in TABULATED), others
