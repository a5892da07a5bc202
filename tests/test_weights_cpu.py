"""CPU-side tests of the per-QP cost weights (include/srbdqp.h srbdqp_weights, srbdqp_set_weights): the record's layout on both sides of the C-ABI, the
exported setters, weights_array(), the oracle's closed forms under arbitrary weights (what the kernels assemble: nothing in them assumes the default
q_diag / r_diag), and the resources of the MODE = 6 instantiations of the general kernel that read the records (no scratch, occupancy no lower than the
MODE = 0 twin)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scenarios as sc
import side_inputs as si
import srbd_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIELDS = ("q_diag", "r_diag", "reserved")


def test_weights_struct_matches_the_header(tmp_path, built_lib):
    from g1_locomotion_amd import _lib
    assert C.sizeof(_lib.Weights) == 128 and _lib.WEIGHTS_DOUBLES * 8 == 128
    src = tmp_path / "weights.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srbdqp.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(srbdqp_weights));\n'
                   + "".join(f'    printf(" %zu", offsetof(srbdqp_weights, {f}));\n' for f in FIELDS) + "    return 0;\n}\n")
    exe = tmp_path / "weights"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.Weights)
    assert got[1:] == [getattr(_lib.Weights, f).offset for f in FIELDS]
    assert [getattr(_lib.Weights, f).offset // 8 for f in FIELDS] == [0, 13, 14]   # the columns of weights_array()


def test_the_setters_are_exported(built_lib):
    from g1_locomotion_amd import _lib
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in ("srbdqp_set_weights", "srbdqp_set_weights_device", "srbdqp_ragged_set_weights", "srbdqp_ragged_set_weights_device"):
        assert f" T {name}\n" in syms, name
        assert name in _lib.EXPORTS
        assert getattr(built_lib, name).restype is C.c_int
    # a null handle is refused, not dereferenced
    rec = (_lib.Weights * 1)()
    assert built_lib.srbdqp_set_weights(None, C.cast(rec, C.c_void_p), 1) == _lib.E_INVALID
    assert built_lib.srbdqp_set_weights_device(None, None, 0) == _lib.E_INVALID
    assert built_lib.srbdqp_ragged_set_weights(None, C.cast(rec, C.c_void_p), 1) == _lib.E_INVALID
    assert built_lib.srbdqp_ragged_set_weights_device(None, None, 0) == _lib.E_INVALID


def test_weights_array_broadcasts_and_fills_the_config(built_lib):
    from g1_locomotion_amd import _lib
    from g1_locomotion_amd.mpc import weights_array
    cfg = _lib.default_config()
    a = weights_array(3)
    assert a.shape == (3, 16) and a.dtype == np.float64
    assert np.all(a[:, :13] == np.array(list(cfg.q_diag))) and np.all(a[:, 13] == cfg.r_diag) and np.all(a[:, 14:] == 0.0)
    q = np.arange(1.0, 14.0)
    a = weights_array(3, q_diag=q, r_diag=np.array([1e-4, 2e-4, 3e-4]))
    assert np.all(a[:, :13] == q) and np.array_equal(a[:, 13], [1e-4, 2e-4, 3e-4])
    qb = np.arange(26.0).reshape(2, 13)
    a = weights_array(2, q_diag=qb, r_diag=5e-4)
    assert np.array_equal(a[:, :13], qb) and np.all(a[:, 13] == 5e-4)
    assert np.all(weights_array(2, q_diag=7.0)[:, :13] == 7.0) and np.all(weights_array(2, q_diag=7.0)[:, 13] == cfg.r_diag)
    # another config's weights
    cfg.r_diag = 2.5e-3
    cfg.q_diag[5] = 77.0
    a = weights_array(2, cfg=cfg)
    assert np.all(a[:, 13] == 2.5e-3) and np.all(a[:, 5] == 77.0)
    assert weights_array(0).shape == (0, 16)
    for bad in (dict(q_diag=np.ones(12)), dict(q_diag=np.ones((2, 13))), dict(q_diag=np.ones((13, 3))), dict(r_diag=np.ones(2)), dict(r_diag=np.ones((3, 1)))):
        with pytest.raises(ValueError):
            weights_array(3, **bad)
    with pytest.raises(ValueError):
        weights_array(-1)
    # a record array is what Weights describes, row by row; the draw of the tests has the same layout
    a = weights_array(2, r_diag=[1e-3, 2e-3])
    recs = (_lib.Weights * 2).from_buffer_copy(a.tobytes())
    assert recs[1].r_diag == 2e-3 and list(recs[0].q_diag) == list(_lib.default_config().q_diag) and list(recs[0].reserved) == [0.0, 0.0]
    d = si.draw_weights(4, 1)
    assert d.shape == (4, 16) and np.all(d[:, 14:] == 0.0) and np.all(d[0, 0:3] == 0.0) and np.all(d[0, 6:9] == 0.0) and np.all(d[1, :13] == 0.0) and np.all(d[:, 13] > 0.0)


@pytest.mark.parametrize("N,schedule", [(4, "three"), (10, "single"), (10, "mixed"), (16, "double"), (20, "three")])
def test_the_closed_forms_hold_for_arbitrary_weights(N, schedule):
    """For the first four QPs of the GPU tests' draw -- zero angular weights, all q = 0 and two ordinary draws -- the closed-form Hessian and gradient (pair
    form and rank-6 form) agree with the presolved build_qp() to 1e-11 relative, and wrench_reduce() + wrench_kinv_op() invert K = P + sigma I + A' rho A to
    the 1e-8 of the refined inverse that tests/test_oracle_turning.py::test_wrench_reduction_is_the_inverse_of_the_dense_k asks.  (This exercises the oracle
    alone -- the twin the GPU tests compare against --, so it does not depend on the setters: it passes with or without them.)"""
    B = 4
    x0, xr, ft, ct = si.batch(B, N, si.batch_seed(N, schedule), schedule)
    rec = si.draw_weights(B, si.weights_seed(N))
    for b in range(B):
        p = si.params(N, weights=rec[b])
        red, vi, ri = orc.presolve(orc.build_qp(p, x0[b], xr[b], ft[b], ct[b]), ct[b])
        P, q, vi2 = orc.closed_form_hessian_gradient(p, x0[b], xr[b], ft[b], ct[b])
        np.testing.assert_array_equal(vi, vi2)
        sP, sq = np.abs(red["P"]).max(), max(1.0, np.abs(red["q"]).max())
        assert np.abs(P - red["P"]).max() <= 1e-11 * sP, (b, np.abs(P - red["P"]).max() / sP)
        assert np.abs(q - red["q"]).max() <= 1e-11 * sq, (b, np.abs(q - red["q"]).max() / sq)
        P6 = orc.closed_form_hessian_rank6(p, xr[b], ft[b], ct[b])
        assert P6.shape == P.shape and np.abs(P6 - red["P"]).max() <= 1e-11 * sP, (b, np.abs(P6 - red["P"]).max() / sP)
        wr = orc.wrench_reduce(p, xr[b], ft[b], ct[b])
        np.testing.assert_array_equal(vi, wr["vi"])
        Kinv, res = sc.refined_inverse(sc.dense_k(p, red))
        assert res <= 1e-11
        op = orc.wrench_kinv_op(wr)
        Kw = np.stack([op(e) for e in np.eye(len(vi))], axis=1)
        assert np.abs(Kw - Kinv).max() <= 1e-8 * np.abs(Kinv).max(), (b, np.abs(Kw - Kinv).max() / np.abs(Kinv).max())


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
def test_weight_kernels_keep_nothing_in_scratch_and_their_occupancy(rows, N):
    """One srbdqp_wrench_wt_kernel per horizon the setters accept, with 0 bytes of scratch and the occupancy of its MODE = 0 twin (the batch kernel of the
    same N and waves per SIMD)."""
    by = {r["name"].strip(): r for r in rows}
    wk = [r for name, r in by.items() if name.startswith(f"srbdqp_wrench_wt_kernel<{N}, ")]
    assert len(wk) == 1, [r["name"] for r in wk]
    wk = wk[0]
    wps = int(re.match(rf"srbdqp_wrench_wt_kernel<{N}, (\d+)>", wk["name"].strip()).group(1))
    twin = by[f"srbdqp_wrench_kernel<{N}, double, double, 0, {wps}, double, 5, 0>"]
    assert wk["scratch"] == 0, (wk["name"], wk["scratch"])
    assert wk["occupancy"] >= twin["occupancy"], (wk["name"], wk["occupancy"], twin["occupancy"])


def test_no_weight_kernel_at_n24(rows):
    """N = 24 has no MODE = 6 instantiation (as it has no MODE = 2 one): the setters refuse it instead."""
    assert [r for r in rows if r["name"].strip().startswith("srbdqp_wrench_wt_kernel<")]
    assert not [r for r in rows if r["name"].strip().startswith("srbdqp_wrench_wt_kernel<24, ")]
