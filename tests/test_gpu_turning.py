"""GPU parity of every kernel family that ships on turning, stepping and uneven-ground horizons (tests/scenarios.py::turning_batch): a yaw
that changes from step to step ("turn" ramps, "wrap" ramps through +-pi, "random" per step), footholds that move at every touch-down and lie
at different heights, non-zero roll / pitch / angular-velocity / v_z references.  On the constant-yaw, fixed-foothold inputs of
synthetic_batch() a kernel that reads the yaw or the foothold of the wrong step is bit-identical to a correct one
(tests/test_oracle_turning.py::test_a_wrong_step_index_is_invisible_on_the_old_inputs_and_visible_on_these); here it is not.

Tolerances, stated once -- none is new, each is the one the existing file of that family states:
  assembly, entry by entry (P, q, T, V, Bd vs the oracle's dense products / wrench_reduce):   1e-11 relative  (test_gpu_parity / test_gpu_wrench)
  general kernel's operator Bd + V' T^-1 V vs the refined inverse of the dense K:             1e-8 relative   (test_gpu_wrench)
  fp64 forces vs the ADMM twin TOL_TWIN_N = 2e-3 N, iterations within one check; vs the exact optimum TOL_EXACT_N = 5e-2 N
  fp32 forces vs the fp32 twin TOL32_TWIN_N = 2e-2 N, iterations within two checks; vs the exact optimum TOL32_EXACT_N = 1e-1 N
  roll-out (all 13 rows, the Euler-angle sum included) 1e-5 fp64 / 1e-3 fp32 (staged batch-1: 1e-4, as its test); KKT of the returned pair:
  primal <= 1e-4, stationarity <= 1e-3 max(1, |q|_inf); swing forces and duals exactly 0
  at scale vs the C oracle: statuses equal, |iters difference| <= check_every, forces <= TOL_TWIN_N (<= 1e-4 N where the counts are equal);
  roll-out vs the dense model on the kernel's own forces 1e-8 (reasoned in the test)
  two-phase vs one-shot: statuses equal, iterations within 5, forces 1e-6 N, states 1e-8 (test_two_phase_call_equals_the_one_shot_call)
  non-default constants vs the C oracle: forces <= 1e-3 N where the counts are equal, <= 5 TOL_TWIN_N else, states 1e-4
  (test_non_default_constants_reach_every_kernel)
A QP the oracle itself leaves at the iteration cap is held to its twin only.  Every solve case asserts ON THE ORACLE's result that at least
3/4 of its QPs are solved and that at least one has a force on a friction or fz bound (seeds were chosen on the CPU for that).

Worst deviation observed on an MI355X per group, next to its bound (printed at the end of a run with -s):
  a. assembly    4-wave P 1.1e-15, q 2.2e-15; one-wave P 8.2e-16, q 4.6e-16; general T 7.2e-13, q 8.8e-16, V 3.5e-12, Bd 5.5e-12       / 1e-11
                 (the float64 reference's own V / Bd error on these inputs: up to 2.5e-12); general operator vs the refined inverse 3.6e-9 / 1e-8
  b. solve fp64  twin: one-wave and split 2.7e-8, 4-wave 8.1e-7, general 1.2e-5 / 2e-3 N; exact: 1.8e-3, 3.1e-3, 4.3e-3 / 5e-2 N;
                 roll-out 6.5e-9, 3.6e-8, 8.3e-6 (general, N = 24) / 1e-5
     solve fp32  twin 7.2e-4 (fp64 tiles), 1.9e-3 (fp32 tiles) / 2e-2 N; exact 5.5e-3, 4.9e-3 / 1e-1 N; roll-out 3.8e-4, 2.5e-4 / 1e-3
  c. batch-1     staged: twin 2.9e-8 (4-wave lat), 5.1e-7 (general lat) / 2e-3 N, exact 3.1e-3 / 5e-2 N, roll-out 1.5e-6 / 1e-4;
                 MPC.update twin 6.7e-7 / 2e-3 N, roll-out 1.2e-6 / 1e-5; two-phase vs one-shot forces 1.9e-10 / 1e-6 N, states 8.6e-11 / 1e-8
  d. at scale    forces vs the C oracle, all QPs = equal counts: one-wave 4.5e-7, 4-wave 5.0e-7, general 5.9e-6 / 1e-4 N;
                 roll-out vs the dense model on the kernel's own forces 3.3e-13 / 1e-8
  e. ragged      twin 1.0e-6 / 2e-3 N, exact 1.7e-3 / 5e-2 N, roll-out 6.7e-6 / 1e-5
  f. constants   general fp64 vs the C oracle 5.5e-8 / 1e-3 N, states 8.2e-8 / 1e-4; fp32 twin 2.2e-4 / 2e-2 N, exact 2.0e-2 / 1e-1 N;
                 zeroed groups and rho_fz_scale, all three kernels: forces <= 1.1e-7 / 1e-3 N, states <= 1.3e-7 / 1e-4
  golden         twin 2.0e-7 / 2e-3 N, exact 1.9e-3 / 5e-2 N, states vs the exact roll-out 8.5e-6 / 1e-4
"""
import functools
import os

import numpy as np
import pytest

import scenarios as sc
import srbd_oracle as orc
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TOL_TWIN_N = 2e-3          # tests/test_gpu_parity.py, tests/test_gpu_wrench.py
TOL_EXACT_N = 5e-2
TOL32_TWIN_N = 2e-2        # tests/test_gpu_wrench.py
TOL32_EXACT_N = 1e-1
TOL_ASM = 1e-11
TOL_KINV = 1e-8

_worst = {}      # group -> [worst deviation of this run, bound]


def _note(group, value, bound):
    w = _worst.setdefault(group, [0.0, bound])
    w[0] = max(w[0], float(value))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst observed deviation / bound, per group")
    for g in sorted(_worst):
        print(f"  {g:44s} {_worst[g][0]:.3e} / {_worst[g][1]:.0e}")


def _engine(N, **kw):
    from g1_locomotion_amd import BatchMPC
    kw.setdefault("rho_restart_iter", -1)       # off unless the test is about it
    return BatchMPC(horizon=N, **kw)


# seeds: one per (horizon, pattern, yaw kind); five of them moved on, chosen on the CPU from the ORACLE's result alone so that the case holds the
# conditions above (3/4 of its QPs solved by the fixed-rho twin, a force on a bound).  A sixth, (20, "three", "random"), because the REFERENCE does
# not hold the assembly bound on the first draw: one step's three stance contacts are nearly collinear (cond E = 1e8) and orc.wrench_reduce()'s own
# float64 Bd is 1.1e-11 from the same block formed in extended precision (the kernel's was 1.2e-11 from the reference);
# tests/test_oracle_turning.py::test_wrench_reference_holds_the_assembly_bound_on_the_gpu_inputs keeps every assembly input under 3e-12.
SEED_SHIFT = {(10, "single", "random"): 1000, (4, "single", "turn"): 1000, (20, "three", "wrap"): 1000, (24, "single", "wrap"): 2000, (24, "mixed", "turn"): 2000,
              (20, "three", "random"): 1000}


def _seed(N, schedule, yaw):
    return 6000 + 10 * N + 3 * ("single", "double", "mixed", "three").index(schedule) + sc.YAW_KINDS.index(yaw) + SEED_SHIFT.get((N, schedule, yaw), 0)


@functools.lru_cache(maxsize=None)
def _inputs(N, schedule, yaw, B, dt=0.04):
    return sc.batch(B, N, _seed(N, schedule, yaw), schedule, yaw=yaw, pcom=True, dt=dt)


def _conditions(statuses, forces, ct, p):
    """The conditions that keep a solve case honest, on the ORACLE's result."""
    statuses = np.asarray(statuses)
    assert (statuses == orc.STATUS_SOLVED).mean() >= 0.75, statuses
    assert any(sc.bound_active(forces[b], ct[b], p) for b in range(len(statuses)) if statuses[b] == orc.STATUS_SOLVED)


@functools.lru_cache(maxsize=None)
def _twin64(N, schedule, yaw, B, use_pcom=False):
    """Per QP: the fp64 twin (orc.update, fixed rho) and, where it is solved, the exact optimum.  Cached: the kernels of a family share it."""
    x0, xr, ft, ct, pc = _inputs(N, schedule, yaw, B)
    p = orc.params_for(N)
    refs = []
    for b in range(B):
        ref = orc.update(p, x0[b], xr[b], ft[b], ct[b], pcom_hor=pc[b] if use_pcom else None)
        ref["xs"] = orc.solve_reference(p, ref["qp"])[0] if ref["status"] == orc.STATUS_SOLVED else None
        refs.append(ref)
    _conditions([r["status"] for r in refs], [r["u"] for r in refs], ct, p)
    return refs


def _check64(group, out, b, ref, N, ct, p, x_tol=1e-5):
    """One QP of an fp64 solve against its twin and the exact optimum: the assertions of test_wrench_f64_matches_oracle_and_exact_optimum."""
    assert out["status"][b] == ref["status"] and ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER), (b, out["status"][b], ref["status"])
    assert abs(int(out["iters"][b]) - ref["iters"]) <= p.check_every, (b, out["iters"][b], ref["iters"])
    du, dx = np.abs(out["u"][b] - ref["u"]).max(), np.abs(out["x"][b] - ref["x"]).max()
    _note(group + " twin [N]", du, TOL_TWIN_N); _note(group + " roll-out", dx, x_tol)
    assert du <= TOL_TWIN_N, (b, du)
    assert dx <= x_tol, (b, dx)
    kq, vi, ri = orc.presolve(ref["qp"], ct[b])
    if ref["status"] == orc.STATUS_SOLVED:   # a QP that ends at the iteration cap (on the oracle too) is only held to its twin
        de = np.abs(out["u"][b].reshape(-1) - ref["xs"] * p.force_scale).max()
        _note(group + " exact [N]", de, TOL_EXACT_N)
        assert de <= TOL_EXACT_N, (b, de)
        if out.get("y") is not None:
            kr = orc.kkt_residuals(kq["P"], kq["q"], kq["A"], kq["l"], kq["u"], out["u"][b].reshape(-1)[vi] / p.force_scale, out["y"][b][ri])
            assert kr["primal"] <= 1e-4 and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(ref["qp"]["q"]).max()), kr
    off = np.setdiff1d(np.arange(12 * N), vi)
    assert np.all(out["u"][b].reshape(-1)[off] == 0.0)              # swing contacts carry exactly zero force
    if out.get("y") is not None:
        assert np.all(out["y"][b][np.setdiff1d(np.arange(20 * N), ri)] == 0.0)


# ---- a. assembly, entry by entry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yaw", sc.YAW_KINDS)
@pytest.mark.parametrize("kernel", ["compact", "wave"])
@pytest.mark.parametrize("N,schedule", [(10, "single"), (10, "double"), (10, "mixed"), (8, "single"), (8, "mixed"), (4, "double"), (4, "single"),
                                        (12, "single"), (16, "single"), (20, "single")])
def test_assembly_matches_oracle(torch_first, built_lib, N, schedule, kernel, yaw):
    """tests/test_gpu_parity.py::test_assembly_matches_oracle on turning inputs, with the CoM horizon taken from x_ref and given explicitly:
    P and q of the 4-wave and the one-wave kernel against the dense products B'QB + R, B'Q(A x0 - x_ref), entry by entry (an entry that is
    off names its step and contact: variable 12 k + 3 i + axis)."""
    from g1_locomotion_amd import _lib
    B = 4
    x0, xr, ft, ct, pc = _inputs(N, schedule, yaw, B)
    one_wave = kernel == "wave" and (schedule == "single" and N <= 10 or N == 4)     # <= 64 presolved variables, <= 4 x 4 tiles
    with _engine(N, kernel=_lib.KERNEL_WAVE if kernel == "wave" else _lib.KERNEL_COMPACT) as eng:
        got = {False: eng.assemble(x0, xr, ft, ct), True: eng.assemble(x0, xr, ft, ct, pcom=pc)}
        assert eng.kernel_name().startswith("wave_" if one_wave else "compact_"), eng.kernel_name()
    p = orc.params_for(N)
    grp = f"a. assembly {'one-wave' if one_wave else '4-wave'}"
    for use_pcom in (False, True):
        g = got[use_pcom]
        for b in range(B):
            qp = orc.build_qp(p, x0[b], xr[b], ft[b], ct[b], pcom_hor=pc[b] if use_pcom else None)
            red, vi, ri = orc.presolve(qp, ct[b])
            dP = np.abs(g["P"][b][np.ix_(vi, vi)] - red["P"])
            eP, eq = dP.max() / np.abs(red["P"]).max(), np.abs(g["q"][b][vi] - red["q"]).max() / max(1.0, np.abs(red["q"]).max())
            _note(grp + " P", eP, TOL_ASM); _note(grp + " q", eq, TOL_ASM)
            r, c = np.unravel_index(np.argmax(dP), dP.shape)
            assert eP <= TOL_ASM, (b, use_pcom, eP, "variables", int(vi[r]), int(vi[c]), "= step, contact", divmod(int(vi[r]) // 3, 4), divmod(int(vi[c]) // 3, 4))
            assert eq <= TOL_ASM, (b, use_pcom, eq, int(vi[np.argmax(np.abs(g["q"][b][vi] - red["q"]))]))
            off = np.setdiff1d(np.arange(12 * N), vi)
            assert np.all(g["P"][b][off, :] == 0.0) and np.all(g["P"][b][:, off] == 0.0) and np.all(g["q"][b][off] == 0.0)
            np.testing.assert_array_equal(g["l"][b], qp["l"])
            np.testing.assert_array_equal(g["u"][b], qp["u"])
    assert not np.array_equal(got[True]["P"], got[False]["P"])


WRENCH_ASM, B_ASM = [(4, "double"), (8, "mixed"), (10, "single"), (10, "double"), (10, "three"), (12, "mixed"), (16, "double"), (16, "single"),
                     (20, "double"), (20, "three"), (24, "mixed"), (24, "single")], 3


@pytest.mark.parametrize("yaw", sc.YAW_KINDS)
@pytest.mark.parametrize("N,schedule", WRENCH_ASM)
def test_wrench_assembly_matches_oracle(torch_first, built_lib, N, schedule, yaw):
    """tests/test_gpu_wrench.py::test_wrench_assembly_matches_oracle on turning inputs, CoM horizon from x_ref and explicit: T, V, Bd, q and the
    coordinate map of the general kernel against orc.wrench_reduce() at 1e-11, and the operator they define against the inverse of the dense
    K = B'QB + R + sigma I + A' rho A at 1e-8 -- the inverse refined in extended precision (scenarios.refined_inverse), its residual asserted."""
    from g1_locomotion_amd import _lib
    B = B_ASM
    x0, xr, ft, ct, pc = _inputs(N, schedule, yaw, B)
    with _engine(N, kernel=_lib.KERNEL_WRENCH) as eng:
        got = {False: eng.assemble_wrench(x0, xr, ft, ct), True: eng.assemble_wrench(x0, xr, ft, ct, pcom=pc)}
    p = orc.params_for(N)
    for use_pcom in (False, True):
        d = got[use_pcom]
        for b in range(B):
            pcom = pc[b] if use_pcom else None
            wr = orc.wrench_reduce(p, xr[b], ft[b], ct[b], pcom_hor=pcom)
            ng, vi, goff = wr["n_g"], wr["vi"], wr["goff"]
            np.testing.assert_array_equal(d["goff"][b], goff)
            T = d["T"][b]
            eT = np.abs(T[:ng, :ng] - wr["T"]).max() / np.abs(wr["T"]).max()
            assert eT <= TOL_ASM, (b, use_pcom, eT, np.unravel_index(np.argmax(np.abs(T[:ng, :ng] - wr["T"])), (ng, ng)), goff)
            assert np.all(T[ng:, :] == 0.0) and np.all(T[:, ng:] == 0.0)
            red, vi2, ri = orc.presolve(orc.build_qp(p, x0[b], xr[b], ft[b], ct[b], pcom_hor=pcom), ct[b])
            eq = np.abs(d["q"][b][vi] - red["q"]).max() / max(1.0, np.abs(red["q"]).max())
            assert eq <= TOL_ASM, (b, use_pcom, eq)
            off = np.setdiff1d(np.arange(12 * N), vi)
            assert np.all(d["q"][b][off] == 0.0) and np.all(d["Bd"][b][off] == 0.0) and np.all(d["Vcol"][b][off] == 0.0)
            nu = len(vi)
            V = np.zeros((ng, nu)); Bd = np.zeros((nu, nu))
            for idx, v in enumerate(vi):                      # V (n_g x n_u) and Bd (n_u x n_u) from the per-variable rows the lanes hold
                k = v // 12
                same = [i for i, vv in enumerate(vi) if vv // 12 == k]
                Bd[idx, same] = d["Bd"][b][v][[vi[i] % 12 for i in same]]
                V[goff[k]:goff[k + 1], idx] = d["Vcol"][b][v][:goff[k + 1] - goff[k]]
            eV = np.abs(V - wr["V"]).max() / np.abs(wr["V"]).max()
            eB = np.abs(Bd - wr["Bd"]).max() / max(np.abs(wr["Bd"]).max(), 1e-3)
            assert eV <= TOL_ASM and eB <= TOL_ASM, (b, use_pcom, eV, eB)
            for name, e in (("T", eT), ("q", eq), ("V", eV), ("Bd", eB)):
                _note("a. assembly general " + name, e, TOL_ASM)
            if b == 0:      # the operator these entries define, on one QP per variant (the extended-precision inverse is the slow part of this file)
                Kinv, res = sc.refined_inverse(sc.dense_k(p, red))
                Kw = Bd + V.T @ np.linalg.solve(T[:ng, :ng], V)
                eK = np.abs(Kw - Kinv).max() / np.abs(Kinv).max()
                _note("a. assembly general K^-1 operator", eK, TOL_KINV)
                assert eK <= TOL_KINV, (b, use_pcom, eK, res)
    assert not np.array_equal(got[True]["T"], got[False]["T"])


# ---- b. solve -------------------------------------------------------------------------------------------------------------------------------
PRESOLVED = [(10, "single"), (10, "double"), (10, "mixed"), (8, "mixed"), (8, "single"), (4, "single"), (4, "double")]
WRENCH = PRESOLVED[:3] + [(10, "three"), (8, "mixed"), (4, "double"), (12, "mixed"), (16, "double"), (20, "double"), (20, "mixed"), (20, "three"),
                          (24, "single"), (24, "mixed")]
B64 = 6


def _kinds(N):
    return sc.YAW_KINDS if N <= 10 else sc.YAW_KINDS[:2]        # "random" yaw: N <= 10 solves only (the oracle leaves too many longer ones at the cap)


@pytest.mark.parametrize("kernel", ["auto", "split", "wave"])
@pytest.mark.parametrize("N,schedule,yaw", [(N, s, y) for N, s in PRESOLVED for y in _kinds(N)])
def test_solve_matches_oracle_and_exact_optimum(torch_first, built_lib, kernel, N, schedule, yaw):
    """tests/test_gpu_parity.py::test_solve_matches_oracle_and_exact_optimum on turning inputs: the one-wave kernel, the split pipeline and the
    4-wave kernel (chosen by AUTO and forced).  More than 64 presolved variables: split and wave fall back to the 4-wave kernel, by name."""
    from g1_locomotion_amd import _lib
    kid = {"auto": _lib.KERNEL_AUTO, "split": _lib.KERNEL_SPLIT, "wave": _lib.KERNEL_WAVE}[kernel]
    x0, xr, ft, ct, pc = _inputs(N, schedule, yaw, B64)
    with _engine(N, kernel=kid) as eng:
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        small = schedule == "single" or N == 4                                       # <= 64 presolved variables
        want = {"auto": "wave_", "split": "split_", "wave": "wave_"}[kernel] if small else "compact_"
        assert eng.kernel_name().startswith(want), eng.kernel_name()
        name = eng.kernel_name().split("_")[0]
    refs = _twin64(N, schedule, yaw, B64)
    p = orc.params_for(N)
    for b in range(B64):
        _check64(f"b. solve {name}", out, b, refs[b], N, ct, p)


@pytest.mark.parametrize("N,schedule,yaw", [(N, s, y) for N, s in WRENCH for y in _kinds(N)])
def test_wrench_f64_matches_oracle_and_exact_optimum(torch_first, built_lib, N, schedule, yaw):
    from g1_locomotion_amd import _lib
    x0, xr, ft, ct, pc = _inputs(N, schedule, yaw, B64)
    use_pcom = schedule in ("mixed", "three")                   # these cases give the CoM horizon explicitly
    with _engine(N, kernel=_lib.KERNEL_WRENCH) as eng:
        out = eng.solve(x0, xr, ft, ct, pcom=pc if use_pcom else None, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}", eng.kernel_name()
    refs = _twin64(N, schedule, yaw, B64, use_pcom)
    p = orc.params_for(N)
    for b in range(B64):
        _check64("b. solve wrench_f64", out, b, refs[b], N, ct, p)


def _tile_inputs(N, schedule, yaw, B):
    """The contact patterns of tests/test_gpu_wrench.py::test_wrench_f32_tiles_match_twin_and_exact_optimum on turning footholds."""
    x0, xr, ft, ct, pc = _inputs(N, "double" if schedule == "three" else schedule, yaw, B)
    ct = ct.copy()
    if schedule == "three":                          # 3 or 4 stance contacts on every step
        rng = np.random.default_rng(N)
        for b in range(B):
            for k in range(N):
                if rng.random() < 0.5:
                    ct[b, k, rng.integers(0, 4)] = 0
    if schedule == "mixed":
        ct[::2] = 1                                  # every other QP in full double support: eligible for fp32 tiles
        ct[0, 3:5] = 0                               # ... one of them with a flight phase (0 contacts: still eligible)
    return x0, xr, ft, ct


@functools.lru_cache(maxsize=None)
def _twin32(N, schedule, yaw, B, tiles):
    x0, xr, ft, ct = _tile_inputs(N, schedule, yaw, B) if tiles else _inputs(N, schedule, yaw, B)[:4]
    p = orc.params_for(N, eps_abs=2e-6, eps_rel=2e-6)       # the fp32 path's tolerance floor
    refs = []
    for b in range(B):
        ref = orc.update_split(p, x0[b], xr[b], ft[b], ct[b], dtype=np.float32, **(dict(tile_dtype="auto") if tiles else {}))
        ref["xs"] = orc.solve_reference(p, ref["qp"])[0] if ref["status"] == orc.STATUS_SOLVED else None
        refs.append(ref)
    _conditions([r["status"] for r in refs], [r["u"] for r in refs], ct, p)
    return refs, p, ct


def _check32(group, out, b, ref, N, ct, p):
    """One QP of an fp32 solve: the assertions of tests/test_gpu_wrench.py's fp32 tests, with the fp64 rule for the status (equal to the twin's;
    the twin leaves some turning QPs at the cap) and the exact optimum for the solved ones."""
    assert out["status"][b] == ref["status"] and ref["status"] in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER), (b, out["status"][b], ref["status"], out["iters"][b], ref["iters"])
    assert abs(int(out["iters"][b]) - ref["iters"]) <= 2 * p.check_every, (b, out["iters"][b], ref["iters"])
    du, dx = np.abs(out["u"][b] - ref["u"]).max(), np.abs(out["x"][b] - ref["x"]).max()
    _note(group + " twin [N]", du, TOL32_TWIN_N); _note(group + " roll-out", dx, 1e-3)
    assert du <= TOL32_TWIN_N, (b, du)
    assert dx <= 1e-3, (b, dx)
    kq, vi, ri = orc.presolve(ref["qp"], ct[b])
    u64 = out["u"][b].reshape(-1).astype(np.float64)
    if ref["status"] == orc.STATUS_SOLVED:
        de = np.abs(u64 - ref["xs"] * p.force_scale).max()
        _note(group + " exact [N]", de, TOL32_EXACT_N)
        assert de <= TOL32_EXACT_N, (b, de)
        kr = orc.kkt_residuals(kq["P"], kq["q"], kq["A"], kq["l"], kq["u"], u64[vi] / p.force_scale, out["y"][b].astype(np.float64)[ri])
        assert kr["primal"] <= 1e-4 and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(ref["qp"]["q"]).max()), kr
    assert np.all(u64[np.setdiff1d(np.arange(12 * N), vi)] == 0.0)
    assert np.all(out["y"][b][np.setdiff1d(np.arange(20 * N), ri)] == 0.0)


@pytest.mark.parametrize("yaw", ["turn", "wrap"])
@pytest.mark.parametrize("N,schedule", [(20, "double"), (20, "mixed"), (10, "double"), (10, "single"), (16, "three"), (24, "mixed")])
def test_wrench_f32_matches_twin_and_exact_optimum(torch_first, built_lib, N, schedule, yaw):
    from g1_locomotion_amd import _lib
    B = 4
    x0, xr, ft, ct, pc = _inputs(N, schedule, yaw, B)
    with _engine(N, kernel=_lib.KERNEL_WRENCH) as eng:
        out = eng.solve(x0, xr, ft, ct, want_y=True, dtype=np.float32)
        assert eng.kernel_name() == f"wrench_f32_n{N}", eng.kernel_name()
    assert out["u"].dtype == np.float32 and out["x"].dtype == np.float32
    refs, p, _ = _twin32(N, schedule, yaw, B, False)
    for b in range(B):
        _check32("b. solve wrench_f32", out, b, refs[b], N, ct, p)


@pytest.mark.parametrize("yaw", ["turn", "wrap"])
@pytest.mark.parametrize("N,schedule", [(20, "double"), (24, "double"), (16, "three"), (12, "double"), (10, "double"), (8, "three"), (4, "double"), (20, "mixed")])
def test_wrench_f32_tiles_match_twin_and_exact_optimum(torch_first, built_lib, N, schedule, yaw):
    """SRBDQP_FLAG_F32_TILES: T factored in fp32 MFMA tiles, x_q refined once; against the twin with the same rule (tile_dtype="auto")."""
    from g1_locomotion_amd import _lib
    B = 4
    x0, xr, ft, ct = _tile_inputs(N, schedule, yaw, B)
    with _engine(N, kernel=_lib.KERNEL_WRENCH, flags=_lib.FLAG_F32_TILES) as eng:
        out = eng.solve(x0, xr, ft, ct, want_y=True, dtype=np.float32)
        assert eng.kernel_name() == f"wrench_f32_n{N}", eng.kernel_name()
    refs, p, ct2 = _twin32(N, schedule, yaw, B, True)
    assert np.array_equal(ct, ct2)
    for b in range(B):
        _check32("b. solve wrench_f32 tiles", out, b, refs[b], N, ct, p)
    n32 = sum(orc.fp32_tiles_ok(ct[b]) for b in range(B))
    assert n32 == (B if schedule != "mixed" else B // 2), n32          # the case exercises what its name says


# ---- c. the batch-1 paths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,schedule,suffix,yaw", [(10, "single", "compact_f64_n10_s2_lat", "turn"), (10, "single", "compact_f64_n10_s2_lat", "wrap"),
                                                   (8, "single", "compact_f64_n8_s2_lat", "wrap"), (4, "single", "compact_f64_n4_s2_lat", "random"),
                                                   (10, "double", "wrench_f64_n10_lat", "turn"), (10, "mixed", "wrench_f64_n10_lat", "wrap"),
                                                   (10, "mixed", "wrench_f64_n10_lat", "random"), (8, "double", "wrench_f64_n8_lat", "turn")])
def test_staged_batch1_low_latency_instantiations(torch_first, built_lib, N, schedule, suffix, yaw):
    """solve_staged(1) (what MPC.update() uses), one QP at a time: the 4-wave set-up + one-wave iteration kernel and the low-latency
    instantiation of the general kernel, each QP against the twin, the batch kernels and the same call with SRBDQP_FLAG_NO_LAT."""
    from g1_locomotion_amd import BatchMPC, _lib
    x0, xr, ft, ct, pc = _inputs(N, schedule, yaw, B64)
    refs = _twin64(N, schedule, yaw, B64)
    p = orc.params_for(N)
    with BatchMPC(horizon=N, rho_restart_iter=-1) as eng, BatchMPC(horizon=N, rho_restart_iter=-1, flags=_lib.FLAG_NO_LAT) as plain:
        batch = eng.solve(x0, xr, ft, ct)
        st, st2 = eng.stage(), plain.stage()
        for b in range(B64):
            for s_ in (st, st2):
                s_["x0"][0] = x0[b]; s_["x_ref"][0] = xr[b]; s_["foot"][0] = ft[b].reshape(N, 12); s_["contact"][0] = ct[b].reshape(N, 4)
            eng.solve_staged(1, want_x=True, want_y=True)
            plain.solve_staged(1, want_x=True)
            assert eng.kernel_name() == suffix, eng.kernel_name()
            assert not plain.kernel_name().endswith("_lat"), plain.kernel_name()
            one = dict(u=st["u"][:1], x=st["x"][:1], y=st["y"][:1], status=st["status"][:1], iters=st["iters"][:1])
            _check64("c. staged " + suffix.split("_")[0] + "_lat", one, 0, refs[b], N, ct[b:b + 1], p, x_tol=1e-4)
            assert int(st2["status"][0]) == refs[b]["status"] == int(batch["status"][b]) and abs(int(st2["iters"][0]) - refs[b]["iters"]) <= p.check_every
            assert np.abs(st["u"][0] - st2["u"][0]).max() <= TOL_TWIN_N and np.abs(st["u"][0] - batch["u"][b]).max() <= TOL_TWIN_N


@pytest.mark.parametrize("yaw,schedule", [("turn", "double"), ("wrap", "double"), ("wrap", "single"), ("random", "mixed")])
def test_mpc_update_drop_in_path(torch_first, built_lib, yaw, schedule):
    """MPC.update() with the reference caller's per-step lists (contact, footholds) and an explicit p_com_horizon, on turning inputs: every QP of
    the case through one MPC object, against the twin the engine's defaults have (orc.default_params: rho re-balanced every 55 iterations)."""
    from g1_locomotion_amd import mpc
    N = 10
    x0, xr, ft, ct, pc = _inputs(N, schedule, yaw, B64)
    p = orc.default_params(N)
    M = mpc.MPC(dt=0.04, strict=False)
    M.init_matrices()
    st, us = [], []
    try:
        for b in range(B64):
            ref = orc.update(p, x0[b], xr[b], ft[b], ct[b], pcom_hor=pc[b])
            st.append(ref["status"]); us.append(ref["u"])
            M.x_ref_hor[:] = xr[b]
            u0, xo = M.update([ct[b, k].copy() for k in range(N)], [ft[b, k].copy() for k in range(N)], pc[b].copy(), x_current=x0[b].reshape(13, 1), one_rollout=True)
            assert M.status == ref["status"] and abs(M.iters - ref["iters"]) <= p.check_every, (b, M.status, M.iters, ref["iters"])
            du, dx = np.abs(M.u_opt - ref["u"]).max(), np.abs(xo - ref["x"]).max()
            _note("c. MPC.update twin [N]", du, TOL_TWIN_N); _note("c. MPC.update roll-out", dx, 1e-5)
            assert du <= TOL_TWIN_N and dx <= 1e-5, (b, du, dx)
            assert np.array_equal(u0.reshape(-1), M.u_opt[0]) and np.array_equal(xo, M.x_opt)
    finally:
        M.close()
    _conditions(st, us, ct, p)


@pytest.mark.parametrize("N,schedule,yaw", [(10, "single", "turn"), (10, "single", "wrap"), (10, "single", "random"), (8, "single", "wrap"), (4, "double", "turn"),
                                            (4, "double", "random")])
def test_two_phase_call_equals_the_one_shot_call(torch_first, built_lib, N, schedule, yaw):
    """prepare_staged from a WRONG predicted state + solve_prepared from the measured one: the gradient patch dq/dx0 (x0 - x0_pred) contains the
    prefix sums C_k of the per-step Rz(yaw_k)', with and without an explicit CoM horizon; against the one-shot call and the twin."""
    from g1_locomotion_amd import BatchMPC
    B = B64
    x0, xr, ft, ct, pc = _inputs(N, schedule, yaw, B)
    rng = np.random.default_rng(N)
    p = orc.params_for(N)
    refs = _twin64(N, schedule, yaw, B)
    with BatchMPC(horizon=N, rho_restart_iter=-1) as eng:
        for use_pcom in (False, True):
            ref = eng.solve(x0, xr, ft, ct, pcom=pc if use_pcom else None)
            st = eng.stage()
            assert st["capacity"] >= B
            st["x_ref"][:B] = xr; st["foot"][:B] = ft.reshape(B, N, 12); st["contact"][:B] = ct.reshape(B, N, 4); st["pcom"][:B] = pc
            st["x0"][:B] = x0 + rng.normal(size=x0.shape) * np.array([0.2] * 3 + [0.05] * 3 + [0.5] * 6 + [0.0])     # the prediction: off
            eng.prepare_staged(B, use_pcom=use_pcom)
            assert eng.kernel_name().startswith("prepare_f64_n")
            st["x0"][:B] = x0                                                                                          # the measurement
            eng.solve_prepared(B, want_x=True)
            assert eng.kernel_name().startswith("prepared_f64_n")
            u, x, status, iters = st["u"][:B].copy(), st["x"][:B].copy(), st["status"][:B].copy(), st["iters"][:B].copy()
            np.testing.assert_array_equal(status, ref["status"])
            assert np.abs(iters - ref["iters"]).max() <= 5, (iters, ref["iters"])
            du, dx = np.abs(u - ref["u"]).max(), np.abs(x - ref["x"]).max()
            _note("c. two-phase vs one-shot [N]", du, 1e-6); _note("c. two-phase vs one-shot roll-out", dx, 1e-8)
            assert du <= 1e-6 and dx <= 1e-8, (use_pcom, du, dx)
            if not use_pcom:
                for b in range(B):
                    assert status[b] == refs[b]["status"] and np.abs(u[b] - refs[b]["u"]).max() <= TOL_TWIN_N


# ---- d. at scale against the C oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yaw", ["turn", "wrap"])
@pytest.mark.parametrize("N,schedule,B", [(10, "single", 1024), (10, "mixed", 1024), (8, "mixed", 1024), (16, "single", 1024), (20, "double", 1024)])
def test_large_batch_against_c_oracle(torch_first, built_lib, N, schedule, B, yaw):
    """Every QP of a large turning batch against the compiled oracle, the engine with its default rho restart and the oracle with the same rule
    (orc.default_params): statuses equal, iteration counts within one check for EVERY QP, forces within the twin bound for every QP and within
    1e-4 N where the counts are equal.  (No bound on the share of equal counts: the one of the older tests was measured on other inputs.)"""
    import c_oracle
    from g1_locomotion_amd import BatchMPC
    x0, xr, ft, ct = sc.turning_batch(B, N, _seed(N, schedule, yaw) + 1, schedule, yaw=yaw)
    p = orc.default_params(N)
    ref = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=8)
    _conditions(ref["status"], ref["u"], ct, p)
    with BatchMPC(horizon=N) as eng:
        out = eng.solve(x0, xr, ft, ct)
        assert eng.kernel_name().startswith(("compact_", "wave_", "wrench_")), eng.kernel_name()
        name = eng.kernel_name().split("_")[0]
    np.testing.assert_array_equal(out["status"], ref["status"])
    assert np.abs(out["iters"].astype(int) - ref["iters"].astype(int)).max() <= p.check_every
    same = out["iters"] == ref["iters"]
    err = np.abs(out["u"] - ref["u"]).reshape(B, -1).max(1)
    print(f"N={N} {schedule} {yaw} {name}: equal iteration counts {same.mean():.4f}, solved {(ref['status'] == 1).mean():.4f}, err same {err[same].max():.2e} all {err.max():.2e}")
    _note(f"d. scale {name} equal counts [N]", err[same].max(), 1e-4); _note(f"d. scale {name} all [N]", err.max(), TOL_TWIN_N)
    assert err[same].max() <= 1e-4 and err.max() <= TOL_TWIN_N, (err[same].max(), err.max())
    assert np.all(out["u"].reshape(B, N, 4, 3)[ct == 0] == 0.0)
    # Roll-out.  The states are linear in the forces, x = A_qp x0 + B_qp u, and with the torso's small yaw inertia |B_qp|_inf reaches 70 - 210 per newton
    # on these inputs (N = 10 ... 20), so forces that agree with the C oracle's to 6e-6 N may leave states 1e-3 apart (2.6e-5 seen at N = 20): a fixed
    # state bound does not follow from the force bound.  Held instead, on the QP whose states differ most and on the first 15: the kernel's roll-out
    # against the dense model applied to the kernel's OWN forces at 1e-8 (<= 240 terms, sum of magnitudes <= 210 x 300 N, 1.1e-16 each: 1.6e-9), and
    # against the C oracle's states at what the force difference of that QP allows.
    dxq = np.abs(out["x"] - ref["x"]).reshape(B, -1).max(1)
    for b in sorted(set(range(15)) | {int(np.argmax(dxq))}):
        qp = orc.build_qp(p, x0[b], xr[b], ft[b], ct[b])
        own = np.abs(out["x"][b] - orc.rollout(qp, x0[b], out["u"][b].reshape(-1) / p.force_scale, p.force_scale)).max()
        _note(f"d. scale {name} roll-out vs own forces", own, 1e-8)
        assert own <= 1e-8, (b, own)
        assert dxq[b] <= np.abs(qp["B_qp"]).sum(1).max() * err[b] + 1e-8, (b, dxq[b], err[b])


# ---- e. ragged fleets and per-QP robot records ------------------------------------------------------------------------------------------------
def test_ragged_horizons_bucketed_launch(torch_first, built_lib):
    """One ragged fleet, horizons 8 / 12 / 16 / 24, yaw kinds turn / wrap and every schedule mixed across the buckets: every QP against its twin
    and, where solved, the exact optimum, in the caller's order."""
    from g1_locomotion_amd import RaggedMPC
    rng = np.random.default_rng(5)
    problems = []
    for i in range(32):
        N = int(rng.choice([8, 12, 16, 24]))
        x0, xr, ft, ct = (a[0] for a in sc.turning_batch(1, N, 9900 + i, str(rng.choice(["single", "mixed", "double"])), yaw=("turn", "wrap")[i % 2]))
        problems.append(dict(x0=x0, x_ref=xr, foot=ft, contact=ct))
    eng = RaggedMPC(horizons=(8, 12, 16, 24), rho_restart_iter=-1)
    try:
        res = eng.solve(problems)
    finally:
        eng.close()
    st, us, cts = [], [], []
    for pr, r in zip(problems, res):
        N = pr["x_ref"].shape[0]
        p = orc.params_for(N)
        ref = orc.update(p, pr["x0"], pr["x_ref"], pr["foot"], pr["contact"])
        st.append(ref["status"]); us.append(ref["u"]); cts.append(pr["contact"])
        assert r["status"] == ref["status"] and abs(r["iters"] - ref["iters"]) <= p.check_every
        du, dx = np.abs(r["u"] - ref["u"]).max(), np.abs(r["x"] - ref["x"]).max()
        _note("e. ragged twin [N]", du, TOL_TWIN_N); _note("e. ragged roll-out", dx, 1e-5)
        assert r["u"].shape == pr["foot"].shape and du <= TOL_TWIN_N, (N, du)
        assert r["x"].shape == (N + 1, 13) and dx <= 1e-5
        if ref["status"] == orc.STATUS_SOLVED:
            xs, _ = orc.solve_reference(p, ref["qp"])
            de = np.abs(r["u"].reshape(-1) - xs * p.force_scale).max()
            _note("e. ragged exact [N]", de, TOL_EXACT_N)
            assert de <= TOL_EXACT_N, (N, de)
    _conditions(st, us, cts, orc.params_for(8))


@pytest.mark.parametrize("N,schedule,yaw", [(12, "mixed", "wrap"), (20, "three", "turn")])
def test_per_qp_records_match_the_oracle(torch_first, built_lib, N, schedule, yaw):
    """set_robots() (the general kernel's MODE = 2 instantiation) on turning inputs, through tests/side_inputs.py check_qp: per QP against
    the oracle with THAT QP's mass, inertia, mu and fz bounds; engine and oracle with the default rho restart."""
    from g1_locomotion_amd import BatchMPC
    import side_inputs as si
    B = 8
    x0, xr, ft, ct, pc = _inputs(N, schedule, yaw, B)
    rec = si.draw_robots(B, 2900 + N)
    with BatchMPC(horizon=N) as eng:
        out0 = eng.solve(x0, xr, ft, ct)
        eng.set_robots(rec)
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}_rb", eng.kernel_name()
    moved = 0
    for b in range(B):
        p = si.params(N, robot=rec[b])
        si.check_qp(out, b, N, p, si.twin(p, x0[b], xr[b], ft[b], ct[b]), ct[b])
        moved += int(np.abs(out["u"][b] - out0["u"][b]).max() > 1.0)
    assert moved >= B // 4, moved


# ---- f. non-default constants on the general kernel -------------------------------------------------------------------------------------------
KW = dict(dt=0.03, mass=41.0, inertia=(0.11, 0.09, 0.006), mu=0.55, fz_min=5.0, fz_max=420.0,
          q_diag=(250.0, 320.0, 120.0, 380.0, 410.0, 700.0, 2.0, 1.5, 1.0, 15.0, 25.0, 30.0, 0.0), r_diag=3.0e-4,
          force_scale=60.0, rho=0.8, alpha=1.5, sigma=2.0e-6, eps_abs=2.0e-6, eps_rel=2.0e-6, max_iter=180, check_every=4)   # tests/test_gpu_parity.py


def _vs_c_oracle(group, out, ref, p):
    """The bounds of tests/test_gpu_parity.py::test_non_default_constants_reach_every_kernel (its share of equal iteration counts was measured on
    other inputs and is not carried over)."""
    np.testing.assert_array_equal(out["status"], ref["status"])
    assert np.abs(out["iters"].astype(int) - ref["iters"].astype(int)).max() <= p.check_every
    same = out["iters"] == ref["iters"]
    err = np.abs(out["u"] - ref["u"]).reshape(len(same), -1).max(1)
    dx = np.abs(out["x"] - ref["x"]).max()
    _note(group + " equal counts [N]", err[same].max(), 1e-3); _note(group + " all [N]", err.max(), 5 * TOL_TWIN_N); _note(group + " roll-out", dx, 1e-4)
    assert err[same].max() <= 1e-3 and err.max() <= 5 * TOL_TWIN_N, (err[same].max(), err.max())
    assert dx <= 1e-4


@pytest.mark.parametrize("N,schedule,yaw", [(10, "double", "turn"), (12, "mixed", "wrap"), (20, "double", "turn")])
def test_non_default_constants_reach_the_general_kernel(torch_first, built_lib, N, schedule, yaw):
    """Another dt, mass, inertia, friction, force bounds, weights, scaling and ADMM parameters on the general kernel: fp64 against the C oracle,
    fp32 against the fp32 twin, both with the same values.  First, on the oracle alone: the changed constants move the forces by more than 1 N,
    so a constant the kernel ignored could not pass."""
    import c_oracle
    from g1_locomotion_amd import _lib
    B, B32 = 128, 4
    x0, xr, ft, ct = sc.turning_batch(B, N, _seed(N, schedule, yaw) + 2, schedule, yaw=yaw, dt=KW["dt"])
    p = orc.SrbdParams(**KW)
    ref = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=8)
    ref0 = c_oracle.solve_batch(orc.params_for(N, dt=KW["dt"]), x0, xr, ft, ct, nthreads=8)
    assert np.median(np.abs(ref["u"] - ref0["u"]).reshape(B, -1).max(1)) > 1.0          # the constants matter
    _conditions(ref["status"], ref["u"], ct, p)
    with _engine(N, kernel=_lib.KERNEL_WRENCH, **KW) as eng:
        out = eng.solve(x0, xr, ft, ct)
        assert eng.kernel_name() == f"wrench_f64_n{N}", eng.kernel_name()
        out32 = eng.solve(x0[:B32], xr[:B32], ft[:B32], ct[:B32], want_y=True, dtype=np.float32)
        assert eng.kernel_name() == f"wrench_f32_n{N}", eng.kernel_name()
    _vs_c_oracle("f. constants wrench_f64", out, ref, p)
    for b in range(B32):
        r32 = orc.update_split(p, x0[b], xr[b], ft[b], ct[b], dtype=np.float32)
        r32["xs"] = orc.solve_reference(p, r32["qp"])[0] if r32["status"] == orc.STATUS_SOLVED else None
        _check32("f. constants wrench_f32", out32, b, r32, N, ct, p)


ZERO_ANGLES = (0.0, 0.0, 0.0) + orc.SrbdParams().q_diag[3:]
ZERO_OMEGA = orc.SrbdParams().q_diag[:6] + (0.0, 0.0, 0.0) + orc.SrbdParams().q_diag[9:]


@pytest.mark.parametrize("kernel,schedule", [("wave", "single"), ("compact", "single"), ("wrench", "mixed")])
@pytest.mark.parametrize("what,kw", [("angles", dict(q_diag=ZERO_ANGLES)), ("omega", dict(q_diag=ZERO_OMEGA)), ("rho_fz_scale", dict(rho_fz_scale=1.0))])
def test_zeroed_weight_groups_and_penalty_ratio_reach_every_kernel(torch_first, built_lib, kernel, schedule, what, kw):
    """N = 10 on the one-wave, the 4-wave and the general kernel: the weights of a whole group of states set to 0 (Euler angles; angular
    velocity), and rho_fz_scale = 1 given explicitly, against the C oracle with the same values.  First, on the oracle alone: a zeroed group
    moves the forces by more than 1 N (median over the batch: 4 N angles, 40 N angular velocity); rho_fz_scale only steers the ADMM, so there the
    assertion is on the oracle's iteration counts.
    rho_eq_scale is left out: the presolved QP has no equality row, and the oracle's result does not depend on it at all (asserted here)."""
    import c_oracle
    from g1_locomotion_amd import _lib
    N, B = 10, 256
    x0, xr, ft, ct = sc.turning_batch(B, N, 7700, schedule, yaw="turn")
    p = orc.params_for(N, **kw)
    ref = c_oracle.solve_batch(p, x0, xr, ft, ct, nthreads=8)
    ref0 = c_oracle.solve_batch(orc.params_for(N), x0, xr, ft, ct, nthreads=8)
    if what == "rho_fz_scale":
        # (iteration counts are multiples of check_every, so many coincide: they differ for 35 % / 46 % of these QPs, and for 28 % / 37 % by MORE
        #  than one check interval -- each of those alone fails the comparison below if the kernel ran the default ratio; at least 1 in 10 is asked)
        assert (np.abs(ref["iters"].astype(int) - ref0["iters"].astype(int)) > p.check_every).mean() >= 0.1
        req = c_oracle.solve_batch(orc.params_for(N, rho_eq_scale=10.0, **kw), x0, xr, ft, ct, nthreads=8)
        assert np.array_equal(req["u"], ref["u"]) and np.array_equal(req["iters"], ref["iters"])
    else:
        assert np.median(np.abs(ref["u"] - ref0["u"]).reshape(B, -1).max(1)) > 1.0
    _conditions(ref["status"], ref["u"], ct, p)
    kid = {"wave": _lib.KERNEL_AUTO, "compact": _lib.KERNEL_COMPACT, "wrench": _lib.KERNEL_WRENCH}[kernel]
    with _engine(N, kernel=kid, max_contacts_per_step=2 if schedule == "single" else 4, **kw) as eng:
        out = eng.solve(x0, xr, ft, ct)
        assert eng.kernel_name().startswith(kernel + "_"), eng.kernel_name()
    _vs_c_oracle(f"f. {what} {kernel}", out, ref, p)


# ---- frozen numbers ---------------------------------------------------------------------------------------------------------------------------
GOLDEN = [(name, N, path) for name, N in [("n10_turn_single", 10), ("n10_wrap_mixed", 10), ("n10_turn_double", 10), ("n8_wrap_mixed", 8), ("n4_random_double", 4)]
          for path in ("staged", "batch", "wave", "wrench")] + [("n20_turn_double", 20, "wrench")]


@pytest.mark.parametrize("name,N,path", GOLDEN)
def test_committed_turning_fixtures_gate_the_kernels(torch_first, built_lib, name, N, path):
    """tests/golden/srbd_turning_golden.npz (made by tests/golden/make_turning_golden.py) through the HIP path itself, as
    tests/test_gpu_parity.py::test_committed_golden_fixtures_gate_the_kernels runs the constant-yaw file: the staged batch-1 call (MPC.update), the
    4-wave kernel, the one-wave kernel (more than 64 presolved variables: its documented fall-back, by name) and the general kernel; forces
    against the frozen exact optimum and the frozen twin, KKT residuals of the returned pair.  Numbers that do not move when the oracle is edited."""
    from g1_locomotion_amd import _lib, mpc
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "srbd_turning_golden.npz"))
    x0, xr, ft, ct = (gold[f"{name}/{k}"] for k in ("x0", "x_ref", "foot", "contact"))
    u_exact, u_admm, it_admm = gold[f"{name}/u_exact"], gold[f"{name}/u_admm"], int(gold[f"{name}/iters_admm"])
    p = orc.SrbdParams()
    if path == "staged":
        assert it_admm < 55                  # below the first mark of the default rho restart: MPC()'s defaults run the frozen twin's iterates
        M = mpc.MPC(dt=0.04, horizon=N, strict=False)
        M.init_matrices()
        M.x_ref_hor[:] = xr
        u0, xo = M.update(list(ct), list(ft), xr[:, 3:6].copy(), x_current=x0.reshape(13, 1))
        u, x, status, iters, y = M.u_opt, M.x_opt, M.status, M.iters, None
        assert np.array_equal(u0.reshape(-1), u[0]) and np.array_equal(xo, x)
        M.close()
    else:
        kid = {"batch": _lib.KERNEL_COMPACT, "wave": _lib.KERNEL_WAVE, "wrench": _lib.KERNEL_WRENCH}[path]
        small = N == 4 or int(ct.sum(1).max()) <= 2             # the one-wave kernel's instantiations: <= 64 presolved variables
        with _engine(N, kernel=kid) as eng:
            out = eng.solve(x0[None], xr[None], ft[None], ct[None], want_y=True)
            assert eng.kernel_name().startswith({"batch": "compact_", "wave": "wave_" if small else "compact_", "wrench": "wrench_"}[path]), eng.kernel_name()
        u, x, status, iters, y = out["u"][0], out["x"][0], int(out["status"][0]), int(out["iters"][0]), out["y"][0]
    assert status == orc.STATUS_SOLVED
    assert abs(iters - it_admm) <= p.check_every, (iters, it_admm)
    du, de, dx = np.abs(u - u_admm).max(), np.abs(u - u_exact).max(), np.abs(x - gold[f"{name}/x_exact"]).max()
    _note("golden twin [N]", du, TOL_TWIN_N); _note("golden exact [N]", de, TOL_EXACT_N); _note("golden roll-out vs exact", dx, 1e-4)
    assert du <= TOL_TWIN_N and de <= TOL_EXACT_N and dx <= 1e-4, (du, de, dx)
    if y is not None:
        qp = orc.build_qp(p, x0, xr, ft, ct)
        red, vi, ri = orc.presolve(qp, ct)
        kr = orc.kkt_residuals(red["P"], red["q"], red["A"], red["l"], red["u"], u.reshape(-1)[vi] / p.force_scale, y[ri])
        assert kr["primal"] <= 1e-4 and kr["stationarity"] <= 1e-3 * max(1.0, np.abs(qp["q"]).max()), kr
