"""The oracle holds the QP's symmetries (tests/symmetries.py) on every case the GPU suite (tests/test_gpu_symmetries.py) runs: orc.update, orc.solve_reference
and tests/side_inputs.py::twin under an external wrench and under contact normals.  No GPU.

This file is the reference's half of the pair bar: the deviations printed here (-s) are the D of pair_bar(N) = 100 D_N.  It also decides which
transformations are symmetries of the two side inputs: one enters the GPU table for a side input only if the twin holds it here.

TWIN_BAR_N.  The transformed scene's QP data differ from the base scene's by rounding alone -- relative 1.1e-16 for the rotation, the mirror and the
permutations (other summation orders), and 1000 m x 2.2e-16 = 2.2e-13 m on lever arms of ~0.1 m for the shift --, and the ADMM's iterates carry such a
perturbation amplified by at most cond(K) <= 2e8 (tests/scenarios.py::refined_inverse): 2.2e-12 x 2e8 x 1e-2 (a lever-arm error moves a 300 N force by
its relative size times the share of the moment in the cost, under 1 %) ~ 4e-6 N at worst.  1e-5 N is asked: a decade under the 1e-4 N that a convention
error may be as small as, two under the suites' 2e-3 N.  Measured: <= 9.3e-7 N (the restarted twin under a wrench at N = 10), <= 5e-7 N elsewhere,
<= 8e-8 N at N <= 10 without a side input.  Status and iteration count must be IDENTICAL in every pair."""
import numpy as np
import pytest

import side_inputs as si
import srbd_oracle as orc
import symmetries as sy

TWIN_BAR_N = 1e-5
BROKEN_N = 1e-3         # a transformation that is NO symmetry of a side input moves the twin's forces by more than this on some scene of the case


@pytest.mark.parametrize("path,N,schedule,yaw,B", sy.CASES)
def test_the_twin_holds_every_transformation(path, N, schedule, yaw, B):
    """orc.update (side inputs: side_inputs.twin) of the transformed scene = the transformed result of the base scene: forces, states, status, iterations."""
    dev = sy.twin_deviation(path, N, schedule, yaw, B)
    assert [n for n, _ in sy.transforms_of(path)] == list(dev)
    print(f"\nD {path} N={N} {schedule} {yaw}: " + ", ".join(f"{n} |du| {v[0]:.1e} N |dx| {v[1]:.1e}" for n, v in dev.items()))
    for name, (du, dx, same_status, same_iters) in dev.items():
        assert same_status and same_iters, (name, [(r["status"], r["iters"]) for r in sy.twins(path, N, schedule, yaw, B)])
        assert du <= TWIN_BAR_N and dx <= TWIN_BAR_N, (name, du, dx)
    ref = sy.twins(path, N, schedule, yaw, B)
    assert sum(r["status"] == orc.STATUS_SOLVED for r in ref[:B]) >= (3 * B) // 4, [r["status"] for r in ref[:B]]       # the case is about solved QPs
    if path == "wave_restart":      # the case must exercise the second pass: past the first mark, SOLVED, and another answer than the twin without the restart gives
        assert sy.restarted(ref, B) >= sy.RESTARTED_MIN, [r["iters"] for r in ref[:B]]
        x0, xr, ft, ct, pc, _, _ = sy.stacked(path, N, schedule, yaw, B)
        plain = [orc.update(orc.params_for(N), x0[b], xr[b], ft[b], ct[b], pcom_hor=pc[b]) for b in range(B)]
        moved = [b for b in range(B) if not np.array_equal(ref[b]["u"], plain[b]["u"])]
        print(f"restarted scenes: iterations {[ref[b]['iters'] for b in moved]} with the restart, {[plain[b]['iters'] for b in moved]} without")
        assert len(moved) >= sy.RESTARTED_MIN, moved


@pytest.mark.parametrize("path,N,schedule,yaw,B", [c for c in sy.CASES if c[0] not in sy.SIDE_OF and not c[0].startswith("staged")])
def test_the_exact_optimum_holds_every_transformation(path, N, schedule, yaw, B):
    """orc.solve_reference -- an active-set solve that shares no iteration with the ADMM -- of the transformed QP = the transformed optimum."""
    x0, xr, ft, ct, pc, _, backs = sy.stacked(path, N, schedule, yaw, B)
    p = sy.twin_params(path, N)
    xs = [orc.solve_reference(p, orc.build_qp(p, x0[b], xr[b], ft[b], ct[b], pc[b]))[0].reshape(N, 12) * p.force_scale for b in range(len(x0))]
    for j, (name, back) in enumerate(backs):
        du = max(np.abs(back(xs[(j + 1) * B + b])[0] - xs[b]).max() for b in range(B))
        print(f"exact optimum {path} N={N} {name}: {du:.1e} N")
        assert du <= TWIN_BAR_N, (name, du)


@pytest.mark.parametrize("path", ["ew", "cn"])
def test_which_transformations_the_side_inputs_keep(path):
    """All five on the twin under the side input, whether transforms_of() lists them or not: one the twin holds must be listed (the GPU suite would
    otherwise leave it out unnoticed), and one it breaks must not be.  The wrench keeps all five.  Tilted normals do not keep rot90: contact_frames picks
    the tangent axes by a world-axis rule, so the pyramid's edges do not turn with the world."""
    _, N, schedule, yaw, B = next(c for c in sy.CASES if c[0] == path)
    base, side, p = sy.scenes(N, schedule, yaw, B), sy.side_input(path, N, B), sy.twin_params(path, N)
    kind = sy.SIDE_OF[path]
    solve = lambda s, v, b: si.twin(p, s[0][b], s[1][b], s[2][b], s[3][b], pcom=s[4][b], **{kind: v[b]})
    r0 = [solve(base, side, b) for b in range(B)]
    held = []
    for name in sy.NAMES:
        *img, back = sy.TRANSFORMS[name](*base)
        r1 = [solve(img, sy.side_image(name, kind, side), b) for b in range(B)]
        du = max(np.abs(back(r1[b]["u"])[0] - r0[b]["u"]).max() for b in range(B))
        print(f"{path} {name}: {du:.1e} N")
        assert du <= TWIN_BAR_N or du >= BROKEN_N, (name, du)             # held or broken, nothing in between
        if du <= TWIN_BAR_N:
            held.append(name)
    assert held == [n for n, _ in sy.transforms_of(path)], held
    assert (path == "cn") == ("rot90" not in held)


def test_a_neutral_side_input_changes_nothing():
    """The side-input twin with a zero wrench is the plain twin bit for bit on an image too (so the "ew" bars rest on the same arithmetic)."""
    N, B = 10, 2
    base = sy.scenes(N, "mixed", "turn", 6)
    *img, back = sy.mirror(*base)
    p = orc.default_params(N)
    for b in range(B):
        a = si.twin(p, img[0][b], img[1][b], img[2][b], img[3][b], pcom=img[4][b], ext_wrench=np.zeros((N, 6)))
        c = orc.update(p, img[0][b], img[1][b], img[2][b], img[3][b], pcom_hor=img[4][b])
        assert np.array_equal(a["u"], c["u"]) and a["iters"] == c["iters"]


@pytest.mark.parametrize("name", sy.NAMES)
def test_back_inverts_the_transformation(name):
    """back() of a transformed state and of forces moved like the contact points gives the originals (to rounding: yaw + pi/2 - pi/2, p + 1000 - 1000)."""
    N, B = 8, 3
    x0, xr, ft, ct, pc = sy.scenes(N, "mixed", "random", 6)
    x0, xr, ft, ct, pc = x0[:B], xr[:B], ft[:B], ct[:B], pc[:B]
    x = np.concatenate([x0[:, None], xr], axis=1)
    t0, tr, tf, tc, tp, back = sy.TRANSFORMS[name](x0, xr, ft, ct, pc)
    u = ft                                                           # the foot points stand in for forces: they move the same way, but for the shift
    tu = tf - (np.tile(sy.SHIFT, 4) if name == "shift" else 0.0)
    bu, bx = back(tu, np.concatenate([t0[:, None], tr], axis=1))
    assert np.abs(bu - u).max() <= 1e-12 and np.abs(bx - x).max() <= 1e-12
    assert tc.sum() == ct.sum() and tc.dtype == ct.dtype
    if name == "rot90":
        assert np.abs(tr[..., 2]).max() > np.pi                      # a yaw outside (-pi, pi] is part of the test: not re-wrapped


def test_the_bars_have_teeth():
    """A convention error in the transformation -- the sign of one mirrored torque component dropped, one x/y swapped in rot90 -- is newtons away from the twin's
    bar: what the pair bar separates is far apart."""
    N, B = 10, 6
    base, w, p = sy.scenes(N, "mixed", "turn", B), sy.side_input("ew", N, B), orc.default_params(N)
    b = 0
    r0 = si.twin(p, *(a[b] for a in base[:4]), pcom=base[4][b], ext_wrench=w[b])
    *img, back = sy.mirror(*base)
    wrong = sy.side_image("mirror", "ext_wrench", w)
    wrong[..., 0] *= -1.0                                            # tau_x keeps its sign: a polar-vector mirror of an axial vector
    r1 = si.twin(p, *(a[b] for a in img[:4]), pcom=img[4][b], ext_wrench=wrong[b])
    assert np.abs(back(r1["u"])[0] - r0["u"]).max() >= 1e3 * TWIN_BAR_N
    *img, back = sy.rot90(*base)
    img[4] = img[4].copy()
    img[4][..., 0], img[4][..., 1] = base[4][..., 1], base[4][..., 0]        # pcom: (y, x) in the place of (-y, x)
    r2 = orc.update(orc.params_for(N), *(a[b] for a in img[:4]), pcom_hor=img[4][b])
    r3 = orc.update(orc.params_for(N), *(a[b] for a in base[:4]), pcom_hor=base[4][b])
    assert np.abs(back(r2["u"])[0] - r3["u"]).max() >= 1e3 * TWIN_BAR_N


@pytest.mark.parametrize("path,N,schedule,yaw,B", sy.F32_CASES)
def test_the_float32_twin_meets_the_fp32_bars_on_every_image(path, N, schedule, yaw, B):
    """What the GPU suite asks of the fp32 kernels, asked of the float32 twin first, 1000 m from the origin included (the inputs rounded to float32 after
    the transformation): status SOLVED at least two check intervals under the cap, forces within TOL32_EXACT_N = 1e-1 N of the exact optimum of the rounded
    QP, states within 1e-3 of that optimum's roll-out."""
    refs, p = sy.twins32(path, N, schedule, yaw, B)
    names = ["base"] + [n for n, _ in sy.transforms_of(path, f32=True)]
    x0s, worst = sy.rounded(sy.stacked(path, N, schedule, yaw, B, f32=True)[0]), {}
    for b, ref in enumerate(refs):
        assert ref["status"] == orc.STATUS_SOLVED and ref["iters"] <= p.max_iter - 2 * p.check_every, (names[b // B], b % B, ref["status"], ref["iters"])
        de = np.abs(ref["u"].reshape(-1) - ref["xs"] * p.force_scale).max()
        dx = np.abs(ref["x"] - orc.rollout(ref["qp"], x0s[b], ref["xs"], p.force_scale)).max()
        w = worst.setdefault(names[b // B], [0.0, 0.0])
        w[:] = max(w[0], de), max(w[1], dx)
        assert de <= 1e-1 and dx <= 1e-3, (names[b // B], b % B, de, dx)
    print("\n" + "\n".join(f"f32 twin {path} N={N} {n}: exact {v[0]:.1e} N, x {v[1]:.1e}" for n, v in worst.items()))


def test_pair_bar_is_a_hundred_times_the_twins_own_deviation():
    for N in sorted({c[1] for c in sy.CASES}):
        d = sy.twin_d(N)
        print(f"D_{N} = {d:.2e}  pair_bar = {sy.pair_bar(N):.2e}" + (f"   under a wrench: D = {sy.twin_d(N, 'ext_wrench'):.2e}, on contact frames: D = {sy.twin_d(N, 'normals'):.2e}" if N == 10 else ""))
        assert 0.0 < d <= TWIN_BAR_N and sy.pair_bar(N) == 100.0 * d
        assert sy.pair_bar(N) <= 0.5 * si.TOL_TWIN_N                  # the pair bar is the sharper one at every horizon
