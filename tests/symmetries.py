"""The exact symmetries of the SRBD QP -- TEST INFRASTRUCTURE ONLY (plain module, imported by tests/test_symmetries_cpu.py and tests/test_gpu_symmetries.py).

Each transformation maps a scene (x0, x_ref, foot, contact, pcom) to OTHER input numbers whose solution is known exactly from the base scene's: the
forces transform like the contact points.  A solver compared with ITSELF across such a pair needs no twin arithmetic, so a convention the kernel and its
twin share (an x/y mix-up, a heel/toe asymmetry, a sign that only shows at negative yaw, a cancellation far from the origin) cannot hide in it.

State layout [roll, pitch, yaw, p (3), omega (3), v (3), g]; contacts 0, 1 = left heel, toe, 2, 3 = right heel, toe.
  rot90     the world turned +90 deg about z: (x, y) -> (-y, x) on p, omega, v, the foot points, pcom and the forces; yaw + pi/2 on x0 and every row of
            x_ref, NOT re-wrapped (both sides of the yaw error move together; a yaw outside (-pi, pi] is part of the test).  Roll and pitch stay: their rates
            are Rz(yaw)' omega, and yaw and omega turn together.  Exact because q_diag weighs x and y alike and the friction pyramid is square.
  mirror    y -> -y: the state times S13, points, pcom and forces times (1, -1, 1), contact columns and foot points permuted [2, 3, 0, 1].  At any yaw.
  relabel   heel <-> toe within each foot: [1, 0, 3, 2] on foot points, contact flags and forces.
  swapfeet  [2, 3, 0, 1] without the mirror: the stance pair moves to the other lanes of the one-wave and the 4-wave kernel.
  shift     + SHIFT metres on x0[3:6], x_ref[:, 3:6], every foot point and pcom; the forces are unchanged, the CoM rows of x come back shifted.
Rotations other than multiples of 90 deg are no symmetry (the pyramid is not invariant under them).

Every function takes arrays with any leading axes (one QP or a batch) and returns the five transformed arrays and `back`: back(u, x) maps the forces
u (..., N, 12) and the states x (..., N + 1, 13) of the TRANSFORMED scene into the base scene's frame and labels (x may be None).  side_image() does the
same for the two side inputs that live in the world frame: the external wrench [tau (3), f (3)] -- force like a vector, torque like a vector under rot90
and with (-1, 1, -1) under mirror (an axial vector) -- and the contact normals (vectors, permuted with the contacts).

Bars (tests/test_gpu_symmetries.py).  D_N is the largest deviation the fp64 TWIN shows between orc.update(T scene) and T(orc.update(scene)) over all fp64
cases of horizon N in CASES and all five transformations, computed inside the test run (twin_deviation), never a constant: the twin's LAPACK calls round
differently from host to host.  The cases under a side input have a D of their own (twin_d says why).  pair_bar(N) = 100 D_N holds a kernel's pair whose two
runs stop at the same iteration.  Two decades: the kernels form K^-1 explicitly in tile inversions and sum in lane order where the twin calls LAPACK -- the
amplification by cond(K) is the same, the constants are not.  A pair whose runs stop a check interval apart is held to TOL_TWIN_N only, and at most one pair
in eight of a case may be of that kind."""
import functools

import numpy as np

import scenarios as sc
import side_inputs as si
import srbd_oracle as orc

S13 = np.array([-1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, 1.0])
S3 = np.array([1.0, -1.0, 1.0])
S3_AXIAL = np.array([-1.0, 1.0, -1.0])
FEET_SWAPPED, HEEL_TOE_SWAPPED = [2, 3, 0, 1], [1, 0, 3, 2]
SHIFT = (37.0, -1000.0, 0.0)
SHIFT_F32 = (1000.0, -700.0, 0.0)
NAMES = ("rot90", "mirror", "relabel", "swapfeet", "shift")
MARGIN = 100.0              # pair_bar(N) / D_N
MAX_UNEQUAL_SHARE = 0.125   # pairs of a case that may stop at different iterations


def _turn(v, sign=1.0):
    """(x, y) -> (-y, x) on the last axis of v (..., 3) [sign = -1: the inverse]; a copy."""
    out = np.array(v, dtype=np.float64)
    out[..., 0], out[..., 1] = -sign * np.asarray(v)[..., 1], sign * np.asarray(v)[..., 0]
    return out


def _points(a, fn):
    """fn on the (..., 4, 3) view of a (..., 12) array of four points / forces / normals."""
    a = np.asarray(a, dtype=np.float64)
    return fn(a.reshape(a.shape[:-1] + (4, 3))).reshape(a.shape)


def _state_turn(x, sign):
    out = np.array(x, dtype=np.float64)
    for c in (3, 6, 9):
        out[..., c:c + 3] = _turn(out[..., c:c + 3], sign)
    out[..., 2] = out[..., 2] + sign * (np.pi / 2)
    return out


def rot90(x0, x_ref, foot, contact, pcom):
    def back(u, x=None):
        return _points(u, lambda f: _turn(f, -1.0)), None if x is None else _state_turn(x, -1.0)
    return _state_turn(x0, 1.0), _state_turn(x_ref, 1.0), _points(foot, _turn), np.array(contact), _turn(pcom), back


def mirror(x0, x_ref, foot, contact, pcom):
    flip = lambda f: f[..., FEET_SWAPPED, :] * S3

    def back(u, x=None):
        return _points(u, flip), None if x is None else np.asarray(x, dtype=np.float64) * S13
    return np.asarray(x0) * S13, np.asarray(x_ref) * S13, _points(foot, flip), np.asarray(contact)[..., FEET_SWAPPED], np.asarray(pcom) * S3, back


def _permuted(perm):
    def transform(x0, x_ref, foot, contact, pcom):
        def back(u, x=None):            # (both permutations are involutions)
            return _points(u, lambda f: f[..., perm, :]), None if x is None else np.array(x, dtype=np.float64)
        return np.array(x0), np.array(x_ref), _points(foot, lambda f: f[..., perm, :]), np.asarray(contact)[..., perm], np.array(pcom), back
    return transform


relabel = _permuted(HEEL_TOE_SWAPPED)
swapfeet = _permuted(FEET_SWAPPED)


def shifted(by):
    by = np.asarray(by, dtype=np.float64)

    def transform(x0, x_ref, foot, contact, pcom):
        x0, x_ref = np.array(x0, dtype=np.float64), np.array(x_ref, dtype=np.float64)
        x0[..., 3:6] += by
        x_ref[..., 3:6] += by

        def back(u, x=None):
            if x is not None:
                x = np.array(x, dtype=np.float64)
                x[..., 3:6] -= by
            return np.array(u), x
        return x0, x_ref, _points(foot, lambda f: f + by), np.array(contact), np.asarray(pcom, dtype=np.float64) + by, back
    return transform


shift = shifted(SHIFT)
TRANSFORMS = dict(rot90=rot90, mirror=mirror, relabel=relabel, swapfeet=swapfeet, shift=shift)
TRANSFORMS_F32 = dict(TRANSFORMS, shift=shifted(SHIFT_F32))


def side_image(name, kind, v):
    """The image under transformation `name` of a side input: kind "ext_wrench", v (..., N, 6) = [tau, f]; kind "normals", v (..., N, 12)."""
    v = np.array(v, dtype=np.float64)
    if kind == "ext_wrench":
        if name == "rot90":
            v[..., 0:3], v[..., 3:6] = _turn(v[..., 0:3]), _turn(v[..., 3:6])
        elif name == "mirror":
            v[..., 0:3] *= S3_AXIAL
            v[..., 3:6] *= S3
        return v
    assert kind == "normals", kind
    if name == "rot90":
        return _points(v, _turn)
    if name == "mirror":
        return _points(v, lambda f: f[..., FEET_SWAPPED, :] * S3)
    if name in ("relabel", "swapfeet"):
        return _points(v, lambda f: f[..., HEEL_TOE_SWAPPED if name == "relabel" else FEET_SWAPPED, :])
    return v


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
# (path, N, schedule, yaw kind, B).  B = 6 at N <= 12, 3 at N >= 16 (the twins of a case take a few seconds).  Yaw kinds: every kind at N <= 10; "random"
# is left to N <= 10 as in tests/test_gpu_turning.py (the fixed-rho twin leaves too many longer ones at the cap).
def _b(N):
    return 6 if N <= 12 else 3


WAVE_RESTART = dict(rho_restart_iter=40, rho_restart_count=4)        # tests/test_gpu_parity.py::test_one_wave_kernel_restarts_in_place, its second case
CASES = [("wave", 4, "single", "random", 6), ("wave", 8, "single", "wrap", 6), ("wave", 10, "single", "turn", 6), ("wave_restart", 10, "single", "wrap", 6),
         ("compact", 10, "single", "random", 6), ("compact_auto", 12, "single", "turn", 6),
         ("wrench", 4, "double", "turn", 6), ("wrench", 8, "mixed", "random", 6), ("wrench", 10, "double", "wrap", 6), ("wrench", 10, "three", "turn", 6),
         ("wrench", 12, "mixed", "wrap", 6), ("wrench", 16, "double", "turn", 3), ("wrench", 20, "mixed", "wrap", 3), ("wrench", 24, "mixed", "turn", 3),
         ("staged_compact", 10, "single", "turn", 6), ("staged_wrench", 10, "double", "wrap", 6),
         ("any_horizon", 7, "mixed", "turn", 6), ("any_horizon", 15, "mixed", "wrap", 3),
         ("ew", 10, "mixed", "turn", 6), ("staged_ew", 10, "mixed", "wrap", 6), ("cn", 10, "mixed", "turn", 6)]
RAGGED_HORIZONS, RAGGED_PER_HORIZON = (8, 12, 16, 24), 2
F32_CASES = [("f32", 10, "double", "turn", 6), ("f32_tiles", 20, "double", "turn", 3), ("f32", 20, "mixed", "wrap", 3)]
SIDE_OF = {"ew": "ext_wrench", "staged_ew": "ext_wrench", "cn": "normals"}
assert all(B == _b(N) for _, N, _, _, B in CASES + F32_CASES)


# Three seeds moved on, each chosen on the CPU from the ORACLE's result alone.  seed() is shared by every case of the same (N, schedule, yaw kind), so a
# moved seed moves the scenes of ALL of them:
#   (20, "double", "turn") and (20, "mixed", "wrap"): the fp32 cases ask for status SOLVED outright (as tests/test_gpu_wrench.py's), and on the first draws
#     the float32 twin leaves one scene at the iteration cap.  With these every scene and image of the three fp32 cases ends SOLVED in the float32 twin at
#     least two check intervals under the cap.  The fp64 case ("wrench", 20, "mixed", "wrap") runs the same, moved, scenes.
#   (10, "single", "wrap"): the "wave_restart" case is about the in-place restart, and on the first draws no scene goes past the first mark of 40
#     iterations (the restarted twin equals the plain one bit for bit).  With this one the twin takes base scenes 0 and 3 to 90 and 85 iterations -- past the
#     second mark -- and ends them SOLVED, images alike (RESTARTED_MIN below).  No other case draws this triple.
# tests/test_symmetries_cpu.py asserts all of it.
SEED_SHIFT = {(20, "double", "turn"): 1000, (20, "mixed", "wrap"): 2000, (10, "single", "wrap"): 2000}
RESTARTED_MIN = 2           # base scenes of the "wave_restart" case that must run past the first restart mark and end SOLVED (in every block of images too)


def seed(N, schedule, yaw):
    return 8100 + 10 * N + 3 * si.SCHEDULES.index(schedule) + sc.YAW_KINDS.index(yaw) + SEED_SHIFT.get((N, schedule, yaw), 0)


@functools.lru_cache(maxsize=None)
def scenes(N, schedule, yaw, B):
    """The B base scenes of a case: (x0, x_ref, foot, contact, pcom) of scenarios.batch(..., pcom=True)."""
    return sc.batch(B, N, seed(N, schedule, yaw), schedule, yaw=yaw, pcom=True)


@functools.lru_cache(maxsize=None)
def side_input(path, N, B):
    """The side input of the B base scenes of an "ew" / "staged_ew" / "cn" case (None for every other path)."""
    if path not in SIDE_OF:
        return None
    if SIDE_OF[path] == "ext_wrench":
        return si.draw_wrench(B, N, si.wrench_seed(N))
    return si.drawn_normals(B, N, np.random.default_rng(77 + N), per_step=True)


def transforms_of(path, f32=False):
    """The transformations a path is held to.  With tilted normals the tangent axes of contact_frames follow a world-axis convention (the pyramid's edges
    are not turned with the world), so rot90 is no symmetry of that QP: tests/test_symmetries_cpu.py shows the twin breaks it by newtons and holds the other
    four, and only those enter."""
    names = tuple(n for n in NAMES if not (path == "cn" and n == "rot90"))
    table = TRANSFORMS_F32 if f32 else TRANSFORMS
    return [(n, table[n]) for n in names]


def stacked(path, N, schedule, yaw, B, f32=False):
    """The batch of one solve call: the B base scenes followed by their images, block by block in the order of transforms_of(path) ->
    (x0, x_ref, foot, contact, pcom, side or None, backs); backs[j] maps block j + 1 into the base frame."""
    base = scenes(N, schedule, yaw, B)
    side = side_input(path, N, B)
    parts, sides, backs = [base], [side], []
    for name, fn in transforms_of(path, f32):
        *img, back = fn(*base)
        parts.append(tuple(img)); backs.append((name, back))
        sides.append(None if side is None else side_image(name, SIDE_OF[path], side))
    out = [np.concatenate([p[i] for p in parts]) for i in range(5)]
    out[3] = out[3].astype(np.uint8)
    return tuple(out) + (None if side is None else np.concatenate(sides), backs)


# ---- the twin and its own deviations --------------------------------------------------------------------------------------------------------------
def twin_params(path, N):
    """The oracle's parameters of a path's solve: the fixed-rho twin where the engine runs with the restart off (as tests/test_gpu_wrench.py::_engine), the
    restarted one where the test is about it or the path keeps the engine's default (the side inputs, the any-horizon mode: as their own suites)."""
    if path == "wave_restart":
        return orc.params_for(N, rho_restart_iter=WAVE_RESTART["rho_restart_iter"], rho_restart_count=min(WAVE_RESTART["rho_restart_count"], 3))
    if path in SIDE_OF or path == "any_horizon":
        return orc.default_params(N)
    return orc.params_for(N)


def _twin_key(path):
    """Paths whose twins are the same computation share one cache entry."""
    return {"wave": "plain", "compact": "plain", "compact_auto": "plain", "wrench": "plain", "staged_compact": "plain", "staged_wrench": "plain",
            "ragged": "plain", "staged_ew": "ew"}.get(path, path)


def twin_one(path, N, x0, x_ref, foot, contact, pcom, side=None):
    """The fp64 twin of ONE QP of a path -> dict(u, x, status, iters, ...)."""
    p = twin_params(path, N)
    if path in SIDE_OF:
        return si.twin(p, x0, x_ref, foot, contact, pcom=pcom, **{SIDE_OF[path]: side})
    return orc.update(p, x0, x_ref, foot, contact, pcom_hor=pcom)


@functools.lru_cache(maxsize=None)
def _twins(key, N, schedule, yaw, B):
    path = {"plain": "wrench", "ew": "ew"}.get(key, key)
    x0, xr, ft, ct, pc, side, backs = stacked(path, N, schedule, yaw, B)
    return tuple(twin_one(path, N, x0[b], xr[b], ft[b], ct[b], pc[b], None if side is None else side[b]) for b in range(len(x0)))


def twins(path, N, schedule, yaw, B):
    """The twin of every QP of stacked(...): computed once per case, shared by the tests that need it, left unchanged."""
    return _twins(_twin_key(path), N, schedule, yaw, B)


def pair_deviation(res, b, j, B, back):
    """Base QP b against its image in block j + 1 of a stacked result res (a sequence of per-QP dicts with u, x, status, iters): (|du|, |dx|, same status,
    same iteration count), the image mapped into the base frame."""
    r0, r1 = res[b], res[(j + 1) * B + b]
    u1, x1 = back(r1["u"], r1["x"])
    return (float(np.abs(u1 - r0["u"]).max()), float(np.abs(x1 - r0["x"]).max()), int(r0["status"]) == int(r1["status"]), int(r0["iters"]) == int(r1["iters"]))


@functools.lru_cache(maxsize=None)
def twin_deviation(path, N, schedule, yaw, B):
    """{transformation: (largest |du| [N], largest |dx|, every status equal, every iteration count equal)} of the TWIN over the B pairs of a case."""
    ref = twins(path, N, schedule, yaw, B)
    out = {}
    for j, (name, back) in enumerate(stacked(path, N, schedule, yaw, B)[6]):
        d = [pair_deviation(ref, b, j, B, back) for b in range(B)]
        out[name] = (max(v[0] for v in d), max(v[1] for v in d), all(v[2] for v in d), all(v[3] for v in d))
    return out


@functools.lru_cache(maxsize=None)
def twin_d(N, side=None):
    """D_N: the largest deviation (forces in newtons, states in their own units: the larger of the two) of the twin over all fp64 cases of horizon N --
    side=None: the cases without a side input; side="ext_wrench" / "normals": those under that side input.  (Taken apart because the restarted twin under a
    wrench deviates 5e-7 - 9e-7 N at N = 10 where the plain twins stay under 8e-8 N and the one on contact frames under 5e-8 N: one D over all would hold
    the plain kernels and the normals 12 - 19 x more loosely than their own twin allows.  Each is at most the D over all cases of the horizon.)"""
    cases = [c for c in CASES if c[1] == N and SIDE_OF.get(c[0]) == side]
    assert cases, (N, side)
    return max(max(v[0], v[1]) for c in cases for v in twin_deviation(*c).values())


def pair_bar(N, side=None):
    """The bar on a kernel's pair that stopped at equal iteration counts: MARGIN x D_N, D_N from the twin inside this run."""
    return MARGIN * twin_d(N, side)


def restarted(res, B):
    """How many of the B base QPs of the "wave_restart" case ran past the first restart mark and ended SOLVED, in the base block and in EVERY block of images
    of `res` (per-QP dicts of the stacked solve, twin's or kernel's): a case that is about the restart must exercise the second pass."""
    mark = WAVE_RESTART["rho_restart_iter"]
    return sum(all(res[j * B + b]["iters"] > mark and res[j * B + b]["status"] == orc.STATUS_SOLVED for j in range(len(res) // B)) for b in range(B))


# ---- fp32: every image on its own -----------------------------------------------------------------------------------------------------------------
def rounded(a):
    """What an _f32 entry point sees of a float64 array."""
    return np.asarray(a, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def twins32(path, N, schedule, yaw, B):
    """The float32 twin (orc.update_split; "f32_tiles": with the fp32-tile rule) and the exact optimum of every scene of stacked(..., f32=True), the inputs
    rounded to float32 AFTER the transformation (rounding breaks the pairing: 1000 m + 0.1 m keeps 6e-5 m in float32) -> (twins with "xs", parameters)."""
    x0, xr, ft, ct, pc, _, _ = stacked(path, N, schedule, yaw, B, f32=True)
    p = orc.params_for(N, eps_abs=2e-6, eps_rel=2e-6)       # the fp32 path's tolerance floor (tests/test_gpu_wrench.py)
    refs = []
    for b in range(len(x0)):
        ref = orc.update_split(p, x0[b], xr[b], ft[b], ct[b], pcom_hor=pc[b], dtype=np.float32, **(dict(tile_dtype="auto") if path == "f32_tiles" else {}))
        ref["xs"] = orc.solve_reference(p, ref["qp"])[0]
        refs.append(ref)
    return tuple(refs), p


# ---- one ragged fleet -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_fleet():
    """RAGGED_PER_HORIZON base QPs per horizon of RAGGED_HORIZONS (the scenes of that horizon's "wrench" case in CASES; the ragged path takes the CoM horizon
    from x_ref) followed by their five images, block by block -> (problems for RaggedMPC.solve, horizons per QP, backs, twins, number of base QPs)."""
    blocks = [[] for _ in range(1 + len(NAMES))]
    for N in RAGGED_HORIZONS:
        c = next(c for c in CASES if c[0] == "wrench" and c[1] == N)
        x0, xr, ft, ct, _ = (a[:RAGGED_PER_HORIZON] for a in scenes(*c[1:]))
        base = (x0, xr, ft, ct, xr[..., 3:6])
        for j, img in enumerate([base] + [TRANSFORMS[n](*base)[:5] for n in NAMES]):
            blocks[j] += [dict(x0=img[0][b], x_ref=img[1][b], foot=img[2][b], contact=img[3][b].astype(np.uint8)) for b in range(RAGGED_PER_HORIZON)]
    problems = [pr for blk in blocks for pr in blk]
    # (back() of every transformation depends on the transformation alone -- a rotation, a sign pattern, a permutation, a fixed offset --, never on the arrays
    # it was made with: one back per transformation, made on placeholders, serves the QPs of every horizon)
    backs = [(n, TRANSFORMS[n](*(np.zeros(s) for s in ((13,), (1, 13), (1, 12), (1, 4), (1, 3))))[5]) for n in NAMES]
    refs = tuple(orc.update(orc.params_for(pr["x_ref"].shape[0]), pr["x0"], pr["x_ref"], pr["foot"], pr["contact"]) for pr in problems)
    return problems, [pr["x_ref"].shape[0] for pr in problems], backs, refs, len(blocks[0])
