"""GPU tests of the fleet roll-out over terrain (include/srbdqp_cascade.h srbdqp_set_terrain, srbdqp_terrain_sample_*, srbdqp_terrain_inputs_*, and
srbdqp_fleet_advance_* / srbdqp_fleet_rollout_* with a map set) against the NumPy twin of tests/terrain_twin.py (tests/test_terrain_cpu.py
holds the twin itself).

Bounds.  z of the sample, x_ref of the inputs step, stamps, alive flags and footholds: bit for bit -- every operation that makes them is one rounded fp64
operation in a fixed order.  Normals: 1e-15, the square root and the divisions being the target's own (each test prints whether they came out bit-equal).  States
behind a plant step: 1e-9, forces against the twin's solve: side_inputs.TOL_TWIN_N (2e-3 N) -- the bounds of tests/test_gpu_fleet.py and of the side-input suites."""
import numpy as np
import pytest

import srbd_oracle as orc
import fleet_twin as ft
from fleet_loop import _bits, _stamps, crowd, device_loop
import side_inputs as si
import terrain_twin as tt

pytestmark = pytest.mark.gpu
N = 10


@pytest.fixture(scope="module")
def eng():
    import torch  # noqa: F401
    from g1_locomotion_amd import BatchMPC
    e = BatchMPC(horizon=N)
    yield e
    e.close()


@pytest.fixture(scope="module")
def rough():
    """The seeded rough 17 x 9 map, neighbour differences up to 0.5 cell: x in [-1, 3], y in [-1, 1]."""
    m = tt.rough(17, 9, seed=11, cell=0.25, origin=(-1.0, -1.0))
    m.h.setflags(write=False)
    return m


def _points(m, M, seed):
    """M points of every kind: nodes, grid lines, the last row and column, outside all four sides and corners, inside cells (the kinds cycle, so that a
    single point is a node and 64 hold every kind)."""
    rng = np.random.default_rng(seed)
    x1, y1 = m.x0 + (m.nx - 1) * m.cell, m.y0 + (m.ny - 1) * m.cell
    rx = lambda: rng.uniform(m.x0, x1)
    ry = lambda: rng.uniform(m.y0, y1)
    nx_ = lambda: m.x0 + m.cell * rng.integers(0, m.nx)
    ny_ = lambda: m.y0 + m.cell * rng.integers(0, m.ny)
    kinds = [lambda: (nx_(), ny_()), lambda: (nx_(), ry()), lambda: (rx(), ny_()), lambda: (x1, ry()), lambda: (rx(), y1), lambda: (x1, y1),
             lambda: (m.x0 - rng.uniform(0.01, 5.0), ry()), lambda: (x1 + rng.uniform(0.01, 5.0), ry()), lambda: (rx(), m.y0 - rng.uniform(0.01, 5.0)),
             lambda: (rx(), y1 + rng.uniform(0.01, 5.0)), lambda: (m.x0 - 1.0, m.y0 - 2.0), lambda: (x1 + 1e9, m.y0 - 1.0), lambda: (m.x0 - 3.0, y1 + 1e300),
             lambda: (x1 + 0.5, y1 + 0.5), lambda: (rx(), ry()), lambda: (rx(), ry())]
    return np.array([kinds[k % len(kinds)]() for k in range(M)], np.float64)


def _normals_close(got, want, what):
    err = np.abs(got - want).max()
    print(what, "normals: max |gpu - twin|", err, "bit-equal" if np.array_equal(_bits(got), _bits(want)) else "not bit-equal")
    assert err <= 1e-15, err


@pytest.mark.parametrize("which", ["one cell", "3 x 5", "rough"])
def test_sample_against_the_twin(eng, rough, which):
    """z bit for bit and normals within 1e-15, at 1, 64, 65 and 1000 points of every kind, through host buffers and through device pointers."""
    import torch
    m = {"one cell": tt.Map(np.array([[0.1, 0.3], [-0.2, 0.25]]), origin=(0.5, -0.5), cell=0.5),
         "3 x 5": tt.Map(np.random.default_rng(2).uniform(-0.1, 0.1, (5, 3)), origin=(-0.3, 0.2), cell=0.2), "rough": rough}[which]
    eng.set_terrain(**m.args())
    try:
        for M in (1, 64, 65, 1000):
            xy = _points(m, M, 100 + M)
            z, n = tt.sample(m, xy)
            got = eng.terrain_sample(xy)
            assert eng.kernel_name() == "terrain_sample_f64"
            assert np.array_equal(_bits(got["z"]), _bits(z)), M
            _normals_close(got["normal"], n, f"sample, {which}, M = {M}:")
            assert np.array_equal(_bits(eng.terrain_sample(xy, want_normal=False)["z"]), _bits(z))
        dev = torch.device("cuda", 0)
        xy = _points(m, 65, 7)
        xy[3] = (np.nan, 0.0); xy[9] = (0.1, np.inf)
        z, n = tt.sample(m, xy)
        dxy, dz, dn = torch.from_numpy(xy).to(dev), torch.full((65,), -7.0, dtype=torch.float64, device=dev), torch.full((65, 3), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()                                                 # (fleet_loop.py's stream rule)
        eng.terrain_sample_device(65, dxy.data_ptr(), dz.data_ptr(), dn.data_ptr())
        eng.synchronize()
        assert np.array_equal(_bits(dz.cpu().numpy()), _bits(z)) and np.isnan(z[3]) and np.isnan(z[9])
        _normals_close(dn.cpu().numpy(), n, f"sample_device, {which}:")
        assert np.array_equal(dn.cpu().numpy()[[3, 9]], np.tile([0.0, 0.0, 1.0], (2, 1)))
    finally:
        eng.set_terrain(None)


def test_set_terrain_refusals_clearing_and_the_solves_it_leaves_alone(eng):
    from g1_locomotion_amd import SrbdqpError, _lib
    import ctypes as C
    x0, xr, fo, ct = orc.synthetic_batch(16, N, seed=21, schedule="single")
    before = eng.solve(x0, xr, fo, ct)
    with pytest.raises(SrbdqpError, match="no terrain is set"):
        eng.terrain_sample(np.zeros((3, 2)))
    with pytest.raises(SrbdqpError, match="no terrain is set"):
        eng.terrain_inputs(np.zeros((2, 12)), np.zeros((2, N, 13)))
    good = np.array([[0.0, 0.1, 0.2], [0.1, 0.2, 0.3]])
    eng.set_terrain(good, origin=(0.0, 0.0), cell=0.25)
    mark = eng.terrain_sample(np.array([[0.3, 0.1]]))["z"]

    def bad_h(i, j, v):
        a = good.copy()
        a[j, i] = v
        return a

    for kw, words in ((dict(heights=good, cell=0.0), "cell must be finite and positive"), (dict(heights=good, cell=float("nan")), "cell must be finite and positive"),
                      (dict(heights=good, cell=float("inf")), "cell must be finite and positive"), (dict(heights=good, cell=-0.25), "cell must be finite and positive"),
                      (dict(heights=good, cell=0.25, origin=(float("nan"), 0.0)), "origin"), (dict(heights=good, cell=0.25, origin=(0.0, float("inf"))), "origin"),
                      (dict(heights=good[:1], cell=0.25), "at least 2"), (dict(heights=good[:, :1], cell=0.25), "at least 2"),
                      (dict(heights=bad_h(1, 1, np.nan), cell=0.25), r"node \(1, 1\) is not finite"), (dict(heights=bad_h(2, 0, np.inf), cell=0.25), r"node \(2, 0\) is not finite"),
                      (dict(heights=bad_h(1, 0, 0.41), cell=0.25), r"nodes \(0, 0\) and \(1, 0\) differ by more than 1.2 cell"),
                      (dict(heights=bad_h(0, 1, 0.31), cell=0.25), r"nodes \(0, 0\) and \(0, 1\) differ by more than 1.2 cell")):
        with pytest.raises(SrbdqpError, match="srbdqp_set_terrain: .*" + words):
            eng.set_terrain(**kw)
    t = _lib.Terrain()
    t.struct_size, t.nx, t.ny, t.cell = C.sizeof(_lib.Terrain) - 8, 3, 2, 0.25
    assert eng._lib.srbdqp_set_terrain(eng._h, C.byref(t), good.ctypes.data_as(C.c_void_p)) == _lib.E_INVALID
    assert b"struct_size" in eng._lib.srbdqp_last_error(eng._h)
    t.struct_size, t.nx, t.ny = C.sizeof(_lib.Terrain), 1 << 13, (1 << 11) + 1            # nx ny above 2^24: refused before a height is read
    assert eng._lib.srbdqp_set_terrain(eng._h, C.byref(t), good.ctypes.data_as(C.c_void_p)) == _lib.E_INVALID
    assert b"2^24" in eng._lib.srbdqp_last_error(eng._h)
    # every refusal above left the map that was set
    assert np.array_equal(_bits(eng.terrain_sample(np.array([[0.3, 0.1]]))["z"]), _bits(mark))
    during = eng.solve(x0, xr, fo, ct)
    eng.set_terrain(None)
    with pytest.raises(SrbdqpError, match="no terrain is set"):
        eng.terrain_sample(np.zeros((3, 2)))
    eng.set_terrain(None)                                                                # clearing twice is no error
    after = eng.solve(x0, xr, fo, ct)
    for k in ("u", "x", "status", "iters"):
        assert np.array_equal(_bits(during[k]), _bits(before[k])) and np.array_equal(_bits(after[k]), _bits(before[k])), k


@pytest.mark.parametrize("horizon", [4, 10, 20])
def test_terrain_inputs_against_the_twin(rough, horizon):
    """B = 1, 33 (a tile and one robot) and 77: x_ref bit for bit -- column 5 raised, every other entry as it came --, normals within 1e-15."""
    import torch
    from g1_locomotion_amd import BatchMPC
    dev = torch.device("cuda", 0)
    with BatchMPC(horizon=horizon) as e:
        e.set_terrain(**rough.args())
        for B in (1, 33, 77):
            c = crowd("v_ref", B, 300 + B, 1, on=rough)
            feet = c["feet"].copy()
            feet[:, 2::3] += np.random.default_rng(B).normal(size=(B, 4)) * 0.01          # (the z handed in need not lie on the map)
            x_ref = np.random.default_rng(B + 1).normal(size=(B, horizon, 13))
            want = tt.inputs(rough, feet, x_ref)
            got = e.terrain_inputs(feet, x_ref)
            assert e.kernel_name() == "terrain_inputs_f64"
            assert np.array_equal(_bits(got["x_ref"]), _bits(want["x_ref"])), B
            assert np.array_equal(_bits(np.delete(got["x_ref"], 5, axis=2)), _bits(np.delete(x_ref, 5, axis=2)))
            _normals_close(got["normals"], want["normals"], f"inputs, N = {horizon}, B = {B}:")
            dfe, dxr = torch.from_numpy(feet).to(dev), torch.from_numpy(x_ref).to(dev)
            dcn = torch.full((B, horizon, 12), -7.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()                                             # (fleet_loop.py's stream rule)
            e.terrain_inputs_device(B, dfe.data_ptr(), dxr.data_ptr(), dcn.data_ptr())
            e.synchronize()
            assert np.array_equal(_bits(dxr.cpu().numpy()), _bits(got["x_ref"])) and np.array_equal(_bits(dcn.cpu().numpy()), _bits(got["normals"]))


def test_fleet_advance_on_the_rough_map_against_the_twin(eng, rough):
    """One period of 77 robots (a tile of 64 and a remainder of 13) standing on the rough map, tilted by up to 0.3 rad, some of them at a touchdown, some dead,
    under random pushes: stamps, alive flags and footholds (z included) bit for bit, states within 1e-9.  Robot 5 stands on the map's highest node with its CoM
    0.28 m over the ground -- fallen, though its absolute height is above z_min = 0.3 --, robot 6 on the lowest with its CoM 0.32 m over the ground -- up, though
    its absolute height is below z_min."""
    m = rough
    rng = np.random.default_rng(3)
    B = 77
    c = crowd("v_ref", B, 17, 1, on=m)
    x, feet, stamp, standing = c["x"], c["feet"], c["stamp"], c["standing"]
    jh, ih = np.unravel_index(np.argmax(m.h), m.h.shape)
    jl, il = np.unravel_index(np.argmin(m.h), m.h.shape)
    zr, zd = m.h[jh, ih], m.h[jl, il]
    assert zr > 0.05 and zd < -0.05
    x[5, 3:6] = (m.x0 + ih * m.cell, m.y0 + jh * m.cell, zr + 0.28)
    x[6, 3:6] = (m.x0 + il * m.cell, m.y0 + jl * m.cell, zd + 0.32)
    for b in (5, 6):                                                             # their feet under them, on the ground
        f = ft.FEET.copy(); f[:, 0:2] += x[b, 3:5] - ft.COM[0:2]; f[:, 2] = tt.sample(m, f[:, 0:2])[0]
        feet[b] = f.reshape(12)
    x[:, 0:2] += rng.uniform(-0.3, 0.3, (B, 2)); x[5:7, 0:2] = 0.0
    x[:, 6:12] += rng.normal(size=(B, 6)) * 0.05; x[5:7, 6:12] = 0.0
    p = orc.default_params(N)
    u0 = np.tile([0.0, 0.0, p.mass * 9.80665 / 4.0], (B, 4)) + rng.uniform(-20.0, 20.0, (B, 12))
    landing = np.concatenate([x[:, 3:5] + rng.uniform(-0.1, 0.2, (B, 2)), np.zeros((B, 1))], 1)
    push = rng.uniform(-1.0, 1.0, (B, 6)) * np.array([3.0, 3.0, 3.0, 30.0, 30.0, 30.0]); push[5:7] = 0.0
    alive = (rng.random(B) > 0.15).astype(np.uint8); alive[5:7] = 1
    eng.set_terrain(**m.args())
    try:
        for settings in ({}, dict(tilt_max=0.2, z_min=0.59, substeps=7, foot_half_length=0.06)):
            want = tt.advance(m, p, x, feet, stamp, u0, landing, standing=standing, push=push, alive=alive, **settings)
            got = eng.fleet_advance(x, feet, stamp, u0, landing, standing=standing, push=push, alive=alive, **settings)
            assert eng.kernel_name() == "fleet_advance_terrain_f64"
            if not settings:
                assert {1, 2} <= set(want["moved"].tolist()) and (want["moved"] == 0).sum() > 20 and 0 < (alive == 0).sum() < B // 2
                assert want["alive"][5] == 0 and x[5, 5] > 0.3 and want["alive"][6] == 1 and x[6, 5] < 0.3 and want["x"][6, 5] < 0.3
            else:
                assert 0 < (want["alive"][alive == 1] == 0).sum() < (alive == 1).sum()
            moved = np.where(np.any(got["feet"][:, 0:6] != feet[:, 0:6], axis=1), 1, np.where(np.any(got["feet"][:, 6:12] != feet[:, 6:12], axis=1), 2, 0))
            assert np.array_equal(moved, want["moved"])
            assert np.array_equal(_bits(got["stamp"]), _bits(want["stamp"])) and np.array_equal(_bits(got["feet"]), _bits(want["feet"]))
            assert np.array_equal(got["alive"], want["alive"])
            land = got["feet"].reshape(B, 4, 3)[moved > 0]
            assert np.any(land[:, :, 2] != 0.0)                                  # the feet that landed stand on the map, not on z = 0
            err = np.abs(got["x"] - want["x"]).max()
            print("fleet_advance on the rough map against the twin", settings, err)
            assert err < 1e-9, err
            dead = alive == 0
            assert np.array_equal(_bits(got["x"][dead]), _bits(x[dead])) and np.array_equal(_bits(got["feet"][dead]), _bits(feet[dead]))
    finally:
        eng.set_terrain(None)


@pytest.mark.parametrize("B,defer", [(6, False), (70, False), (70, True)])
def test_the_loop_is_the_public_calls(rough, B, defer):
    """rollout_device() over 8 steps on the rough map against mpc_inputs_device -> terrain_inputs_device -> set_contact_normals (device) + solve_device ->
    fleet_advance_device driven step by step on the same engine: every log and every final array bit for bit; once on a SRBDQP_FLAG_DEFER_TAIL engine, where the
    restart passes run on the tail stream with the normals of the call and a flush follows every solve."""
    import torch  # noqa: F401
    from g1_locomotion_amd import BatchMPC, _lib
    steps = 8
    c = crowd("v_ref", B, 40 + B, steps, on=rough)
    with BatchMPC(horizon=N, **(dict(flags=_lib.FLAG_DEFER_TAIL) if defer else {})) as e:
        e.set_terrain(**rough.args())
        call, loop, name = device_loop(e, c, B, steps, "terrain", defer=defer)
    assert name == "fleet_advance_terrain_f64"
    for k in call:
        assert np.array_equal(_bits(call[k]), _bits(loop[k])), k
    assert np.array_equal(_bits(call["x_log"][-1]), _bits(call["x"])) and np.array_equal(_bits(call["x_log"][0]), _bits(c["x"]))
    print("the loop on the rough map: solved", (call["status_log"] == 1).mean(), "alive", call["alive"].mean())
    assert (call["status_log"] == 1).mean() > 0.5 and np.any(call["feet_log"][-1] != call["feet_log"][0])
    fl = call["feet_log"].reshape(-1, 3)                                          # every foothold of every step stands on the map
    assert np.array_equal(_bits(fl[:, 2]), _bits(tt.sample(rough, fl[:, 0:2])[0]))
    assert np.array_equal(_bits(call["x_log"][:, 3]), _bits(np.tile(c["x"][3], (steps + 1, 1)))) and call["alive"][3] == 0   # the robot that came in dead held
    assert call["stamp"][3] == _stamps(c["stamp"], steps)[-1, 3]


def test_chunks_compose(eng, rough):
    """rollout(5) and rollout(7) from where it ended = rollout(12), bit for bit."""
    c = crowd("v_ref", 21, 7, 12, on=rough)
    eng.set_terrain(**rough.args())
    try:
        a = eng.rollout(c["x"], c["feet"], c["stamp"], c["v_ref"], 5, ft.COM, standing=c["standing"], push=c["push"][:5])
        b = eng.rollout(a["x"][-1], a["feet"][-1], a["stamp"], c["v_ref"], 7, ft.COM, standing=c["standing"], push=c["push"][5:], alive=a["alive"])
        w = eng.rollout(c["x"], c["feet"], c["stamp"], c["v_ref"], 12, ft.COM, standing=c["standing"], push=c["push"])
    finally:
        eng.set_terrain(None)
    for k in ("x", "feet"):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k][1:]])), _bits(w[k])), k
    for k in ("u0", "status", "iters"):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k]])), _bits(w[k])), k
    assert np.array_equal(b["alive"], w["alive"]) and np.array_equal(_bits(b["stamp"]), _bits(w["stamp"]))


def test_teacher_forced_parity_on_the_slope(eng):
    """Robots 0, 1, 2 and 5 of the test fleet on z = 0.4 x, 24 steps, every step taken on its own: from the engine's x_log[t], feet_log[t] and u0_log[t] the twin's
    advance gives x_log[t + 1] within 1e-9 and feet_log[t + 1] bit for bit, and the twin's solve -- with the map's normals and the raised height reference -- ends
    with the engine's status and within 2e-3 N of u0_log[t].  No robot falls."""
    T, B = 24, 4
    g = tt.slope_fleet((0.4, 0.0))
    m = tt.plane(0.4, 0.0, nx=9, ny=9, origin=(-1.0, -2.0), cell=0.5)
    eng.set_terrain(**m.args())
    try:
        gpu = eng.rollout(g["x"], g["feet"], g["stamp"], g["v_ref"], T, ft.COM, standing=g["standing"])
    finally:
        eng.set_terrain(None)
    assert gpu["alive"].tolist() == [1] * B
    p = si.params(N)
    flat = lambda a: a.reshape((T * B,) + a.shape[2:])
    x, feet = flat(gpu["x"][:-1]), flat(gpu["feet"][:-1])
    stamp = flat(_stamps(g["stamp"], T)[:-1])
    rep = lambda a: np.tile(a, (T,) + (1,) * (a.ndim - 1))
    standing, v_ref = rep(g["standing"]), rep(g["v_ref"])
    inp, normals = tt.step_inputs(m, p, x, feet, stamp, v_ref, ft.COM, N, standing=standing)
    sol = tt.solve(p, x, inp, normals)
    assert np.array_equal(sol["status"], flat(gpu["status"]))
    du = np.abs(sol["u0"] - flat(gpu["u0"])).max()
    nxt = tt.advance(m, p, x, feet, stamp, flat(gpu["u0"]), inp["landing"], standing=standing)
    dx = np.abs(nxt["x"] - flat(gpu["x"][1:])).max()
    over = gpu["x"][:, :, 5] - 0.4 * gpu["x"][:, :, 3]
    print("teacher-forced on the slope: forces", du, "N, states", dx, "statuses", np.unique(sol["status"]).tolist(), "height over ground", over.min(), over.max())
    assert du < si.TOL_TWIN_N, du
    assert dx < 1e-9, dx
    assert np.array_equal(_bits(nxt["feet"]), _bits(flat(gpu["feet"][1:])))
    assert np.array_equal(_bits(gpu["stamp"]), _bits(_stamps(g["stamp"], T)[-1])) and nxt["alive"].tolist() == [1] * (T * B)
    assert np.any(gpu["feet"][-1] != gpu["feet"][0]) and over.min() > 0.5


def test_an_all_zero_map_against_the_flat_rollout():
    """Step 0 of a roll-out on an all-zero map against step 0 of the flat roll-out of a handle with kernel = SRBDQP_KERNEL_WRENCH (the same solve family; nothing
    is teacher-forced, so only step 0 is compared): equal status, u0 within 2e-3 N."""
    from g1_locomotion_amd import BatchMPC, _lib
    f = ft.fleet()
    args = (f["x"], f["feet"], f["stamp"], f["v_ref"], 2, ft.COM)
    with BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH) as e:
        flat = e.rollout(*args, standing=f["standing"])
        assert e.kernel_name() == "fleet_advance_f64"
    with BatchMPC(horizon=N) as e:
        e.set_terrain(np.zeros((4, 5)), origin=(-2.0, -2.0), cell=1.5)
        zero = e.rollout(*args, standing=f["standing"])
        assert e.kernel_name() == "fleet_advance_terrain_f64"
    du = np.abs(zero["u0"][0] - flat["u0"][0]).max()
    print("zero map against the flat roll-out on the general kernel, step 0:", du, "N")
    assert np.array_equal(zero["status"][0], flat["status"][0]) and du < 2e-3, du
    assert np.all(zero["feet"].reshape(-1, 3)[:, 2] == 0.0)


def test_refusals_of_a_terrain_rollout(rough):
    """What a terrain roll-out refuses, each by its message, before any launch; and a cleared map leaves the flat roll-out of a handle that never had one."""
    import torch
    from g1_locomotion_amd import BatchMPC, SrbdqpError, _lib
    from g1_locomotion_amd.mpc import robots_array, weights_array
    f = ft.fleet()
    steps = 3
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def refused(e, words):
        x, feet, stamp, v = up(f["x"]), up(f["feet"]), up(f["stamp"]), up(f["v_ref"])
        xl = torch.full((steps + 1, 6, 13), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()                                                 # (fleet_loop.py's stream rule)
        with pytest.raises(SrbdqpError, match=words + ".*while a terrain is set"):
            e.rollout_device(6, steps, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), v.data_ptr(), ft.COM, x_log=xl.data_ptr())
        e.synchronize()
        assert torch.all(xl == -7.0) and np.array_equal(x.cpu().numpy(), f["x"]) and np.array_equal(stamp.cpu().numpy(), f["stamp"])
        with pytest.raises(SrbdqpError, match=words + ".*while a terrain is set"):
            e.rollout(f["x"], f["feet"], f["stamp"], f["v_ref"], steps, ft.COM)

    with BatchMPC(horizon=N) as never:
        base = never.rollout(f["x"], f["feet"], f["stamp"], f["v_ref"], steps, ft.COM, standing=f["standing"])
    with BatchMPC(horizon=N) as e:
        e.set_terrain(**rough.args())
        for setter, value in (("set_robots", robots_array(6)), ("set_weights", weights_array(6)), ("set_external_wrench", np.full((6, N, 6), 0.5)),
                              ("set_contact_normals", np.tile([0.0, 0.0, 1.0], (6, N, 4)))):
            getattr(e, setter)(value)
            try:
                refused(e, "srbdqp_fleet_rollout: refused while .*srbdqp_" + setter)
            finally:
                getattr(e, setter)(None)
        ok = e.rollout(f["x"], f["feet"], f["stamp"], f["v_ref"], steps, ft.COM, standing=f["standing"])     # with every side input cleared it runs
        assert ok["x"].shape == (steps + 1, 6, 13)
        e.set_terrain(None)
        again = e.rollout(f["x"], f["feet"], f["stamp"], f["v_ref"], steps, ft.COM, standing=f["standing"])
        for k in ("x", "feet", "u0", "status", "iters", "alive", "stamp"):
            assert np.array_equal(_bits(again[k]), _bits(base[k])), k
        # without a map handle-level normals are refused in the flat roll-out's own words
        e.set_contact_normals(np.tile([0.0, 0.0, 1.0], (6, N, 4)))
        try:
            with pytest.raises(SrbdqpError, match="the plant stands on flat ground"):
                e.rollout(f["x"], f["feet"], f["stamp"], f["v_ref"], steps, ft.COM)
        finally:
            e.set_contact_normals(None)
    for kw, words in ((dict(horizon=9, flags=_lib.FLAG_ANY_HORIZON), "SRBDQP_FLAG_ANY_HORIZON"), (dict(horizon=N, flags=_lib.FLAG_RANK_AWARE), "SRBDQP_FLAG_RANK_AWARE"),
                      (dict(horizon=24), "not at N = 24"), (dict(horizon=N, kernel=_lib.KERNEL_WAVE), "read by the general kernel only"),
                      (dict(horizon=N, kernel=_lib.KERNEL_COMPACT), "read by the general kernel only")):
        with BatchMPC(**kw) as e:
            e.set_terrain(**rough.args())
            refused(e, "srbdqp_fleet_rollout: .*" + words)


def test_a_robot_with_a_nan_state_is_skipped_as_on_flat_ground(eng, rough):
    c = crowd("v_ref", 6, 99, 8, on=rough)
    steps = 8
    args = lambda d: (d["x"], d["feet"], d["stamp"], d["v_ref"], steps, ft.COM)
    g = {k: v.copy() for k, v in c.items()}
    g["x"][4, 7] = np.nan
    keep = [0, 1, 2, 3, 5]
    h = {k: (v[:, keep] if k == "push" else v[keep]) for k, v in c.items()}
    eng.set_terrain(**rough.args())
    try:
        r = eng.rollout(*args(g), standing=g["standing"], push=g["push"])
        w = eng.rollout(*args(h), standing=h["standing"], push=h["push"])
    finally:
        eng.set_terrain(None)
    assert r["alive"][4] == 0 and np.array_equal(r["alive"][keep], w["alive"])
    assert np.array_equal(_bits(r["x"][:, 4]), _bits(np.tile(g["x"][4], (steps + 1, 1)))) and np.array_equal(_bits(r["feet"][:, 4]), _bits(np.tile(g["feet"][4], (steps + 1, 1))))
    assert r["stamp"][4] == _stamps(g["stamp"], steps)[-1, 4]
    for k in ("x", "feet", "u0", "status", "iters"):
        assert np.array_equal(_bits(r[k][:, keep]), _bits(w[k])), k
