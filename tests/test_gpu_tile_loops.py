"""GPU tests of the second trip through the tile loops of the fleet kernels.  srbdqp_fleet_advance_kernel, srbdqp_wrench_observer_kernel (tiles of 64 robots),
srbdqp_mpc_inputs_kernel, srbdqp_mpc_inputs_commanded_kernel (its steered, tracked and two previewed instantiations) and srbdqp_terrain_inputs_kernel (tiles
of 32) all run

    for (tile = blockIdx.x; tile < tiles; tile += gridDim.x)

under launchers that cap the grid at 256 * 32 workgroups, and no other test or bench takes a fleet beyond 128 tiles: the second trip -- the LDS staging reused
behind the trailing barrier, the store flags of the tile before, b0 beyond 2^19 -- runs here alone.

One test per kernel on an engine of horizon 4 (small outputs).  A crowd of 77 robots of the kind the kernel's own twin test uses -- dead and non-finite robots,
robots at a touchdown, standing ones -- is repeated to B = cap * tile + tile + 13 robots, robot b being robot b mod 77 of the crowd: every workgroup takes a
second tile, the last a partial one.  77 shares no factor with 32 or 64, so every robot meets every lane; a robot's arithmetic does not depend on its lane, its
tile or its neighbours, so every output of the large call equals the small call's output gathered by the same index BIT FOR BIT.  What the small call computes
is the other tests' business (test_gpu_cascade.py, test_gpu_steer.py, test_gpu_terrain.py, test_gpu_fleet.py, test_gpu_observer.py: against the twins).  The
tracked and the previewed trips bring the crowds of their own suites -- test_gpu_track.py's odd robots, the previewed crowd with a command that is not a
number -- and take the device forms, which accept them."""
import time

import numpy as np
import pytest

import fleet_loop                    # (its crowd() by the module's name: this file's crowd is the fixture below)
import fleet_twin as ft
from fleet_loop import _bits
import terrain_twin as tt
from test_gpu_track import _odd

pytestmark = pytest.mark.gpu
N, DT, BS = 4, 0.04, 77
CAP = 256 * 32                       # the launchers' grid cap (csrc/srbdqp_wrench_lat_ew.hip, mpc_inputs_launch in csrc/srbdqp.hip)
ROUGH = dict(nx=17, ny=9, seed=11, cell=0.25, origin=(-1.0, -1.0))      # test_gpu_terrain.py's rough map: x in [-1, 3], y in [-1, 1]


def _fleet_size(tile):
    B = CAP * tile + tile + 13
    assert B // tile > CAP and -(-B // tile) == CAP + 2 and B % tile == 13      # a change of the cap or the tile cannot silently empty the test
    return B


@pytest.fixture(scope="module")
def eng():
    import torch  # noqa: F401
    from g1_locomotion_amd import BatchMPC
    e = BatchMPC(horizon=N)
    yield e
    e.close()


@pytest.fixture(scope="module")
def crowd():
    """77 robots on the rough map around their nominal stance at any heading: velocity references and commands of which some are zero, a fifth standing, stamps
    over every phase of the gait (touchdowns of either foot among them), pushes, robot records, estimates, a sixth dead, three whose state is not finite, one foot
    off the map.  Read-only."""
    from g1_locomotion_amd.mpc import robots_array
    rng = np.random.default_rng(77)
    m = tt.rough(**ROUGH)
    B = BS
    at = np.stack([rng.uniform(-0.4, 1.6, B), rng.uniform(-0.5, 0.5, B)], -1)
    feet = np.tile(ft.FEET, (B, 1, 1))
    feet[:, :, 0:2] += at[:, None, :]
    feet[:, :, 2] = tt.sample(m, feet.reshape(-1, 3)[:, 0:2])[0].reshape(B, 4)
    feet[40, 1, 0] += 7.0                                                       # (a contact point off the map: the clamped sample)
    x = np.zeros((B, 13)); x[:, 12] = -9.80665
    x[:, 3:5] = ft.COM[0:2] + at + rng.normal(size=(B, 2)) * 0.005
    x[:, 5] = tt.sample(m, x[:, 3:5])[0] + ft.COM[2] + rng.normal(size=B) * 0.005
    x[:, 0:2] = rng.uniform(-0.2, 0.2, (B, 2)); x[:, 2] = rng.uniform(-3.0, 3.0, B)
    x[:, 6:12] = rng.normal(size=(B, 6)) * 0.05
    x[9, 4] = np.nan; x[33, 11] = np.inf; x[76, 0] = np.nan
    stamp = DT * ((np.arange(B) * 5) % 12).astype(np.float64)
    v_ref = np.where(rng.random((B, 1)) < 0.3, 0.0, rng.uniform(-0.2, 0.3, (B, 2)) * np.array([1.0, 0.4]))
    cmd = rng.uniform(-1.0, 1.0, (B, 3)) * np.array([0.3, 0.1, 1.0])
    kind = np.arange(B) % 7
    cmd[kind == 0] = 0.0; cmd[kind == 1, 0:2] = 0.0; cmd[kind == 2, 2] = 0.0
    standing = (rng.random(B) < 0.2).astype(np.uint8)
    alive = (rng.random(B) > 0.17).astype(np.uint8)
    push = np.where(rng.random((B, 1)) < 0.5, rng.uniform(-1.0, 1.0, (B, 6)) * np.array([3.0, 3.0, 0.3, 30.0, 30.0, 30.0]), 0.0)
    rec = robots_array(B, mass=rng.uniform(25.0, 45.0, B), inertia=np.array([0.0820564, 0.0805015, 0.0032353]) * rng.uniform(0.7, 1.5, (B, 3)))
    w0 = rng.uniform(-1.0, 1.0, (B, 6)) * np.array([2.0, 2.0, 0.5, 30.0, 30.0, 30.0])
    landing = np.concatenate([x[:, 3:5] + rng.normal(size=(B, 2)) * 0.05, np.zeros((B, 1))], 1)
    landing[9] = landing[76] = 0.0
    landing_yaw = rng.uniform(-3.0, 3.0, B)
    # the forces of a standing robot's weight and a little more, so that a period under them stays a period of a robot: m g / 4 a contact, tilted
    u0 = np.zeros((B, 4, 3)); u0[:, :, 2] = rec[:, None, 0] * 9.80665 / 4.0 * rng.uniform(0.8, 1.2, (B, 4)); u0[:, :, 0:2] = rng.uniform(-1.0, 1.0, (B, 4, 2))
    out = dict(x=x, feet=feet.reshape(B, 12), stamp=stamp, v_ref=v_ref, command=cmd, standing=standing, alive=alive, push=push, robots=rec, w0=w0, landing=landing,
               landing_yaw=landing_yaw, u0=u0.reshape(B, 12))
    assert 3 < (alive == 0).sum() < B // 3 and 5 < standing.sum() < B // 2 and len(set(stamp.tolist())) == 12
    for v in out.values():
        v.setflags(write=False)
    return out


def _rep(a, idx):
    return None if a is None else np.take(a, idx, axis=0)


def _same(large, small, idx, what):
    """every array of the large call is the small call's, gathered: bit for bit (NaNs included)"""
    for k, v in small.items():
        if v is None:
            assert large[k] is None, (what, k)
            continue
        want = np.take(v, idx, axis=0)
        assert large[k].shape == want.shape and np.array_equal(_bits(large[k]), _bits(want)), (what, k)
        del want


def _timed(what, t0, B, tile):
    print(f"{what}: B = {B} robots = {-(-B // tile)} tiles of {tile} on {CAP} workgroups, {time.perf_counter() - t0:.1f} s")


def test_mpc_inputs_second_trip(eng, crowd):
    t0 = time.perf_counter()
    c, B = crowd, _fleet_size(32)
    idx = np.arange(B) % BS
    args = lambda f: (f(c["x"]), f(c["feet"]), f(c["stamp"]), f(c["v_ref"]), ft.COM)
    small = eng.mpc_inputs(*args(lambda a: a), standing=c["standing"])
    assert eng.kernel_name() == "mpc_inputs_f64"
    assert small["contact"].min() == 0 and small["contact"][c["standing"] == 1].min() == 1 and np.isnan(small["pcom"]).any()
    large = eng.mpc_inputs(*args(lambda a: np.take(a, idx, axis=0)), standing=_rep(c["standing"], idx))
    _same(large, small, idx, "mpc_inputs")
    del large
    _timed("mpc_inputs, second trip", t0, B, 32)


def test_mpc_inputs_steered_second_trip(eng, crowd):
    t0 = time.perf_counter()
    c, B = crowd, _fleet_size(32)
    idx = np.arange(B) % BS
    args = lambda f: (f(c["x"]), f(c["feet"]), f(c["stamp"]), f(c["command"]), ft.COM)
    small = eng.mpc_inputs_steered(*args(lambda a: a), standing=c["standing"])
    assert eng.kernel_name() == "mpc_inputs_steered_f64"
    assert small["contact"].min() == 0 and np.isnan(small["pcom"]).any() and np.any(small["x_ref"][:, :, 8] != 0.0)
    large = eng.mpc_inputs_steered(*args(lambda a: np.take(a, idx, axis=0)), standing=_rep(c["standing"], idx))
    _same(large, small, idx, "mpc_inputs_steered")
    del large
    _timed("mpc_inputs_steered, second trip", t0, B, 32)


def test_mpc_inputs_tracked_second_trip():
    """The tracked instantiation on test_gpu_track.py's 77-robot crowd, odd robots and all: every output and the pose behind the step equal the 77-robot
    call's gathered by the same index, bit for bit; so does the pose_log row of a one-step roll-out of the large fleet."""
    import torch
    t0 = time.perf_counter()
    B = _fleet_size(32)
    assert B == 262189
    c = _odd(fleet_loop.crowd("commanded", BS, 900, pose=True))
    idx = np.arange(B) % BS
    big = {k: (v if k == "push" else np.take(v, idx, axis=0)) for k, v in c.items()}
    with fleet_loop.engine(N) as e:
        small = fleet_loop.inputs_device(e, c, N, "tracked")
        assert np.isnan(small["pcom"]).any() and np.isnan(small["x_ref"]).any() and small["contact"].min() == 0
        large = fleet_loop.inputs_device(e, big, N, "tracked")
        assert e.kernel_name() == "mpc_inputs_tracked_f64"
        _same(large, small, idx, "mpc_inputs_tracked")
        del large
        # ... and the row of pose_log, which the same kernel writes in a roll-out
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        x, feet, stamp, cm, sd, po = up(big["x"]), up(big["feet"]), up(big["stamp"]), up(big["command"]), up(big["standing"]), up(big["pose"])
        pl = torch.full((1, B, 3), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()                                  # (fleet_loop.py's stream rule)
        e.rollout_device(B, 1, x.data_ptr(), feet.data_ptr(), stamp.data_ptr(), 0, ft.COM, standing=sd.data_ptr(), command=cm.data_ptr(), command_steps=1,
                         track=True, pose=po.data_ptr(), pose_log=pl.data_ptr())
        e.synchronize()
        want = np.take(small["pose"], idx, axis=0)
        assert np.array_equal(_bits(pl.cpu().numpy()[0]), _bits(want)) and np.array_equal(_bits(po.cpu().numpy()), _bits(want))
    _timed("mpc_inputs_tracked, second trip", t0, B, 32)


def test_mpc_inputs_previewed_second_trip():
    """The previewed instantiations, steered and tracked, on test_gpu_preview.py's crowd with a command that is not a number: every output equals the 77-robot
    call's gathered by the same index, bit for bit."""
    import torch
    t0 = time.perf_counter()
    B = _fleet_size(32)
    assert B == 262189
    c = fleet_loop.crowd("preview", BS, 900)
    c["command"][50, 2] = np.nan
    idx = np.arange(B) % BS
    big = {k: np.take(v, idx, axis=0) for k, v in c.items()}
    with fleet_loop.engine(N) as e:
        for flavour in ("steered", "tracked"):
            small = fleet_loop.inputs_device(e, c, N, flavour, preview=True)
            assert small["previewed"].any() and small["contact"].min() == 0 and np.isnan(small["foot"]).any()
            large = fleet_loop.inputs_device(e, big, N, flavour, preview=True)
            _same(large, small, idx, "mpc_inputs_previewed, " + flavour)
            del large
    torch.cuda.empty_cache()                                      # (the gigabyte of cached blocks goes back: the tests behind this one find the allocator as before)
    _timed("mpc_inputs_previewed, second trip", t0, B, 32)


def test_terrain_inputs_second_trip(eng, crowd):
    t0 = time.perf_counter()
    c, B = crowd, _fleet_size(32)
    idx = np.arange(B) % BS
    x_ref = eng.mpc_inputs(c["x"], c["feet"], c["stamp"], c["v_ref"], ft.COM, standing=c["standing"])["x_ref"]
    eng.set_terrain(**tt.rough(**ROUGH).args())
    try:
        small = eng.terrain_inputs(c["feet"], x_ref)
        assert eng.kernel_name() == "terrain_inputs_f64"
        assert np.abs(small["normals"][:, :, 0:2]).max() > 0.1 and np.any(small["x_ref"][:, :, 5] != x_ref[:, :, 5])       # the map is rough under them
        large = eng.terrain_inputs(np.take(c["feet"], idx, axis=0), np.take(x_ref, idx, axis=0))
    finally:
        eng.set_terrain(None)
    _same(large, small, idx, "terrain_inputs")
    del large
    _timed("terrain_inputs, second trip", t0, B, 32)


def _advance_args(c, f):
    return (f(c["x"]), f(c["feet"]), f(c["stamp"]), f(c["u0"]), f(c["landing"])), dict(standing=f(c["standing"]), push=f(c["push"]), alive=f(c["alive"]))


def test_fleet_advance_second_trip(eng, crowd):
    """The flat kernel under pushes and robot records, and the terrain + steered instantiation on the rough map: states, footholds, stamps, alive flags."""
    t0 = time.perf_counter()
    c, B = crowd, _fleet_size(64)
    idx = np.arange(B) % BS
    take = lambda a: np.take(a, idx, axis=0)
    for kernel, extra in (("fleet_advance_f64", {}), ("fleet_advance_terrain_steered_f64", dict(landing_yaw=c["landing_yaw"]))):
        if extra:
            eng.set_terrain(**tt.rough(**ROUGH).args())
        try:
            pos, kw = _advance_args(c, lambda a: a)
            eng.set_robots(c["robots"])
            small = eng.fleet_advance(*pos, **kw, **extra)
            assert eng.kernel_name() == kernel
            moved = np.where(np.any(small["feet"][:, 0:6] != c["feet"][:, 0:6], axis=1), 1, np.where(np.any(small["feet"][:, 6:12] != c["feet"][:, 6:12], axis=1), 2, 0))
            assert {0, 1, 2} <= set(moved.tolist())                                   # touchdowns of either foot, and none
            held = (c["alive"] == 0) | ~np.all(np.isfinite(c["x"]), axis=1)
            assert np.array_equal(_bits(small["x"][held]), _bits(c["x"][held])) and np.all(small["alive"][held] == 0) and small["alive"].any()
            assert not np.any(np.all(small["x"][~held] == c["x"][~held], axis=1))
            pos, kw = _advance_args(c, take)
            eng.set_robots(take(c["robots"]))
            large = eng.fleet_advance(*pos, **kw, **{k: take(v) for k, v in extra.items()})
            assert eng.kernel_name() == kernel
        finally:
            eng.set_robots(None)
            if extra:
                eng.set_terrain(None)
        _same(large, small, idx, kernel)
        del large, pos, kw
    _timed("fleet_advance, second trip (two instantiations)", t0, B, 64)


def test_fleet_advance_logs_and_the_observer_in_a_rollout_second_trip(eng, crowd):
    """One step of the observed roll-out: the plant step writes its logs (x, feet, u0, status, iters) and the observer w_log, fills ew from the estimates handed in
    and measures behind the period -- every log and every final array of the large fleet is the crowd's, gathered.  (The solve between them is the general kernel
    at either size: one QP a workgroup, no tile loop.)"""
    t0 = time.perf_counter()
    c, B = crowd, _fleet_size(64)
    idx = np.arange(B) % BS
    take = lambda a: np.take(a, idx, axis=0)
    run = lambda f: eng.rollout(f(c["x"]), f(c["feet"]), f(c["stamp"]), f(c["v_ref"]), 1, ft.COM, standing=f(c["standing"]), push=f(c["push"])[None], alive=f(c["alive"]),
                                observer=dict(gain=0.5, horizon_decay=0.9), w_est=f(c["w0"]))
    try:
        eng.set_robots(c["robots"])
        small = run(lambda a: a)
        assert (small["status"] == 1).any() and small["alive"].any() and np.any(small["w_log"][0] != c["w0"])
        eng.set_robots(take(c["robots"]))
        large = run(take)
    finally:
        eng.set_robots(None)
    for k in small:                                                              # logs are (steps[+1], B, ...): gather along the robots
        axis = 1 if k in ("x", "u0", "feet", "status", "iters", "w_log") else 0
        want = np.take(small[k], idx, axis=axis)
        assert large[k].shape == want.shape and np.array_equal(_bits(large[k]), _bits(want)), k
        del want
    del large
    _timed("observed roll-out of one step, second trip", t0, B, 64)


def test_wrench_observer_second_trip(eng, crowd):
    t0 = time.perf_counter()
    c, B = crowd, _fleet_size(64)
    idx = np.arange(B) % BS
    take = lambda a: np.take(a, idx, axis=0)
    try:
        eng.set_robots(c["robots"])
        pos, kw = _advance_args(c, lambda a: a)
        nxt = eng.fleet_advance(*pos, **kw)
        args = lambda f: (f(c["x"]), f(nxt["x"]), f(c["feet"]), f(c["u0"]), f(c["w0"]))
        st = dict(gain=0.7, horizon_decay=0.9, torque_max=0.5)
        small = eng.wrench_observer(*args(lambda a: a), alive=nxt["alive"], **st)
        assert eng.kernel_name() == "wrench_observer_f64"
        kept = np.all(small["w_est"] == c["w0"], axis=1)
        assert np.array_equal(kept, nxt["alive"] == 0) and 3 < kept.sum() < BS // 2 and np.any(np.abs(small["w_est"][:, 0:3]) == 0.5)      # kept, measured, clamped
        eng.set_robots(take(c["robots"]))
        large = eng.wrench_observer(*args(take), alive=take(nxt["alive"]), **st)
    finally:
        eng.set_robots(None)
    _same(large, small, idx, "wrench_observer")
    del large
    _timed("wrench_observer, second trip", t0, B, 64)
