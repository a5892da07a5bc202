"""CPU side of the fleet roll-out over terrain (include/srbdqp_cascade.h srbdqp_set_terrain, srbdqp_terrain_*): the library exports the
calls and the binding lists them, the refusals that need no device, the properties of the sample S as tests/terrain_twin.py states it, and the twin roll-out --
on an all-zero map against fleet_twin's flat one, and on the plane z = 0.4 x, where the slope has to matter.

The slope case (fixed on the CPU, NumPy only): robots 0, 1, 2 and 5 of fleet_twin.fleet() on z = 0.4 x, N = 10, T = 24, default parameters (mu = 0.8).  Measured
when it was fixed: all four stay up, every solve ends with status 1, tilt below 0.06 rad, CoM 0.56 - 0.61 m over the ground, first-step forces up to 19.8 N from
the flat-normal solve of the same inputs, which leaves the tilted pyramids by 28 N.

A note on "nodes give back their heights": with fx = 1 (the last column, where i = nx - 2) the definition gives h00 + 1 (h10 - h00), which is h10 only where
that difference is exact.  So the test holds every node bit for bit on a map of dyadic heights (every operation exact), every node with i < nx - 1 and j < ny - 1
bit for bit on a rough map, and the last row and column of the rough map to one unit in the last place."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fleet_twin as ft
import side_inputs as si
import terrain_twin as tt

CALLS = ("srbdqp_set_terrain", "srbdqp_terrain_sample_f64", "srbdqp_terrain_sample_device_f64", "srbdqp_terrain_inputs_f64", "srbdqp_terrain_inputs_device_f64")
N = 10


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def test_the_library_exports_the_terrain_calls_and_the_binding_lists_them(built_lib):
    from g1_locomotion_amd import _lib, BatchMPC
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in CALLS:
        assert f" T {name}\n" in syms, name
        assert name in _lib.SIGNATURES and getattr(built_lib, name).restype is C.c_int
    for method in ("set_terrain", "terrain_sample", "terrain_sample_device", "terrain_inputs", "terrain_inputs_device"):
        assert callable(getattr(BatchMPC, method))
    assert C.sizeof(_lib.Terrain) == 40
    # a null handle is refused, not dereferenced
    t = _lib.Terrain()
    t.struct_size = C.sizeof(_lib.Terrain)
    assert built_lib.srbdqp_set_terrain(None, C.byref(t), None) == _lib.E_INVALID
    assert built_lib.srbdqp_terrain_sample_f64(None, 1, None, None, None) == _lib.E_INVALID
    assert built_lib.srbdqp_terrain_sample_device_f64(None, 1, None, None, None, None) == _lib.E_INVALID
    assert built_lib.srbdqp_terrain_inputs_f64(None, 1, None, None, None) == _lib.E_INVALID
    assert built_lib.srbdqp_terrain_inputs_device_f64(None, 1, None, None, None, None) == _lib.E_INVALID


def _nodes(m):
    i, j = np.meshgrid(np.arange(m.nx), np.arange(m.ny))
    return np.stack([m.x0 + i * m.cell, m.y0 + j * m.cell], -1).reshape(-1, 2), i.reshape(-1), j.reshape(-1)


def test_sample_gives_nodes_back_and_is_continuous_across_cell_edges():
    rng = np.random.default_rng(5)
    # dyadic heights on a dyadic grid: every operation of S is exact, every node comes back bit for bit
    d = tt.Map(rng.integers(-64, 64, (7, 9)) / 1024.0, origin=(-0.5, 0.25), cell=0.125)
    xy, _, _ = _nodes(d)
    z, _ = tt.sample(d, xy)
    assert np.array_equal(_bits(z), _bits(d.h.reshape(-1)))
    # a rough map: interior and first nodes bit for bit, the last row and column (fx or fy = 1) to one unit in the last place
    m = tt.rough(17, 9, seed=11, cell=0.25, origin=(-1.0, -1.0))
    xy, i, j = _nodes(m)
    z, _ = tt.sample(m, xy)
    inner = (i < m.nx - 1) & (j < m.ny - 1)
    want = m.h.reshape(-1)
    assert inner.sum() == 16 * 8 and np.array_equal(_bits(z[inner]), _bits(want[inner]))
    assert np.all(np.abs(z[~inner] - want[~inner]) <= np.spacing(np.abs(want[~inner]).max()))
    # z is continuous across the lines between cells: one unit of the coordinate's last place either side of a line moves z by no more than the slope allows
    line = m.x0 + m.cell * np.arange(1, m.nx - 1)
    y = rng.uniform(m.y0, m.y0 + (m.ny - 1) * m.cell, line.size)
    lo, _ = tt.sample(m, np.stack([np.nextafter(line, -np.inf), y], -1))
    hi, _ = tt.sample(m, np.stack([np.nextafter(line, np.inf), y], -1))
    on, _ = tt.sample(m, np.stack([line, y], -1))
    assert max(np.abs(lo - on).max(), np.abs(hi - on).max()) < 1e-15
    line = m.y0 + m.cell * np.arange(1, m.ny - 1)
    x = rng.uniform(m.x0, m.x0 + (m.nx - 1) * m.cell, line.size)
    lo, _ = tt.sample(m, np.stack([x, np.nextafter(line, -np.inf)], -1))
    hi, _ = tt.sample(m, np.stack([x, np.nextafter(line, np.inf)], -1))
    on, _ = tt.sample(m, np.stack([x, line], -1))
    assert max(np.abs(lo - on).max(), np.abs(hi - on).max()) < 1e-15


def test_sample_of_a_plane_is_the_plane():
    rng = np.random.default_rng(6)
    for sx, sy in ((0.4, 0.0), (0.25, -0.3), (0.0, 0.0), (-0.3, 0.2)):
        m = tt.plane(sx, sy, z0=0.1, nx=9, ny=9, origin=(-1.0, -1.0), cell=0.25)
        xy = rng.uniform(-1.0, 1.0, (500, 2))
        z, n = tt.sample(m, xy)
        s = np.sqrt(sx * sx + sy * sy + 1.0)
        assert np.abs(z - (0.1 + sx * xy[:, 0] + sy * xy[:, 1])).max() < 1e-15
        assert np.abs(n - np.array([-sx, -sy, 1.0]) / s).max() < 1e-15
        assert np.abs(np.sqrt((n * n).sum(-1)) - 1.0).max() < 1e-15


def test_points_off_the_map_clamp_and_nan_gives_nan_on_flat_ground():
    m = tt.rough(5, 4, seed=3, cell=0.5, origin=(1.0, -2.0))
    x1, y1 = m.x0 + (m.nx - 1) * m.cell, m.y0 + (m.ny - 1) * m.cell
    inside = np.array([[1.3, -1.1], [2.9, -0.6]])
    off = {"left": ([-5.0, -1.1], [m.x0, -1.1]), "right": ([1e9, -1.1], [x1, -1.1]), "below": ([1.3, -1e300], [1.3, m.y0]), "above": ([1.3, 7.0], [1.3, y1]),
           "corner 00": ([-1.0, -9.0], [m.x0, m.y0]), "corner 10": ([99.0, -9.0], [x1, m.y0]), "corner 01": ([0.0, 3.0], [m.x0, y1]),
           "corner 11": ([1e308, 1e308], [x1, y1])}
    for name, (p, q) in off.items():
        (zp, np_), (zq, nq) = tt.sample(m, [p]), tt.sample(m, [q])
        assert np.array_equal(_bits(zp), _bits(zq)) and np.array_equal(_bits(np_), _bits(nq)), name
    z, n = tt.sample(m, inside)
    assert np.all(np.isfinite(z))
    bad = np.array([[np.nan, 0.0], [0.0, np.nan], [np.inf, 0.0], [1.3, -np.inf], [np.nan, np.nan]])
    z, n = tt.sample(m, bad)
    assert np.all(np.isnan(z)) and np.array_equal(n, np.tile([0.0, 0.0, 1.0], (5, 1)))
    # every normal such a map can produce keeps n_z >= 0.5: neighbours at most 1.2 cell apart bound gx^2 + gy^2 by 2.88
    steep = tt.Map(np.array([[0.0, 0.6, 0.0], [0.6, 1.2, 0.6], [0.0, 0.6, 0.0]]), cell=0.5)
    _, n = tt.sample(steep, np.random.default_rng(1).uniform(0.0, 1.0, (2000, 2)))
    assert n[:, 2].min() >= 1.0 / np.sqrt(3.88) - 1e-15 > 0.5


def test_twin_on_an_all_zero_map_is_the_flat_twin():
    """The statuses and iteration counts of fleet_twin.rollout(solver="numpy"), states and footholds within 1e-8 -- the bound tests/test_fleet_cpu.py holds the
    two CPU oracles to."""
    f = ft.fleet()
    T = 12
    p = si.params(N)
    flat = ft.rollout(p, f["x"], f["feet"], f["stamp"], f["v_ref"], T, ft.COM, standing=f["standing"], push=ft.fleet_push(T, 6), solver="numpy")
    m = tt.Map(np.zeros((5, 6)), origin=(-1.0, -1.0), cell=1.0)
    r = tt.rollout(m, p, f["x"], f["feet"], f["stamp"], f["v_ref"], T, ft.COM, standing=f["standing"], push=ft.fleet_push(T, 6))
    assert np.array_equal(r["status"], flat["status"]) and np.array_equal(r["iters"], flat["iters"]) and np.array_equal(r["alive"], flat["alive"])
    worst = max(np.abs(r[k] - flat[k]).max() for k in ("x", "feet"))
    print("zero map against the flat twin over", T, "steps:", worst)
    assert worst < 1e-8, worst
    assert np.all(r["normals"] == np.tile([0.0, 0.0, 1.0], 4)) and np.any(r["feet"][-1] != r["feet"][0])


@pytest.fixture(scope="module")
def slope():
    g = tt.slope_fleet((0.4, 0.0))
    m = tt.plane(0.4, 0.0, nx=9, ny=9, origin=(-1.0, -2.0), cell=0.5)
    p = si.params(N)
    return g, m, p, tt.rollout(m, p, g["x"], g["feet"], g["stamp"], g["v_ref"], 24, ft.COM, standing=g["standing"])


def test_the_fleet_walks_up_the_slope(slope):
    g, m, p, r = slope
    assert r["alive"].tolist() == [1] * 4 and np.all(r["status"] == 1)
    x = r["x"]
    over = x[:, :, 5] - 0.4 * x[:, :, 3]
    print("slope 0.4: tilt", np.abs(x[:, :, 0:2]).max(), "height over ground", over.min(), over.max())
    assert np.abs(x[:, :, 0:2]).max() < 0.06 and 0.56 < over.min() and over.max() < 0.61
    assert np.all(x[-1, 2:, 3] - x[0, 2:, 3] > 0.1)                          # the walkers walk uphill
    moved = np.any(r["feet"][-1] != r["feet"][0], axis=1)
    assert moved.tolist() == [False, True, True, True]
    ft_ = r["feet"].reshape(25, 4, 4, 3)
    assert np.abs(ft_[..., 2] - 0.4 * ft_[..., 0]).max() < 1e-15              # every foothold stands on the plane
    s = np.sqrt(1.16)
    assert np.abs(r["normals"].reshape(-1, 3) - np.array([-0.4, 0.0, 1.0]) / s).max() < 1e-15


def test_the_slope_matters_to_the_solve(slope):
    """At some step the flat-normal solve of the same inputs differs from the solve with the map's normals by more than 1 N, and leaves the tilted pyramids by
    more than 1 N (19.8 N and 28 N when the case was fixed)."""
    g, m, p, r = slope
    worst_du, worst_out = 0.0, 0.0
    for t in (0, 6, 12):
        inp, normals = r["inputs"][t], r["normals"][t]
        x = r["x"][t]
        flat = tt.solve(p, x, inp, None)
        for b in range(4):
            worst_du = max(worst_du, np.abs(flat["u0"][b] - r["u0"][t, b]).max())
            tw = si.twin(p, x[b], inp["x_ref"][b], inp["foot"][b], inp["contact"][b], normals=normals[b], pcom=inp["pcom"][b])
            worst_out = max(worst_out, si.cone_violation(p, tw["qp_loc"], tw["T"], flat["u"][b]) * p.force_scale)
    print("flat-normal solve: first-step forces differ by", worst_du, "N; it leaves the tilted pyramids by", worst_out, "N")
    assert worst_du > 1.0 and worst_out > 1.0
