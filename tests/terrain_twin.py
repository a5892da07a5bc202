"""Test helper: the NumPy twin of the fleet roll-out over terrain (include/srbdqp_cascade.h srbdqp_set_terrain, srbdqp_terrain_sample_*, srbdqp_terrain_inputs_*;
DESIGN.md section 18).

sample() is S(x, y) -> (z, n) in the header's operation order, one rounded float64 operation per step (NumPy never fuses a multiply with an add).  advance() and
rollout() are fleet_twin's with the two rules of the terrain plant step -- a foot that touches down stands at S(own xy).z, heel and toe each; both "fallen" tests
compare x[5] - S(com xy).z with z_min -- and the inputs step between cascade_oracle.mpc_inputs and the solve: the normals under the footholds and the height
reference raised by the mean foothold height.  The solve is side_inputs.twin(..., normals=, pcom=)."""
import numpy as np

import cascade_oracle as co
import fleet_twin as ft
import side_inputs as si
from fleet_twin import DEFAULTS, PushedPlant, first_step_flags
import srbd_oracle as orc


class Map:
    """heights (ny, nx), node (i, j) = heights[j, i] at (origin[0] + i cell, origin[1] + j cell)."""

    def __init__(self, heights, origin=(0.0, 0.0), cell=1.0):
        self.h = np.ascontiguousarray(heights, np.float64)
        assert self.h.ndim == 2 and min(self.h.shape) >= 2
        self.ny, self.nx = self.h.shape
        self.x0, self.y0, self.cell = np.float64(origin[0]), np.float64(origin[1]), np.float64(cell)

    def args(self):
        """What BatchMPC.set_terrain takes."""
        return dict(heights=self.h, origin=(float(self.x0), float(self.y0)), cell=float(self.cell))


def plane(sx, sy, z0=0.0, nx=9, ny=9, origin=(-1.0, -1.0), cell=0.5):
    """z = z0 + sx x + sy y sampled on a grid."""
    x = origin[0] + cell * np.arange(nx)
    y = origin[1] + cell * np.arange(ny)
    return Map(z0 + sx * x[None, :] + sy * y[:, None], origin, cell)


def rough(nx, ny, seed, cell=0.25, origin=(-1.0, -1.0), amp=0.5):
    """A seeded rough map: a random walk along x and along y whose neighbour differences stay within amp * cell."""
    rng = np.random.default_rng(seed)
    dx = rng.uniform(-amp * cell, amp * cell, nx)
    dy = rng.uniform(-amp * cell, amp * cell, ny)
    return Map(np.cumsum(dx)[None, :] + np.cumsum(dy)[:, None], origin, cell)


def sample(m, xy):
    """S at the points xy (M, 2) -> z (M,), n (M, 3)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    fin = np.isfinite(x) & np.isfinite(y)
    xs, ys = np.where(fin, x, m.x0), np.where(fin, y, m.y0)
    with np.errstate(over="ignore"):
        u = (xs - m.x0) / m.cell
        v = (ys - m.y0) / m.cell
    u = np.where(u < 0.0, 0.0, np.where(u > m.nx - 1.0, m.nx - 1.0, u))
    v = np.where(v < 0.0, 0.0, np.where(v > m.ny - 1.0, m.ny - 1.0, v))
    i = np.minimum(np.floor(u).astype(np.int64), m.nx - 2)
    j = np.minimum(np.floor(v).astype(np.int64), m.ny - 2)
    fx, fy = u - i.astype(np.float64), v - j.astype(np.float64)
    h00, h10, h01, h11 = m.h[j, i], m.h[j, i + 1], m.h[j + 1, i], m.h[j + 1, i + 1]
    dx0, dx1, dy0, dy1 = h10 - h00, h11 - h01, h01 - h00, h11 - h10
    a = h00 + fx * dx0
    b = h01 + fx * dx1
    z = a + fy * (b - a)
    gx = (dx0 + fy * (dx1 - dx0)) / m.cell
    gy = (dy0 + fx * (dy1 - dy0)) / m.cell
    s = np.sqrt((gx * gx + gy * gy) + 1.0)
    n = np.stack([-gx / s, -gy / s, 1.0 / s], -1)
    z = np.where(fin, z, np.nan)
    n[~fin] = (0.0, 0.0, 1.0)
    return z, n


def inputs(m, feet, x_ref):
    """The twin of srbdqp_terrain_inputs_*: feet (B, 12), x_ref (B, N, 13) -> dict(x_ref, normals (B, N, 12))."""
    feet = np.asarray(feet, np.float64).reshape(-1, 12)
    B = feet.shape[0]
    x_ref = np.array(x_ref, np.float64).reshape(B, -1, 13)
    N = x_ref.shape[1]
    _, n = sample(m, feet.reshape(B * 4, 3)[:, 0:2])
    normals = np.repeat(n.reshape(B, 1, 12), N, axis=1)
    zg = (((feet[:, 2] + feet[:, 5]) + feet[:, 8]) + feet[:, 11]) * 0.25
    x_ref[:, :, 5] = x_ref[:, :, 5] + zg[:, None]
    return dict(x_ref=x_ref, normals=normals)


def advance(m, params, x, feet, stamp, u0, landing, standing=None, push=None, alive=None, robots=None, **settings):
    """fleet_twin.advance on the map m: the same operations in the same order, except the touchdown's z and the height the two fallen tests compare."""
    s = dict(DEFAULTS, **settings)
    x = np.array(x, np.float64).reshape(-1, 13)
    B = x.shape[0]
    feet = np.array(feet, np.float64).reshape(B, 12)
    stamp = np.array(stamp, np.float64).reshape(B)
    u0 = np.asarray(u0, np.float64).reshape(B, 12)
    landing = np.asarray(landing, np.float64).reshape(B, 3)
    standing = np.zeros(B, np.uint8) if standing is None else np.asarray(standing).reshape(B)
    alive = np.ones(B, np.uint8) if alive is None else np.array(np.asarray(alive) != 0, np.uint8).reshape(B)
    dt = params.dt
    stamp1 = stamp + dt
    l0, r0 = first_step_flags(stamp, dt, standing, s["period_steps"], s["double_support_steps"])
    l1, r1 = first_step_flags(stamp1, dt, standing, s["period_steps"], s["double_support_steps"])
    moved = np.zeros(B, np.int32)
    h = dt / s["substeps"]
    fhl = s["foot_half_length"]
    over = lambda xb: xb[5] - sample(m, xb[3:5])[0][0]                        # the CoM's height over the ground under it
    for b in range(B):
        if not alive[b] or not np.all(np.isfinite(x[b])):                     # 1. skip
            alive[b] = 0
            continue
        p = params
        if robots is not None:
            p = orc.SrbdParams(dt=dt, mass=float(robots[b, 0]), inertia=tuple(float(v) for v in robots[b, 1:4]))
        plant = PushedPlant(p)
        plant.push = None if push is None else np.asarray(push, np.float64).reshape(B, 6)[b]
        xb, fb = x[b], feet[b].reshape(4, 3).copy()
        outside0 = over(xb) < s["z_min"] or abs(xb[0]) > s["tilt_max"] or abs(xb[1]) > s["tilt_max"]
        for _ in range(s["substeps"]):                                        # 2. plant
            xb = plant.step(xb, fb, u0[b], h)
        x[b] = xb
        side = 1 if (not l0[b] and l1[b]) else 2 if (not r0[b] and r1[b]) else 0
        if side:                                                              # 4. touchdown: heel and toe each on the ground under them
            c0 = 0 if side == 1 else 6
            heel = np.array([landing[b, 0] - fhl, landing[b, 1]])
            toe = np.array([landing[b, 0] + fhl, landing[b, 1]])
            zz, _ = sample(m, np.stack([heel, toe]))
            feet[b, c0:c0 + 3] = (heel[0], heel[1], zz[0])
            feet[b, c0 + 3:c0 + 6] = (toe[0], toe[1], zz[1])
            moved[b] = side
        if outside0 or not np.all(np.isfinite(xb)) or over(xb) < s["z_min"] or abs(xb[0]) > s["tilt_max"] or abs(xb[1]) > s["tilt_max"]:   # 5. fallen
            alive[b] = 0
    return dict(x=x, feet=feet, stamp=stamp1, alive=alive, moved=moved)


def solve(params, x, inp, normals):
    """The QPs of one control step on the twin of the solve with normals -> dict(u0 (B,12), u (B,N,12), status, iters)."""
    out = [si.twin(params, x[b], inp["x_ref"][b], inp["foot"][b], inp["contact"][b], normals=None if normals is None else normals[b], pcom=inp["pcom"][b])
           for b in range(x.shape[0])]
    return dict(u0=np.stack([o["u"][0] for o in out]), u=np.stack([o["u"] for o in out]), status=np.array([o["status"] for o in out], np.int32),
                iters=np.array([o["iters"] for o in out], np.int32))


def step_inputs(m, params, x, feet, stamp, v_ref, com_target, N, standing=None, **settings):
    """mpc_inputs -> terrain inputs of one control step -> (inp with x_ref raised, normals)."""
    s = dict(DEFAULTS, **settings)
    inp = co.mpc_inputs(x, feet, stamp, v_ref, com_target, N, params.dt, standing=standing, period_steps=s["period_steps"],
                        double_support_steps=s["double_support_steps"], hip_offset_y=s["hip_offset_y"])
    ti = inputs(m, feet, inp["x_ref"])
    return dict(inp, x_ref=ti["x_ref"]), ti["normals"]


def rollout(m, params, x0, feet, stamp, v_ref, steps, com_target, standing=None, push=None, alive=None, horizon=10, **settings):
    """The twin of srbdqp_fleet_rollout_* with a map set: fleet_twin.rollout's dict, plus normals (T,B,N,12) and x_ref5 (T,B): the height references."""
    x = np.array(x0, np.float64).reshape(-1, 13)
    B, N = x.shape[0], int(horizon)
    feet = np.array(feet, np.float64).reshape(B, 12)
    stamp = np.array(stamp, np.float64).reshape(B)
    alive = np.ones(B, np.uint8) if alive is None else np.array(np.asarray(alive) != 0, np.uint8).reshape(B)
    xs, fs, us, st, it, lps, ns, zr, uall, inps = [x.copy()], [feet.copy()], [], [], [], [], [], [], [], []
    for t in range(steps):
        inp, normals = step_inputs(m, params, x, feet, stamp, v_ref, com_target, N, standing=standing, **settings)
        sol = solve(params, x, inp, normals)
        r = advance(m, params, x, feet, stamp, sol["u0"], inp["landing"], standing=standing, push=None if push is None else push[t], alive=alive, **settings)
        x, feet, stamp, alive = r["x"], r["feet"], r["stamp"], r["alive"]
        xs.append(x.copy()); fs.append(feet.copy()); us.append(sol["u0"]); st.append(sol["status"]); it.append(sol["iters"]); lps.append(inp["landing"])
        ns.append(normals); zr.append(inp["x_ref"][:, 0, 5].copy()); uall.append(sol["u"]); inps.append(inp)
    return dict(x=np.array(xs), u0=np.array(us), feet=np.array(fs), status=np.array(st), iters=np.array(it), landing=np.array(lps), alive=alive, stamp=stamp,
                normals=np.array(ns), x_ref5=np.array(zr), u=np.array(uall), inputs=inps)


def slope_fleet(slope=(0.4, 0.0), robots=(0, 1, 2, 5)):
    """Robots 0, 1, 2 and 5 of fleet_twin.fleet() standing on the plane z = slope . (x, y): CoM and footholds raised by the ground under them."""
    f = ft.fleet()
    idx = list(robots)
    g = {k: np.array(v[idx]) for k, v in f.items()}
    z = lambda p: slope[0] * p[..., 0] + slope[1] * p[..., 1]
    feet = g["feet"].reshape(-1, 4, 3)
    feet[:, :, 2] = z(feet)
    g["feet"] = feet.reshape(-1, 12)
    g["x"][:, 5] += z(g["x"][:, 3:5])
    return g
