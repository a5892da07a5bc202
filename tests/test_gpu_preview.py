"""GPU tests of the previewed fleet calls (include/srbdqp_cascade.h srbdqp_mpc_inputs_previewed_*, srbdqp_terrain_inputs_previewed_*,
srbdqp_fleet_rollout_previewed_*) against the NumPy twin of tests/preview_twin.py (tests/test_preview_cpu.py holds the twin itself).

Bounds: those of test_gpu_steer.py and test_gpu_track.py.  What passes through no sine or cosine is compared bit for bit -- the contact schedule, previewed,
the points that are not previewed, the z of a previewed point, everything the steered or tracked call writes too (against the device's own call).  Heel and toe
of a previewed point: 1e-12 absolute -- the device's sin / cos against NumPy's at arguments below 10, on values of order 1, through at most 24 sums.  On a map
the heights are bit for bit and the normals within 1e-15 (test_gpu_terrain.py).  Free-running trajectories: 1e-4 with every iteration count equal to the
twin's (test_gpu_steer.py's bar at 50 steps; here 14).  Device against device -- the loop against the public calls, chunks, the step-1 property -- bit for bit."""
import ctypes as C

import numpy as np
import pytest

import c_oracle  # noqa: F401
import srbd_oracle as orc
import fleet_twin as ft
from fleet_loop import OBS, _bits, crowd, device_loop, direct_rollout, engine, inputs_device
import preview_twin as pvt
import steer_twin as stw
import terrain_twin as tt
import track_twin as ttw

pytestmark = pytest.mark.gpu
N, DT = 10, 0.04
OUTS = ("x_ref", "foot", "contact", "pcom", "landing", "landing_yaw")


def _foot_against_the_twin(got, want, what):
    """previewed and what is not previewed bit for bit, z of a previewed point exactly 0, its xy within 1e-12 -> the largest difference"""
    assert np.array_equal(got["previewed"], want["previewed"]), what
    on = np.repeat(want["previewed"] == 1, 3, axis=2)
    assert np.array_equal(_bits(got["foot"][~on]), _bits(want["foot"][~on])), what
    B, n = want["previewed"].shape[0:2]
    g, w = got["foot"].reshape(B, n, 4, 3)[want["previewed"] == 1], want["foot"].reshape(B, n, 4, 3)[want["previewed"] == 1]
    assert np.all(g[:, 2] == 0.0) and np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w)), what
    with np.errstate(invalid="ignore"):
        d = np.abs(g - w)
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


@pytest.mark.parametrize("horizon,P,ds", [(10, 6, 1), (24, 3, 0), (15, 6, 1), (1, 6, 1), (10, 4, 4)])
def test_previewed_inputs_against_the_twin(horizon, P, ds):
    """B = 1, 33 and 65 (a part tile, a tile and one robot, two tiles and one), steered and tracked: at (N, P, ds) = (10, 6, 1) one or two touchdowns in the
    horizon, at (24, 3, 0) a foot lands four times, (15, 6, 1) is the live-horizon text, (1, 6, 1) and (10, 4, 4) have no touchdown.  Against the twin; every
    output but foot against the device's own steered or tracked call, bit for bit; a command that is not finite spoils its robot's rows and no other's."""
    gait = dict(period_steps=P, double_support_steps=ds)
    worst, landed = 0.0, 0
    with engine(horizon) as e:
        for B in (1, 33, 65):
            c = crowd("preview", B, 500 + 10 * horizon + B, P=P)
            for flavour in ("steered", "tracked"):
                tracked = flavour == "tracked"
                got = inputs_device(e, c, horizon, flavour, preview=True, **gait)
                assert e.kernel_name() == ("mpc_inputs_tracked_previewed_f64" if tracked else "mpc_inputs_previewed_f64")
                plain = inputs_device(e, c, horizon, flavour, **gait)
                want = pvt.mpc_inputs(c["x"], c["feet"], c["stamp"], c["command"], ft.COM, horizon, DT, pose=c["pose"] if tracked else None, standing=c["standing"],
                                      **gait)
                worst = max(worst, _foot_against_the_twin(got, want, (B, tracked)))
                landed += int(want["previewed"].sum())
                for k in plain:                                   # untouched: x_ref, pcom, contact, landing, landing_yaw (and the pose)
                    if k != "foot":
                        assert np.array_equal(_bits(got[k]), _bits(plain[k])), (k, B, tracked)
                assert np.array_equal(got["contact"], want["contact"])
                off = np.repeat(got["previewed"] == 0, 3, axis=2)
                assert np.array_equal(_bits(got["foot"][off]), _bits(plain["foot"][off]))
                if ds >= P or horizon == 1:
                    assert not got["previewed"].any() and np.array_equal(_bits(got["foot"]), _bits(plain["foot"]))
                assert not got["previewed"][c["standing"] == 1].any() and not got["previewed"][:, 0].any()
                if B < 33:
                    continue
                # a command that is not finite: its robot's previewed points are not numbers, every other robot's rows are what they were
                bad = {k: v.copy() for k, v in c.items()}
                bad["command"][5, 2] = np.nan; bad["command"][32, 0] = np.inf
                spoiled = inputs_device(e, bad, horizon, flavour, preview=True, **gait)
                rest = np.setdiff1d(np.arange(B), [5, 32])
                for k in got:
                    assert np.array_equal(_bits(spoiled[k][rest]), _bits(got[k][rest])), (k, B, tracked)
                assert np.array_equal(spoiled["previewed"], got["previewed"]) and np.array_equal(spoiled["contact"], got["contact"])
                for b in (5, 32):
                    on = np.repeat(got["previewed"][b] == 1, 3, axis=1)
                    xy = spoiled["foot"][b][on].reshape(-1, 3)[:, 0:2]
                    assert not np.isfinite(xy).any() or not on.any(), b
                    assert np.array_equal(_bits(spoiled["foot"][b][~on]), _bits(got["foot"][b][~on]))
        # the host form against the device form
        c = crowd("preview", 33, 77, P=P)
        a = e.mpc_inputs_previewed(c["x"], c["feet"], c["stamp"], c["command"], ft.COM, standing=c["standing"], **gait)
        b = inputs_device(e, c, horizon, "steered", preview=True, **gait)
        for k in b:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
        a = e.mpc_inputs_previewed(c["x"], c["feet"], c["stamp"], c["command"], ft.COM, pose=c["pose"], standing=c["standing"], **gait)
        b = inputs_device(e, c, horizon, "tracked", preview=True, **gait)
        for k in b:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    print("previewed inputs against the twin, (N, P, ds) =", (horizon, P, ds), "heel / toe", worst, "previewed contacts", landed)
    assert worst <= 1e-12, worst
    assert (landed > 0) == (ds < P and horizon > 1)


def test_host_form_refusals_leave_the_outputs_untouched():
    """The host forms refuse bad preview settings, what the tracked and steered calls refuse, and -- in a roll-out -- a foot_half_length that differs from the
    fleet settings' before any launch: every output array keeps what it held."""
    from g1_locomotion_amd import _lib, SrbdqpError
    B, T = 6, 3
    c = crowd("preview", B, 3)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with engine(N) as e:
        lib, h = e._lib, e._h
        g = e._gait_struct(6, 1, ft.COM, 0.0645)
        outs = [np.full(s, 7.0) for s in ((B, N, 13), (B, N, 12))] + [np.full((B, N, 4), 7, np.uint8), np.full((B, N, 3), 7.0), np.full((B, 3), 7.0), np.full(B, 7.0)]
        pv = np.full((B, N, 4), 7, np.uint8)
        call = lambda cmd, trk, pose, prv: lib.srbdqp_mpc_inputs_previewed_f64(h, B, p(c["x"]), p(c["feet"]), p(c["stamp"]), p(cmd), p(c["standing"]), C.byref(g),
                                                                               *(p(o) for o in outs), trk, pose, prv, p(pv))
        trk, good = e.track_settings(), e.preview_settings()
        nanc = c["command"].copy(); nanc[2, 1] = np.nan
        nanp = c["pose"].copy(); nanp[4, 0] = np.inf
        for args in ((c["command"], None, None, C.byref(_lib.PreviewSettings(8, 0, 0.085))), (c["command"], None, None, C.byref(e.preview_settings(0.0))),
                     (c["command"], None, None, C.byref(e.preview_settings(np.nan))), (c["command"], None, None, None), (nanc, None, None, C.byref(good)),
                     (c["command"], C.byref(trk), None, C.byref(good)), (c["command"], C.byref(trk), p(nanp), C.byref(good)),
                     (c["command"], C.byref(e.track_settings(lead_max=-1.0)), p(c["pose"]), C.byref(good))):
            assert call(*args) == _lib.E_INVALID
            assert all(np.all(o == 7) for o in outs) and np.all(pv == 7)
        assert call(c["command"], None, None, C.byref(good)) == _lib.OK and not any(np.any(o == 7.0) for o in outs[:2]) and pv.max() <= 1
        # the roll-out: the MPC would preview another foot than the plant puts down
        s = e.fleet_settings(ft.COM)
        x, feet, stamp = c["x"].copy(), c["feet"].copy(), c["stamp"].copy()
        xl = np.full((T + 1, B, 13), 7.0)
        roll = lambda prv, trk=None, pose=None: lib.srbdqp_fleet_rollout_previewed_f64(h, B, T, p(x), p(feet), p(stamp), p(c["command"]), 1, p(c["standing"]), None,
                                                                                       C.byref(s), None, p(xl), None, None, None, None, None, None, None, trk, pose,
                                                                                       None, prv)
        assert roll(C.byref(e.preview_settings(0.09))) == _lib.E_INVALID and "foot_half_length differs" in e._lib.srbdqp_last_error(h).decode()
        assert roll(C.byref(e.preview_settings(-1.0))) == _lib.E_INVALID and roll(None) == _lib.E_INVALID
        assert roll(C.byref(good), C.byref(trk), None) == _lib.E_INVALID
        assert np.all(xl == 7.0) and np.array_equal(x, c["x"]) and np.array_equal(feet, c["feet"]) and np.array_equal(stamp, c["stamp"])
        # what the roll-out it becomes refuses: a wrench set on the engine
        e.set_external_wrench(np.full((B, N, 6), 0.5))
        try:
            with pytest.raises(SrbdqpError, match="srbdqp_set_external_wrench"):
                e.rollout(c["x"], c["feet"], c["stamp"], None, T, ft.COM, command=c["command"], preview=True)
        finally:
            e.set_external_wrench(None)
        assert roll(C.byref(good)) == _lib.OK and not np.any(xl == 7.0)
        with pytest.raises(ValueError, match="preview="):
            e.rollout(c["x"], c["feet"], c["stamp"], c["command"][:, 0:2], T, ft.COM, preview=True)


def test_terrain_inputs_previewed_against_the_twin():
    """B = 33 (a tile and one robot) on test_gpu_terrain.py's rough 17 x 9 map: foot's heights and x_ref bit for bit, normals within 1e-15; with previewed all
    zero, or NULL, the outputs are srbdqp_terrain_inputs_*'s on foot[:, 0]; host and device forms agree; without a map the call is refused."""
    import torch
    from g1_locomotion_amd import SrbdqpError
    m = tt.rough(17, 9, seed=11, cell=0.25, origin=(-1.0, -1.0))
    B = 33
    c = crowd("preview", B, 41)
    c["x"][:, 3] += np.linspace(-0.4, 1.6, B); c["feet"][:, 0::3] += np.linspace(-0.4, 1.6, B)[:, None]
    c["feet"].reshape(B, 4, 3)[:, :, 2] = tt.sample(m, c["feet"].reshape(B * 4, 3)[:, 0:2])[0].reshape(B, 4) + 0.01       # (the z handed in need not lie on the map)
    want_in = pvt.mpc_inputs(c["x"], c["feet"], c["stamp"], c["command"], ft.COM, N, DT, standing=c["standing"])
    x_ref = np.random.default_rng(B).normal(size=(B, N, 13))
    dev = torch.device("cuda", 0)
    with engine(N) as e:
        with pytest.raises(SrbdqpError, match="no terrain is set"):
            e.terrain_inputs_previewed(want_in["foot"], want_in["previewed"], x_ref)
        e.set_terrain(**m.args())
        got = e.terrain_inputs_previewed(want_in["foot"], want_in["previewed"], x_ref)
        assert e.kernel_name() == "terrain_inputs_previewed_f64"
        want = pvt.terrain_inputs(m, want_in["foot"], want_in["previewed"], x_ref)
        assert want_in["previewed"].any() and np.any(want["foot"] != want_in["foot"])
        assert np.array_equal(_bits(got["foot"]), _bits(want["foot"])) and np.array_equal(_bits(got["x_ref"]), _bits(want["x_ref"]))
        assert np.array_equal(_bits(np.delete(got["x_ref"], 5, axis=2)), _bits(np.delete(x_ref, 5, axis=2)))
        err = np.abs(got["normals"] - want["normals"]).max()
        print("terrain inputs previewed: normals max |gpu - twin|", err)
        assert err <= 1e-15, err
        # nothing previewed: the terrain inputs on foot[:, 0]
        old = e.terrain_inputs(c["feet"], x_ref)
        rep = np.repeat(c["feet"][:, None, :], N, axis=1)
        for pv in (np.zeros((B, N, 4), np.uint8), None):
            z = e.terrain_inputs_previewed(rep, pv, x_ref)
            assert np.array_equal(_bits(z["x_ref"]), _bits(old["x_ref"])) and np.array_equal(_bits(z["normals"]), _bits(old["normals"]))
            assert np.array_equal(_bits(z["foot"]), _bits(rep))
        # the device form
        dfo, dpv, dxr = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (want_in["foot"], want_in["previewed"], x_ref))
        dcn = torch.full((B, N, 12), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()                                  # (torch's stream is not the engine's)
        e.terrain_inputs_previewed_device(B, dfo.data_ptr(), dpv.data_ptr(), dxr.data_ptr(), dcn.data_ptr())
        e.synchronize()
        for k, a in dict(foot=dfo, x_ref=dxr, normals=dcn).items():
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(got[k])), k


# ---- the roll-out ----
T14 = 14


def _fleet(mode):
    f = stw.fleet()
    if mode == "terrain":
        z = lambda p: 0.2 * p[..., 0] + 0.1 * p[..., 1]
        feet = f["feet"].reshape(-1, 4, 3)
        feet[:, :, 2] = z(feet)
        f["feet"] = feet.reshape(-1, 12)
        f["x"][:, 5] += z(f["x"][:, 3:5])
    return f


def _slope():
    return tt.plane(0.2, 0.1, nx=17, ny=17, origin=(-2.0, -2.0), cell=0.5)


def _rollout(e, f, steps, mode, **kw):
    more = dict(track=True) if mode == "track" else dict(observer=OBS) if mode == "observer" else {}
    return e.rollout(f["x"], f["feet"], f["stamp"], None, steps, ft.COM, standing=f["standing"], command=f["command"], preview=True, **more, **kw)


@pytest.mark.parametrize("mode", ["flat", "terrain", "observer", "track"])
def test_the_previewed_rollout(mode):
    """The 6-robot steering fleet, N = 10, T = 14 (two touchdowns per foot) -- on flat ground, on a slope, with the observer, tracked: rollout(preview=True)
    is the public calls driven step by step, bit for bit; two chunks of 7 compose bit for bit; and the step-1 property on the device: a previewed inputs call
    on the logged state of step t puts foot[:, 1] of the robots whose foot lands in period t where feet_log[t + 1] has it, bit for bit (on the slope with z)."""
    f = _fleet(mode)
    B = f["x"].shape[0]
    with engine(N) as e:
        if mode == "terrain":
            e.set_terrain(**_slope().args())
        whole = _rollout(e, f, T14, mode)
        # (the loop from where the host form starts: the measured pose, no estimate, every robot alive, no pushes)
        _, loop, _ = device_loop(e, dict(f, pose=ttw.start_pose(f["x"]), w0=np.zeros((B, 6))), B, T14, "flat" if mode == "track" else mode, observer=OBS,
                                 track=True if mode == "track" else None, preview=True, dead=False, call=False)
        for k, lk in dict(x="x_log", feet="feet_log", u0="u0_log", status="status_log", iters="iters_log", stamp="stamp", alive="alive").items():
            assert np.array_equal(_bits(whole[k]), _bits(loop[lk])), k
        assert whole["alive"].tolist() == [1] * B and (whole["status"] == 1).mean() > 0.9
        # chunks
        a = _rollout(e, f, 7, mode)
        carry = dict(alive=a["alive"], **(dict(pose=a["pose"]) if mode == "track" else {}), **(dict(w_est=a["w_est"]) if mode == "observer" else {}))
        g = dict(f, x=a["x"][-1], feet=a["feet"][-1], stamp=a["stamp"])
        b = _rollout(e, g, 7, mode, **carry)
        for k in ("x", "feet"):
            assert np.array_equal(_bits(np.concatenate([a[k], b[k][1:]])), _bits(whole[k])), k
        for k in ("u0", "status", "iters") + (("pose_log",) if mode == "track" else ()) + (("w_log",) if mode == "observer" else ()):
            assert np.array_equal(_bits(np.concatenate([a[k], b[k]])), _bits(whole[k])), k
        # the preview changes what the solves read: another trajectory than the roll-out without it
        more = dict(track=True) if mode == "track" else dict(observer=OBS) if mode == "observer" else {}
        off = e.rollout(f["x"], f["feet"], f["stamp"], None, T14, ft.COM, standing=f["standing"], command=f["command"], **more)
        assert np.any(off["u0"] != whole["u0"])
        # the step-1 property, from the logs
        stamp, checked = f["stamp"].copy(), 0
        for t in range(T14):
            inp = e.mpc_inputs_previewed(whole["x"][t], whole["feet"][t], stamp, f["command"], ft.COM, standing=f["standing"])
            foot = e.terrain_inputs_previewed(inp["foot"], inp["previewed"], inp["x_ref"])["foot"] if mode == "terrain" else inp["foot"]
            for r, i in zip(*np.nonzero(inp["previewed"][:, 1] == 1)):
                assert np.array_equal(_bits(foot[r, 1, 3 * i:3 * i + 3]), _bits(whole["feet"][t + 1, r, 3 * i:3 * i + 3])), (t, r, i)
                checked += 1
            moved = np.any(whole["feet"][t + 1].reshape(B, 4, 3) != whole["feet"][t].reshape(B, 4, 3), axis=2)
            assert np.array_equal(moved, inp["previewed"][:, 1] == 1), t
            stamp = stamp + DT
        assert checked >= 2 * 2 * B
    print("previewed roll-out,", mode, ": contacts checked against the plant", checked)


@pytest.mark.parametrize("track", [False, True])
def test_free_running_against_the_twin(track):
    """The six robots over 14 steps, the engine and the twin with the C solver each on its own trajectory: every robot alive on both, statuses and iteration
    counts equal, states within 1e-4 -- test_gpu_steer.py's bounds for its roll-outs."""
    f = stw.fleet()
    want = pvt.rollout(orc.default_params(N), f["x"], f["feet"], f["stamp"], f["command"], T14, ft.COM, track=track, standing=f["standing"], solver="c")
    with engine(N) as e:
        got = _rollout(e, f, T14, "track" if track else "flat")
    err = np.abs(got["x"] - want["x"]).max(axis=(0, 2))
    efeet = np.abs(got["feet"] - want["feet"]).max()
    print("free-running previewed, track =", track, ": max |x - twin| per robot", err.tolist(), "feet", efeet,
          "steps with other iters", (got["iters"] != want["iters"]).sum(axis=0).tolist())
    assert got["alive"].tolist() == [1] * 6 and want["alive"].tolist() == [1] * 6
    assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["status"], want["status"])
    assert err.max() < 1e-4 and efeet < 1e-4, (err, efeet)
    assert want["previewed"].any()


def test_preview_off_is_the_rollout_as_it_was():
    """rollout(command=, preview=None), steered and tracked, against srbdqp_fleet_rollout_steered_f64 and srbdqp_fleet_rollout_tracked_f64 called directly --
    before and after a previewed roll-out has run on the engine (which re-carves the roll-out allocation): bit for bit, twice."""
    steps, B = T14, 6
    f = stw.fleet()
    f["pose"] = ttw.start_pose(f["x"])                            # (where rollout(track=True) starts without a pose)
    first = {}
    with engine(N) as e:
        for round_ in range(2):
            for tracked in (False, True):
                want = direct_rollout(e, "srbdqp_fleet_rollout_tracked_f64" if tracked else "srbdqp_fleet_rollout_steered_f64", f, steps, f["command"])
                got = e.rollout(f["x"], f["feet"], f["stamp"], None, steps, ft.COM, standing=f["standing"], command=f["command"], track=True if tracked else None,
                                preview=None)
                for k, v in want.items():
                    assert np.array_equal(_bits(got[k]), _bits(v)), (k, tracked, round_)
                if round_ == 0:
                    first[tracked] = want
                else:
                    for k, v in want.items():
                        assert np.array_equal(_bits(first[tracked][k]), _bits(v)), (k, tracked)
            _rollout(e, f, 3, "flat")                             # a previewed roll-out in between
