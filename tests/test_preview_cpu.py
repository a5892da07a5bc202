"""CPU side of the previewed fleet calls (include/srbdqp_cascade.h srbdqp_mpc_inputs_previewed_*, srbdqp_terrain_inputs_previewed_*,
srbdqp_fleet_rollout_previewed_*): the library exports the calls and the binding lists them, the refusals that need no device, the
closed-form touchdown steps against a plain search over cascade_oracle's flags for every (P, ds, p0, N), the properties of the twin of tests/preview_twin.py --
above all that the foothold previewed for horizon step 1 is the one the plant puts down --, and a stand-alone host build of csrc/srbdqp_steer.hpp's
preview_lands, preview_touchdown and preview_foothold against the twin.

Bounds: what passes through no sine or cosine -- the touchdown steps, psi_L -- bit for bit; heel and toe of the host build within 1e-12 of the twin's (the C
library's sines against NumPy's on values of order 1: tests/test_steer_cpu.py's bound).  Inside one implementation the j = 1 property is bit for bit."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import cascade_oracle as co
import fleet_twin as ft
import preview_twin as pvt
import srbd_oracle as orc
import steer_twin as stw
import terrain_twin as tt
import track_twin as ttw

CALLS = ("srbdqp_preview_default_settings", "srbdqp_mpc_inputs_previewed_f64", "srbdqp_mpc_inputs_previewed_device_f64",
         "srbdqp_terrain_inputs_previewed_f64", "srbdqp_terrain_inputs_previewed_device_f64", "srbdqp_fleet_rollout_previewed_device_f64",
         "srbdqp_fleet_rollout_previewed_f64")
N, DT = 10, 0.04
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAITS = [(P, ds) for P in range(1, 9) for ds in range(0, P + 1)]
HORIZONS = (1, 2, 10, 24)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _draw(B, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 13)); x[:, 3:6] = ft.COM + rng.normal(size=(B, 3)) * 0.01; x[:, 0:2] = rng.normal(size=(B, 2)) * 0.02; x[:, 12] = -9.80665
    x[:, 2] = rng.uniform(-3.0, 3.0, B)
    x[:, 6:12] = rng.normal(size=(B, 6)) * 0.05
    feet = np.tile(ft.FEET.reshape(12), (B, 1)) + rng.normal(size=(B, 12)) * 0.01
    stamp = DT * (np.arange(B) % 12).astype(np.float64)
    cmd = rng.uniform(-1.0, 1.0, (B, 3)) * np.array([0.3, 0.1, 1.0])
    return x, feet, stamp, cmd


def test_the_library_exports_the_previewed_calls_and_the_binding_lists_them(built_lib):
    from g1_locomotion_amd import _lib, BatchMPC
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in CALLS:
        assert f" T {name}\n" in syms, name
        assert name in _lib.SIGNATURES and name in _lib.EXPORTS and getattr(built_lib, name).restype is C.c_int
    for method in ("mpc_inputs_previewed", "mpc_inputs_previewed_device", "terrain_inputs_previewed", "terrain_inputs_previewed_device", "preview_settings"):
        assert callable(getattr(BatchMPC, method))
    assert "preview" in inspect.signature(BatchMPC.rollout).parameters and "preview" in inspect.signature(BatchMPC.rollout_device).parameters
    s = _lib.PreviewSettings()
    assert C.sizeof(s) == 16
    assert built_lib.srbdqp_preview_default_settings(C.byref(s)) == _lib.E_INVALID        # struct_size 0: nothing written
    assert s.foot_half_length == 0.0
    s.struct_size = C.sizeof(s)
    assert built_lib.srbdqp_preview_default_settings(C.byref(s)) == _lib.OK and s.foot_half_length == 0.085
    assert built_lib.srbdqp_preview_default_settings(None) == _lib.E_INVALID


def test_refusals_that_need_no_device(built_lib):
    """A NULL handle is refused, not dereferenced; a wrong struct_size and a foot_half_length that is not finite and positive are refused before the handle is
    looked at, in both forms of both calls, steered (trk NULL) and tracked; so is what the tracked and the steered calls refuse there."""
    from g1_locomotion_amd import _lib
    lib = built_lib
    why = lambda: lib.srbdqp_last_error(None).decode()
    B, steps = 4, 5
    cmd = np.tile([0.2, 0.0, 0.3], (steps, B, 1))
    pose = np.zeros((B, 3))
    trk = _lib.TrackSettings(C.sizeof(_lib.TrackSettings), 0, 0.1, 0.3)
    prv = _lib.PreviewSettings(C.sizeof(_lib.PreviewSettings), 0, 0.085)
    inputs = lambda fn, c, k, po, pr, *tail: fn(None, B, *([None] * 3), c, *([None] * 8), k, po, pr, None, *tail)
    roll = lambda fn, c, cs, k, po, pr, *tail: fn(None, B, steps, None, None, None, c, cs, *([None] * 12), k, po, None, pr, *tail)
    forms = ((lib.srbdqp_mpc_inputs_previewed_f64, lib.srbdqp_fleet_rollout_previewed_f64, ()),
             (lib.srbdqp_mpc_inputs_previewed_device_f64, lib.srbdqp_fleet_rollout_previewed_device_f64, (None,)))
    for fin, fro, tail in forms:
        for k, po in ((None, None), (C.byref(trk), _p(pose))):
            # a NULL handle with everything else in order
            assert inputs(fin, _p(cmd[0]), k, po, C.byref(prv), *tail) == _lib.E_INVALID
            assert roll(fro, _p(cmd), 1, k, po, C.byref(prv), *tail) == _lib.E_INVALID and roll(fro, _p(cmd), steps, k, po, C.byref(prv), *tail) == _lib.E_INVALID
            # the settings
            assert inputs(fin, _p(cmd[0]), k, po, None, *tail) == _lib.E_INVALID and "srbdqp_preview_settings" in why() and "struct_size" in why()
            assert roll(fro, _p(cmd), 1, k, po, None, *tail) == _lib.E_INVALID and "srbdqp_preview_settings" in why() and "struct_size" in why()
            for size in (0, 8, 24):
                bad = _lib.PreviewSettings(size, 0, 0.085)
                assert inputs(fin, _p(cmd[0]), k, po, C.byref(bad), *tail) == _lib.E_INVALID and "struct_size" in why(), size
                assert roll(fro, _p(cmd), 1, k, po, C.byref(bad), *tail) == _lib.E_INVALID and "struct_size" in why(), size
            for v in (0.0, -0.1, np.nan, np.inf, -np.inf):
                bad = _lib.PreviewSettings(16, 0, v)
                assert inputs(fin, _p(cmd[0]), k, po, C.byref(bad), *tail) == _lib.E_INVALID and "finite and positive" in why() and "previewed" in why(), v
                assert roll(fro, _p(cmd), steps, k, po, C.byref(bad), *tail) == _lib.E_INVALID and "finite and positive" in why() and "previewed" in why(), v
        # the steered and the tracked roll-outs' own rules, in the previewed call's name
        assert roll(fro, None, 1, None, None, C.byref(prv), *tail) == _lib.E_INVALID and "command is NULL" in why() and "previewed" in why()
        for cs in (0, 2, steps + 1, -1):
            assert roll(fro, _p(cmd), cs, None, None, C.byref(prv), *tail) == _lib.E_INVALID and "command_steps" in why(), cs
        assert roll(fro, _p(cmd), 1, C.byref(trk), None, C.byref(prv), *tail) == _lib.E_INVALID and "pose is NULL" in why()
        assert inputs(fin, _p(cmd[0]), C.byref(trk), None, C.byref(prv), *tail) == _lib.E_INVALID and "pose is NULL" in why()
        bad = _lib.TrackSettings(24, 0, 0.0, 0.3)
        assert inputs(fin, _p(cmd[0]), C.byref(bad), _p(pose), C.byref(prv), *tail) == _lib.E_INVALID and "srbdqp_track_settings" in why()
    # the host forms: a command that is not finite, by robot, steered and tracked
    for bad in (np.nan, np.inf):
        c2 = cmd.copy(); c2[0, 1, 2] = bad
        for k, po in ((None, None), (C.byref(trk), _p(pose))):
            assert roll(lib.srbdqp_fleet_rollout_previewed_f64, _p(c2), 1, k, po, C.byref(prv)) == _lib.E_INVALID
            assert "command of robot 1" in why() and "not finite" in why()


def test_preview_without_a_command_is_a_value_error(built_lib):
    from g1_locomotion_amd import BatchMPC
    eng = BatchMPC.__new__(BatchMPC)          # (the checks under test come before the first use of the handle)
    with pytest.raises(ValueError, match="preview="):
        BatchMPC.rollout(eng, np.zeros((2, 13)), np.zeros((2, 12)), np.zeros(2), np.zeros((2, 2)), 3, ft.COM, preview=True)
    with pytest.raises(ValueError, match="preview="):
        BatchMPC.rollout_device(eng, 2, 3, 1, 1, 1, 1, ft.COM, preview=True)


# ---- the closed forms ----
def _search(flags):
    """The plain search: flags (N,) of one foot -> (lands (N,) bool, latest (N,) int): touchdown at j iff 1 <= j, flags[j - 1] == 0 and flags[j] == 1."""
    n = flags.shape[0]
    lands, latest, last = np.zeros(n, bool), np.zeros(n, np.int64), 0
    for j in range(n):
        if j >= 1 and flags[j - 1] == 0 and flags[j] == 1:
            lands[j], last = True, j
        latest[j] = last
    return lands, latest


def _all_gaits():
    """Every (P, ds, p0, N) -> (lands (N,) 0 / 1 / 2, left (N,), right (N,)) by the search over cascade_oracle's contact flags."""
    want = {}
    for P, ds in GAITS:
        B = 2 * P
        x = np.zeros((B, 13)); x[:, 12] = -9.80665
        ct = co.mpc_inputs(x, np.zeros((B, 12)), DT * np.arange(B, dtype=np.float64), np.zeros((B, 2)), ft.COM, max(HORIZONS), DT, period_steps=P,
                           double_support_steps=ds)["contact"]
        for p0 in range(B):
            assert np.array_equal(ct[p0, :, 0], ct[p0, :, 1]) and np.array_equal(ct[p0, :, 2], ct[p0, :, 3])
            for n in HORIZONS:
                ll, jl = _search(ct[p0, :n, 0])
                lr, jr = _search(ct[p0, :n, 2])
                assert not (ll & lr).any()                          # at most one foot touches down at a step
                want[(P, ds, p0, n)] = (ll * 1 + lr * 2, jl, jr)
    return want


def test_closed_form_touchdowns_against_a_search_over_the_flags():
    want = _all_gaits()
    assert len(want) == sum(2 * P * (P + 1) for P in range(1, 9)) * len(HORIZONS)
    some = 0
    for (P, ds, p0, n), (lands, jl, jr) in want.items():
        got = np.array([[pvt.lands(p0, k, P, ds), pvt.touchdown(p0, k, P, ds, False), pvt.touchdown(p0, k, P, ds, True)] for k in range(n)])
        assert np.array_equal(got[:, 0], lands) and np.array_equal(got[:, 1], jl) and np.array_equal(got[:, 2], jr), (P, ds, p0, n)
        if ds == P or n == 1:
            assert not got.any(), (P, ds, p0, n)                     # no swing, or no step behind the present: no touchdown
        some += int(lands.any())
    assert some > 500
    # a standing robot has none
    assert not any(pvt.lands(-1, k, 6, 1) or pvt.touchdown(-1, k, 6, 1, r) for k in range(24) for r in (False, True))


# ---- properties of the twin ----
def test_previewed_is_all_zero_where_nothing_lands_and_stamps_may_be_negative():
    B = 24
    x, feet, stamp, cmd = _draw(B, 1)
    plain = stw.mpc_inputs(x, feet, stamp, cmd, ft.COM, N, DT)
    for kw, n in ((dict(standing=np.ones(B, np.uint8)), N), (dict(), 1), (dict(period_steps=4, double_support_steps=4), N)):
        a = pvt.mpc_inputs(x, feet, stamp, cmd, ft.COM, n, DT, **kw)
        b = stw.mpc_inputs(x, feet, stamp, cmd, ft.COM, n, DT, **kw)
        assert not a["previewed"].any() and np.array_equal(_bits(a["foot"]), _bits(b["foot"])), kw
    a = pvt.mpc_inputs(x, feet, stamp, cmd, ft.COM, N, DT)
    assert a["previewed"].any() and not a["previewed"][:, 0].any()
    for k in ("x_ref", "contact", "pcom", "landing", "landing_yaw"):                      # untouched
        assert np.array_equal(_bits(a[k]), _bits(plain[k])), k
    assert np.array_equal(_bits(a["foot"][a["previewed"].repeat(3, axis=2) == 0]), _bits(plain["foot"][a["previewed"].repeat(3, axis=2) == 0]))
    # a contact is in stance at the step it becomes previewed, and stays previewed to the end of the horizon (a foot that swings again keeps its last point)
    first = np.diff(a["previewed"].astype(int), axis=1, prepend=0)
    assert np.all(first >= 0) and np.all(a["contact"][first == 1] == 1)
    # negative stamps: the phase wraps upwards, as the gait's does
    neg = stamp - 12 * DT * 3
    c = pvt.mpc_inputs(x, feet, neg, cmd, ft.COM, N, DT)
    assert np.array_equal(c["previewed"], a["previewed"]) and np.array_equal(_bits(c["foot"]), _bits(a["foot"]))
    assert np.array_equal(pvt.phase0(np.array([-DT, -12 * DT, -13 * DT]), DT, 6), [11, 0, 11])
    # a command that is not finite spoils its own robot's previewed points and no other's
    bad = cmd.copy(); bad[3, 2] = np.nan; bad[7, 0] = np.inf
    d = pvt.mpc_inputs(x, feet, stamp, bad, ft.COM, N, DT)
    rest = np.setdiff1d(np.arange(B), [3, 7])
    assert np.array_equal(_bits(d["foot"][rest]), _bits(a["foot"][rest])) and np.array_equal(d["previewed"], a["previewed"])
    # the tracked form: the same footholds, from the measured state
    t = pvt.mpc_inputs(x, feet, stamp, cmd, ft.COM, N, DT, pose=ttw.start_pose(x) + 0.02)
    assert np.array_equal(_bits(t["foot"]), _bits(a["foot"])) and np.array_equal(t["previewed"], a["previewed"]) and "pose" in t


@pytest.mark.parametrize("ground", ["flat", "slope"])
def test_the_foothold_previewed_for_step_1_is_the_one_the_plant_puts_down(ground):
    """40 steps of the twin roll-out: wherever a foot lands in period t, foot[:, 1] of solve t equals the feet behind the period, bit for bit -- on the slope
    with z --, and psi_L,1 == landing_yaw."""
    T = 40
    if ground == "flat":
        f, m = stw.fleet(), None
    else:
        f, m = tt.slope_fleet((0.2, 0.1), robots=(1, 2, 3, 4, 5)), tt.plane(0.2, 0.1, nx=17, ny=17, origin=(-2.0, -2.0), cell=0.5)
        f["command"] = stw.COMMANDS[[1, 2, 3, 4, 5]].copy(); f["standing"] = np.zeros(5, np.uint8)
    p = orc.default_params(N)
    r = pvt.rollout(p, f["x"], f["feet"], f["stamp"], f["command"], T, ft.COM, terrain=m, standing=f["standing"])
    B = f["x"].shape[0]
    assert r["alive"].tolist() == [1] * B
    checked = 0
    for t in range(T):
        land = r["previewed"][t, :, 1] == 1                          # (B, 4): the contacts whose touchdown is at j = 1
        prev0 = r["previewed"][t, :, 0]
        assert not prev0.any()
        for b, i in zip(*np.nonzero(land)):
            assert np.array_equal(_bits(r["foot"][t, b, 1, 3 * i:3 * i + 3]), _bits(r["feet"][t + 1, b, 3 * i:3 * i + 3])), (t, b, i)
            checked += 1
        # ... and a contact that does not land in period t stays where it was
        still = np.repeat(~land, 3, axis=1)
        assert np.array_equal(_bits(r["feet"][t + 1][still]), _bits(r["feet"][t][still]))
    assert checked >= 2 * 6 * B                                       # every robot put each foot down several times
    if ground == "slope":
        assert np.abs(r["feet"][-1].reshape(B, 4, 3)[:, :, 2]).max() > 0.01
    # psi_L,1 == landing_yaw
    inp = pvt.mpc_inputs(r["x"][7], r["feet"][7], f["stamp"] + 7 * DT, f["command"], ft.COM, N, DT)
    j1 = ~np.isnan(inp["psi_l"][:, 1])
    assert j1.any() and np.array_equal(_bits(inp["psi_l"][j1, 1]), _bits(inp["landing_yaw"][j1]))


def test_terrain_inputs_previewed_with_nothing_previewed_are_the_terrain_inputs():
    B = 9
    x, feet, stamp, cmd = _draw(B, 3)
    m = tt.rough(8, 8, 5, cell=0.5, origin=(-1.5, -1.5), amp=0.1)
    feet.reshape(B, 4, 3)[:, :, 2] = tt.sample(m, feet.reshape(B * 4, 3)[:, 0:2])[0].reshape(B, 4)
    inp = stw.mpc_inputs(x, feet, stamp, cmd, ft.COM, N, DT)
    a = pvt.terrain_inputs(m, inp["foot"], None, inp["x_ref"])
    b = tt.inputs(m, feet, inp["x_ref"])
    assert np.array_equal(_bits(a["x_ref"]), _bits(b["x_ref"])) and np.array_equal(_bits(a["normals"]), _bits(b["normals"]))
    assert np.array_equal(_bits(a["foot"]), _bits(inp["foot"]))
    pv = pvt.mpc_inputs(x, feet, stamp, cmd, ft.COM, N, DT)
    c = pvt.terrain_inputs(m, pv["foot"], pv["previewed"], pv["x_ref"])
    on = pv["previewed"] == 1
    z = c["foot"].reshape(B, N, 4, 3)[:, :, :, 2]
    assert np.array_equal(_bits(z[on]), _bits(tt.sample(m, c["foot"].reshape(-1, 3)[:, 0:2])[0].reshape(B, N, 4)[on])) and np.any(z[on] != 0.0)
    assert np.array_equal(_bits(z[~on]), _bits(pv["foot"].reshape(B, N, 4, 3)[:, :, :, 2][~on]))
    assert np.array_equal(_bits(c["x_ref"][:, :, 5]), _bits(pv["x_ref"][:, :, 5] + (((z[:, :, 0] + z[:, :, 1]) + z[:, :, 2]) + z[:, :, 3]) * 0.25))


# ---- the stand-alone host build ----
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """The stand-alone program of tests/preview_host_main.cpp, built with the host compiler: with the address and undefined-behaviour sanitizers where the
    compiler has their runtimes, plainly where it has not."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++, c++, clang++) to build the preview's host program with")
    exe = str(tmp_path_factory.mktemp("preview") / "preview_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "g1_locomotion_amd", "csrc"), "-o", exe,
            os.path.join(ROOT, "tests", "preview_host_main.cpp")]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)
    return exe


def _run(exe, rows):
    text = "\n".join(" ".join(repr(float(w)) for w in row) for row in rows) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return [[float(w) for w in line.split()] for line in out.stdout.strip().splitlines()]


def test_host_built_touchdown_steps_for_every_gait(host_program):
    want = _all_gaits()
    keys = list(want) + [(6, 1, -1, 24), (3, 0, -1, 10)]               # ... and a standing robot
    lines = _run(host_program, [[0], [len(keys)]] + [list(k) for k in keys])
    assert len(lines) == sum(k[3] for k in keys)
    at = 0
    for key in keys:
        got = np.array(lines[at:at + key[3]], np.int64)
        at += key[3]
        if key[2] < 0:
            assert not got.any(), key
            continue
        lands, jl, jr = want[key]
        assert np.array_equal(got[:, 0], lands) and np.array_equal(got[:, 1], jl) and np.array_equal(got[:, 2], jr), key


@pytest.mark.parametrize("horizon,P,ds", [(10, 6, 1), (24, 3, 0), (2, 1, 0)])
def test_host_built_footholds_against_the_twin(host_program, horizon, P, ds):
    """preview_foothold as the kernel calls it, on 24 robots over every phase, one of them standing, two with a state or a command that is not finite: the
    steps and psi_L bit for bit (no sine), heel and toe within 1e-12 of the twin's, and the touchdown at step 1 bit for bit the plant's touchdown of the
    call's own landing point."""
    B = 24
    x, feet, _, cmd = _draw(B, 20 + horizon)
    phase = np.arange(B) % (2 * P)
    phase[5] = -1
    x[6, 3], cmd[7, 2] = np.nan, np.inf
    stamp = DT * np.where(phase < 0, 0, phase).astype(np.float64) - 2 * P * DT * 5         # negative stamps
    standing = (phase < 0).astype(np.uint8)
    half = 0.085
    tw = pvt.mpc_inputs(x, feet, stamp, cmd, ft.COM, horizon, DT, standing=standing, period_steps=P, double_support_steps=ds, foot_half_length=half)
    rows = [[1], [DT, horizon, P, ds, 0.0645, half, B]] + [np.concatenate([[phase[b]], x[b], cmd[b]]).tolist() for b in range(B)]
    lines = _run(host_program, rows)
    assert len(lines) == B * (horizon + 1)
    worst, seen, first = 0.0, 0, 0
    for b in range(B):
        blk = lines[b * (horizon + 1):(b + 1) * (horizon + 1)]
        own, steps = np.array(blk[0]), np.array(blk[1:])
        with np.errstate(invalid="ignore"):
            assert _bits(own[2:3]) == _bits(tw["landing_yaw"][b:b + 1]) or (np.isnan(own[2]) and np.isnan(tw["landing_yaw"][b]))
        for k in range(horizon):
            f = int(steps[k, 0])
            assert f == pvt.lands(int(phase[b]), k, P, ds)
            if not f:
                continue
            c0 = 0 if f == 1 else 6
            want = np.concatenate([tw["foot"][b, k, c0:c0 + 2], tw["foot"][b, k, c0 + 3:c0 + 5]])
            assert tw["previewed"][b, k, c0 // 3] == 1 and np.array_equal(np.isnan(steps[k, 1:5]), np.isnan(want)), (b, k)
            assert _bits(steps[k, 5:6]) == _bits(tw["psi_l"][b:b + 1, k]) or (np.isnan(steps[k, 5]) and np.isnan(tw["psi_l"][b, k])), (b, k)
            if np.isfinite(want).all():
                worst = max(worst, np.abs(steps[k, 1:5] - want).max())
                seen += 1
            if k == 1:                                                # the plant's touchdown of this call's landing point
                assert np.array_equal(_bits(steps[k, 1:5]), _bits(own[3:7])) and _bits(steps[k, 5:6]) == _bits(own[2:3]), b
                first += 1
    print("host build against the twin", worst, "touchdowns", seen, "at step 1", first)
    assert seen > B // 2 and (first >= 2 or horizon < 2) and worst < 1e-12, worst


# ---- the build's resources ----
def test_the_previewed_instantiations_keep_nothing_in_scratch_memory(built_lib):
    """Read through tests/test_build_resources.py's helper (tools/resource_table.py on the build's kernel-resource-usage remarks): the sixteen previewed
    instantiations of srbdqp_mpc_inputs_commanded_kernel -- steered and tracked, the seven tabulated horizons and the live one -- and the previewed terrain
    inputs kernel are there, each with ScratchSize 0, and the thirty-two plain instantiations beside them still are."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table
    log = os.path.join(os.environ.get("TMPDIR", "/tmp"), "srbdqp_build.log")
    if not (os.path.exists(log) and "PreviewFeet" in open(log).read()):
        # no log of the current sources (the library came with the tree): compile the second code object's device code once more for its remarks
        src = os.path.join(ROOT, "g1_locomotion_amd", "csrc")
        log = os.path.join(os.environ.get("TMPDIR", "/tmp"), "srbdqp_build_lat.log")
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-c", "--cuda-device-only", "-o", os.devnull,
               os.path.join(src, "srbdqp_wrench_lat_ew.hip"), "-Rpass-analysis=kernel-resource-usage"]
        with open(log, "w") as lf:
            subprocess.check_call(cmd, stderr=lf)
    rows = [r for r in resource_table.parse(log) if "srbdqp_mpc_inputs_commanded_kernel" in r["name"] or "srbdqp_terrain_inputs_previewed_kernel" in r["name"]]
    new = [r for r in rows if "PreviewFeet" in r["name"] or "terrain_inputs_previewed" in r["name"]]
    print("previewed instantiations:", [(r["name"].split("(")[0], r["vgprs"], r["lds"], r["scratch"]) for r in new])
    assert len(new) == 17 and len(rows) == 33
    assert all(r["scratch"] == 0 for r in rows), [(r["name"], r["scratch"]) for r in rows if r["scratch"]]
