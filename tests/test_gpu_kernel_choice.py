"""Which kernel a solve runs (srbdqp.hip plan_solve): one row per configuration and call either side of every threshold and rule of the choice, with the
srbdqp_kernel_name() -- for the staged one-QP rows also the srbdqp_batch1_launch_path() up to its colon -- and the number of SOLVED QPs that the library of the
commit BEFORE plan_solve existed gave for it (recorded from that library on an MI355X and pasted into EXPECTED; the table passes on that library too).  Every row
is a real solve of a seeded tests/scenarios.py problem, and every status is SOLVED or MAX_ITER.

Names that other tests assert already, and that have no row here:
  * the side-input forms _rb, _wt, _ew, _cn alone, robots + weights (_wt) and robots + weights + wrench (_ew): tests/test_gpu_side_inputs.py
    (check_parity, under each kind's own module, and test_records_weights_and_wrench_combine);
  * _ra: tests/test_gpu_rank_aware.py; a live horizon (_h<n>): tests/test_gpu_any_horizon.py;
  * SRBDQP_FLAG_DEFER_TAIL at N = 4, a device-API call and then the flush on <4, 4>: tests/test_gpu_parity.py::test_deferred_tails_at_n4_without_a_contact_bound
    (the row here adds the name the flush itself leaves);
  * the fp32 tile-class split does not show in the name: the tile tests of tests/test_gpu_turning.py.
A ragged object reports no kernel name: its row (one tabulated and one live bucket) checks the statuses alone."""
import ctypes as C

import numpy as np
import pytest

import scenarios as sc
import srbd_oracle as orc
from gpu_helpers import torch_first  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

AUTO, COMPACT, SPLIT, WAVE, WRENCH = "AUTO", "COMPACT", "SPLIT", "WAVE", "WRENCH"
NO_SPIN, SETUP4, NO_LAT, DEFER = 2, 4, 32, 64          # _lib.FLAG_*


def _contacts(ct, counts):
    """The contact flags of one QP with counts[k] stance contacts at step k: the first of (left heel, left toe, right heel, right toe)."""
    ct = ct.copy()
    for k, c in enumerate(counts):
        ct[0, k] = [1] * c + [0] * (4 - c)
    return ct


def _problem(N, B, schedule, seed):
    """schedule: a tests/scenarios.py schedule, "heel" (single support on the heels: one stance contact per step), or a tuple of stance contacts per step."""
    if isinstance(schedule, tuple):
        x0, xr, ft, ct = sc.batch(B, N, seed, "double")
        return x0, xr, ft, _contacts(ct, schedule)
    if schedule == "heel":
        x0, xr, ft, ct = sc.batch(B, N, seed, "single")
        ct = ct.copy()
        ct[:, :, 1::2] = 0
        return x0, xr, ft, ct
    return sc.batch(B, N, seed, schedule)


# (id, horizon, kernel, config fields, call, B, schedule); call: host, device, device+flush, staged, prepared, host+stamps
ROWS = []


def _row(rid, N, kernel, cfg, call, B, schedule):
    ROWS.append((rid, N, kernel, cfg, call, B, schedule))


# kWrenchMinBatch: N = 10 double support, AUTO, the 4-wave kernel below 512 QPs and the general one from there
for B in (511, 512):
    for call in ("device", "host"):
        _row(f"n10_double_{call}_b{B}", 10, AUTO, {}, call, B, "double")
# kWrenchMinBatchN20: N = 20 single support, the compact kernel below 256 QPs; with a stamp buffer at every size
for B in (255, 256):
    for call in ("host", "host+stamps"):
        _row(f"n20_single_{call}_b{B}", 20, AUTO, {}, call, B, "single")
# kTail1MaxBatch: the staged call's _lat instantiation up to 8 QPs; SRBDQP_FLAG_NO_LAT: never; SRBDQP_FLAG_NO_SPIN: no completion word, the one-wave kernel
for B in (8, 9):
    for name, flags in (("", 0), ("_nolat", NO_LAT), ("_nospin", NO_SPIN)):
        _row(f"n10_single_staged{name}_b{B}", 10, AUTO, dict(flags=flags), "staged", B, "single")
# kStagedWrenchMinVars: one staged QP with 60 presolved variables (20 stance contacts) stays on the 4-wave kernel, with 63 it takes the general kernel's _lat;
# N = 4 (at most 48) never does
_row("n8_staged1_neff60", 8, AUTO, {}, "staged", 1, (4, 4, 2, 2, 2, 2, 2, 2))
_row("n8_staged1_neff63", 8, AUTO, {}, "staged", 1, (4, 4, 3, 2, 2, 2, 2, 2))
_row("n10_staged1_neff60", 10, AUTO, {}, "staged", 1, (4, 2, 2, 2, 2, 2, 2, 2, 2, 0))
_row("n10_staged1_neff63", 10, AUTO, {}, "staged", 1, (4, 3, 2, 2, 2, 2, 2, 2, 2, 0))
_row("n4_staged1_double", 4, AUTO, {}, "staged", 1, "double")
_row("n10_staged1_single", 10, AUTO, {}, "staged", 1, "single")
# max_contacts_per_step: the device API takes the config's bound (0: 4), the host API scans the batch where the config leaves it open
for N in (4, 8, 12):
    for mcs, schedule in ((0, "mixed"), (1, "heel"), (2, "single"), (3, "three"), (4, "double")):
        for call in ("device", "host"):
            _row(f"n{N}_mcs{mcs}_{call}", N, AUTO, dict(max_contacts_per_step=mcs), call, 4, schedule)
# the device API on a batch that would fit <N, 2>, bound left open: <N, 4>
_row("n8_mcs0_single_device", 8, AUTO, {}, "device", 4, "single")
_row("n8_mcs0_single_host", 8, AUTO, {}, "host", 4, "single")
# each explicit kernel at N = 10 and at N = 16
for N in (10, 16):
    for kernel in (COMPACT, SPLIT, WAVE, WRENCH):
        _row(f"n{N}_{kernel.lower()}_host", N, kernel, {}, "host", 4, "single")
_row("n10_wave_host+stamps", 10, WAVE, {}, "host+stamps", 4, "single")
_row("n10_auto_host+stamps", 10, AUTO, {}, "host+stamps", 4, "single")
_row("n10_split_host+stamps", 10, SPLIT, {}, "host+stamps", 4, "single")
_row("n24_host", 24, AUTO, {}, "host", 4, "single")
_row("n10_split_setup4", 10, SPLIT, dict(flags=SETUP4), "host", 4, "single")
# SRBDQP_FLAG_DEFER_TAIL: on the one-wave kernel, on a kernel that restarts by launches (the passes on the tail stream), at N = 4 (<4, 4> for the launch and the flush)
_row("n10_defer_wave", 10, AUTO, dict(flags=DEFER, max_contacts_per_step=2), "device+flush", 64, "single")
_row("n10_defer_compact", 10, COMPACT, dict(flags=DEFER), "device+flush", 64, "single")
_row("n12_defer_compact", 12, AUTO, dict(flags=DEFER, max_contacts_per_step=2), "device+flush", 64, "single")
_row("n4_defer_wave", 4, AUTO, dict(flags=DEFER), "device+flush", 64, "single")
_row("n10_defer_staged1", 10, AUTO, dict(flags=DEFER), "staged", 1, "single")
# rho_restart_iter = -1 against automatic (the rows above)
_row("n10_norestart_wave", 10, AUTO, dict(rho_restart_iter=-1), "host", 4, "single")
_row("n12_norestart_compact", 12, AUTO, dict(rho_restart_iter=-1), "host", 4, "single")
_row("n10_norestart_defer", 10, AUTO, dict(rho_restart_iter=-1, flags=DEFER), "device+flush", 4, "single")
_row("n10_norestart_defer_wave", 10, AUTO, dict(rho_restart_iter=-1, flags=DEFER, max_contacts_per_step=2), "device+flush", 4, "single")
# the two-phase call at N = 4: <4, 2> and <4, 4> from the staged flags
_row("n4_prepared_single", 4, AUTO, {}, "prepared", 1, "single")
_row("n4_prepared_double", 4, AUTO, {}, "prepared", 1, "double")

# id -> (srbdqp_kernel_name, srbdqp_batch1_launch_path up to its colon -- staged one-QP rows -- or None, QPs that end SOLVED): the parent commit's library
EXPECTED = {
    "n10_double_device_b511": ("compact_f64_n10_s4", None, 507),
    "n10_double_host_b511": ("compact_f64_n10_s4", None, 507),
    "n10_double_device_b512": ("wrench_f64_n10", None, 511),
    "n10_double_host_b512": ("wrench_f64_n10", None, 511),
    "n20_single_host_b255": ("compact_f64_n20_s2", None, 245),
    "n20_single_host+stamps_b255": ("compact_f64_n20_s2", None, 235),
    "n20_single_host_b256": ("wrench_f64_n20", None, 253),
    "n20_single_host+stamps_b256": ("compact_f64_n20_s2", None, 241),
    "n10_single_staged_b8": ("compact_f64_n10_s2_lat", None, 8),
    "n10_single_staged_nolat_b8": ("compact_f64_n10_s2", None, 8),
    "n10_single_staged_nospin_b8": ("wave_f64_n10_s2", None, 8),
    "n10_single_staged_b9": ("compact_f64_n10_s2", None, 9),
    "n10_single_staged_nolat_b9": ("compact_f64_n10_s2", None, 9),
    "n10_single_staged_nospin_b9": ("wave_f64_n10_s2", None, 9),
    "n8_staged1_neff60": ("compact_f64_n8_s4", "undecided", 1),
    "n8_staged1_neff63": ("wrench_f64_n8_lat", "aql", 1),
    "n10_staged1_neff60": ("compact_f64_n10_s4", "undecided", 1),
    "n10_staged1_neff63": ("wrench_f64_n10_lat", "aql", 1),
    "n4_staged1_double": ("compact_f64_n4_s4", "undecided", 1),
    "n10_staged1_single": ("compact_f64_n10_s2_lat", "aql", 1),
    "n4_mcs0_device": ("wave_f64_n4_s4", None, 4),
    "n4_mcs0_host": ("wave_f64_n4_s4", None, 4),
    "n4_mcs1_device": ("wave_f64_n4_s2", None, 4),
    "n4_mcs1_host": ("wave_f64_n4_s2", None, 4),
    "n4_mcs2_device": ("wave_f64_n4_s2", None, 4),
    "n4_mcs2_host": ("wave_f64_n4_s2", None, 4),
    "n4_mcs3_device": ("wave_f64_n4_s4", None, 4),
    "n4_mcs3_host": ("wave_f64_n4_s4", None, 4),
    "n4_mcs4_device": ("wave_f64_n4_s4", None, 4),
    "n4_mcs4_host": ("wave_f64_n4_s4", None, 4),
    "n8_mcs0_device": ("compact_f64_n8_s4", None, 4),
    "n8_mcs0_host": ("compact_f64_n8_s4", None, 4),
    "n8_mcs1_device": ("wave_f64_n8_s2", None, 4),
    "n8_mcs1_host": ("wave_f64_n8_s2", None, 4),
    "n8_mcs2_device": ("wave_f64_n8_s2", None, 4),
    "n8_mcs2_host": ("wave_f64_n8_s2", None, 4),
    "n8_mcs3_device": ("compact_f64_n8_s4", None, 4),
    "n8_mcs3_host": ("compact_f64_n8_s4", None, 4),
    "n8_mcs4_device": ("compact_f64_n8_s4", None, 4),
    "n8_mcs4_host": ("compact_f64_n8_s4", None, 4),
    "n12_mcs0_device": ("wrench_f64_n12", None, 4),
    "n12_mcs0_host": ("wrench_f64_n12", None, 4),
    "n12_mcs1_device": ("compact_f64_n12_s2", None, 4),
    "n12_mcs1_host": ("compact_f64_n12_s2", None, 4),
    "n12_mcs2_device": ("compact_f64_n12_s2", None, 4),
    "n12_mcs2_host": ("compact_f64_n12_s2", None, 4),
    "n12_mcs3_device": ("wrench_f64_n12", None, 4),
    "n12_mcs3_host": ("wrench_f64_n12", None, 4),
    "n12_mcs4_device": ("wrench_f64_n12", None, 4),
    "n12_mcs4_host": ("wrench_f64_n12", None, 4),
    "n8_mcs0_single_device": ("compact_f64_n8_s4", None, 4),
    "n8_mcs0_single_host": ("wave_f64_n8_s2", None, 4),
    "n10_compact_host": ("compact_f64_n10_s2", None, 4),
    "n10_split_host": ("split_f64_n10_s2", None, 4),
    "n10_wave_host": ("wave_f64_n10_s2", None, 4),
    "n10_wrench_host": ("wrench_f64_n10", None, 4),
    "n16_compact_host": ("compact_f64_n16_s2", None, 4),
    "n16_split_host": ("compact_f64_n16_s2", None, 4),
    "n16_wave_host": ("compact_f64_n16_s2", None, 4),
    "n16_wrench_host": ("wrench_f64_n16", None, 4),
    "n10_wave_host+stamps": ("wave_f64_n10_s2", None, 4),
    "n10_auto_host+stamps": ("compact_f64_n10_s2", None, 4),
    "n10_split_host+stamps": ("compact_f64_n10_s2", None, 4),
    "n24_host": ("wrench_f64_n24", None, 4),
    "n10_split_setup4": ("split_f64_n10_s2", None, 4),
    "n10_defer_wave": ("wave_defer_f64_n10_s2|wave_defer_f64_n10_s2", None, 64),
    "n10_defer_compact": ("compact_f64_n10_s4|compact_f64_n10_s4", None, 64),
    "n12_defer_compact": ("compact_f64_n12_s2|compact_f64_n12_s2", None, 64),
    "n4_defer_wave": ("wave_defer_f64_n4_s4|wave_defer_f64_n4_s4", None, 64),
    "n10_defer_staged1": ("compact_f64_n10_s2_lat", "undecided", 1),
    "n10_norestart_wave": ("wave_f64_n10_s2", None, 4),
    "n12_norestart_compact": ("compact_f64_n12_s2", None, 4),
    "n10_norestart_defer": ("compact_f64_n10_s4|compact_f64_n10_s4", None, 4),
    "n10_norestart_defer_wave": ("wave_f64_n10_s2|wave_f64_n10_s2", None, 4),
    "n4_prepared_single": ("prepare_f64_n4_s2|prepared_f64_n4_s2", "undecided", 1),
    "n4_prepared_double": ("prepare_f64_n4_s4|prepared_f64_n4_s4", "undecided", 1),
}
RAGGED_SOLVED = 6


def run_row(torch, row):
    """-> (kernel name [+ '|' + the name after the flush], launch path or None, statuses)"""
    from g1_locomotion_amd import BatchMPC, _lib
    rid, N, kernel, cfg, call, B, schedule = row
    x0, xr, ft, ct = _problem(N, B, schedule, seed=9100 + 7 * N + B)
    keep = []
    with BatchMPC(horizon=N, kernel=getattr(_lib, "KERNEL_" + kernel), **cfg) as eng:
        if call.endswith("+stamps"):
            keep.append(torch.zeros((B, 16), dtype=torch.int64, device="cuda"))
            _lib.check(eng._lib.srbdqp_set_stamp_buffer(eng._h, C.c_void_p(keep[0].data_ptr())), eng._h)
        path = None
        if call.startswith("host"):
            status = eng.solve(x0, xr, ft, ct)["status"]
            name = eng.kernel_name()
        elif call.startswith("device"):
            d = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (x0, xr, ft, ct.astype(np.uint8))]
            u = torch.zeros((B, N, 12), dtype=torch.float64, device="cuda")
            st = torch.full((B,), -77, dtype=torch.int32, device="cuda")
            eng.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), u.data_ptr(), status=st.data_ptr())
            name = eng.kernel_name()
            if call == "device+flush":
                eng.flush()
                name += "|" + eng.kernel_name()
            eng.synchronize()
            torch.cuda.synchronize()
            status = st.cpu().numpy()
        else:
            s = eng.stage()
            s["x0"][:B] = x0; s["x_ref"][:B] = xr; s["foot"][:B] = ft.reshape(B, N, 12); s["contact"][:B] = ct.reshape(B, N, 4)
            if call == "prepared":
                eng.prepare_staged(B)
                name = eng.kernel_name()
                eng.solve_prepared(B)
                name += "|" + eng.kernel_name()
            else:
                eng.solve_staged(B)
                name = eng.kernel_name()
            if B == 1:
                path = eng.batch1_launch_path().split(":")[0]
            status = np.array(s["status"][:B])
    return name, path, status


def run_ragged(torch):
    """One tabulated bucket (N = 8) and one live one (N = 7, on the instantiation for 8): -> statuses"""
    from g1_locomotion_amd import RaggedMPC
    probs = []
    for i, N in enumerate((8, 7, 7, 8, 8, 7)):
        x0, xr, ft, ct = sc.batch(1, N, 9300 + i, ("single", "double", "mixed")[i % 3])
        probs.append(dict(x0=x0[0], x_ref=xr[0], foot=ft[0].reshape(N, 12), contact=ct[0].reshape(N, 4)))
    rg = RaggedMPC(horizons=(8, 7))
    try:
        return np.array([r["status"] for r in rg.solve(probs)])
    finally:
        rg.close()


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_kernel_choice(torch_first, built_lib, row):
    name, path, status = run_row(torch_first, row)
    print(f'    "{row[0]}": ("{name}", {path!r}, {int((status == orc.STATUS_SOLVED).sum())}),   # statuses {sorted(set(status.tolist()))}')
    assert np.isin(status, (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER)).all(), status
    assert (name, path, int((status == orc.STATUS_SOLVED).sum())) == EXPECTED[row[0]]


def test_ragged_object_with_a_tabulated_and_a_live_bucket(torch_first, built_lib):
    status = run_ragged(torch_first)
    print(f"RAGGED_SOLVED = {int((status == orc.STATUS_SOLVED).sum())}   # statuses {status.tolist()}")
    assert np.isin(status, (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER)).all(), status
    assert int((status == orc.STATUS_SOLVED).sum()) == RAGGED_SOLVED
