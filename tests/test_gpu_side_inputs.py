"""GPU tests that the four per-QP side inputs share, parametrised over tests/side_inputs.py KINDS: robot records (the general kernel's MODE = 2 instantiation,
wrench_f64_n<N>_rb), cost weights (MODE = 6, _wt), contact normals (MODE = 4, _cn) and the external wrench (MODE = 7, _ew).  The bars, the draws and the seeds
are described in tests/side_inputs.py; what is particular to one kind is in its own module (test_gpu_robots.py, test_gpu_weights.py,
test_gpu_contact_normals.py, test_gpu_ext_wrench.py), the refusals in test_gpu_variant_refusals.py.  The parity and the neutral-input test keep their
names and cases in the kinds' modules; their one body each is here (check_parity, check_neutral)."""
import re

import numpy as np
import pytest

import side_inputs as si
import srbd_oracle as orc
from gpu_helpers import device_solve, ragged_device_solve, refusal, to_dev, torch_first  # noqa: F401  (torch_first: the fixture)

pytestmark = pytest.mark.gpu

by_kind = pytest.mark.parametrize("kind", si.KINDS, ids=lambda k: k.name)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_parity(kind, N, schedule):
    """The parity test of every kind (each kind's module has it over si.HORIZONS x si.SCHEDULES under its own name): per QP against the twin with THAT QP's
    record, by the bars of si.check_qp, and what the kind asks of the batch as a whole."""
    from g1_locomotion_amd import BatchMPC
    B = kind.B
    x0, xr, ft, ct, rec = kind.case(B, N, schedule)
    with BatchMPC(horizon=N) as eng:
        out0 = eng.solve(x0, xr, ft, ct)                             # without the input: the config's robot and weights, flat ground, no wrench
        getattr(eng, kind.setter)(rec)
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        assert eng.kernel_name() == f"wrench_f64_n{N}{kind.suffix}", eng.kernel_name()
    both = [si.reference(kind, N, rec[b], x0[b], xr[b], ft[b], ct[b]) for b in range(B)]
    refs = [r for _, r in both]
    print(f"{kind.name} N={N} {schedule}: max |u - twin| {max(np.abs(out['u'][b] - refs[b]['u']).max() for b in range(B)):.3e} N, "
          f"max |x - twin| {max(np.abs(out['x'][b] - refs[b]['x']).max() for b in range(B)):.3e}, "
          f"max |iters - twin| {max(abs(int(out['iters'][b]) - refs[b]['iters']) for b in range(B))}")
    for b, (p, ref) in enumerate(both):
        si.check_qp(out, b, N, p, ref, ct[b])
    moved = sum(int(np.abs(out["u"][b] - out0["u"][b]).max() > 1.0) for b in range(B))
    solved = sum(int(r["status"] == orc.STATUS_SOLVED) for r in refs)
    most = max(int(r["iters"]) for r in refs)
    print(f"{kind.name} N={N} {schedule}: {solved} of {B} SOLVED, {moved} moved by > 1 N, most iterations {most}")
    if kind.min_solved is not None:
        assert solved >= kind.min_solved, f"only {solved} of {B} QPs are solved in the twin"
    if kind.min_moved is not None:
        assert moved >= kind.min_moved, f"only {moved} of {B} QPs moved by > 1 N from the solution without the input"
    if kind.restart_mark and N == 10:   # the restart passes ran with the input: a QP that needed them agrees with the twin
        assert most > orc.default_restart(N)[0], most


NEUTRAL_CASES = [(4, "double"), (10, "mixed"), (10, "single"), (16, "double"), (20, "three")]
_neutral = {}


def _neutral_runs(kind):
    """Per case: (a KERNEL_WRENCH solve without the input, the same QPs with the neutral input set, the same after clearing it, the three kernel names,
    check_every).  Computed once per kind: a kind may assert what all five cases showed."""
    from g1_locomotion_amd import BatchMPC, _lib
    if kind.name not in _neutral:
        runs = _neutral[kind.name] = {}
        for N, schedule in NEUTRAL_CASES:
            B = 48
            x0, xr, ft, ct = si.batch(B, N, 700 + N, schedule)
            with BatchMPC(horizon=N, kernel=_lib.KERNEL_WRENCH) as eng:
                ref = eng.solve(x0, xr, ft, ct, want_y=True)
                names = [eng.kernel_name()]
                getattr(eng, kind.setter)(kind.neutral(B, N, eng.cfg))
                out = eng.solve(x0, xr, ft, ct, want_y=True)
                names.append(eng.kernel_name())
                getattr(eng, kind.setter)(None)
                back = eng.solve(x0, xr, ft, ct, want_y=True)
                runs[(N, schedule)] = (ref, out, back, names + [eng.kernel_name()], eng.cfg.check_every)
    return _neutral[kind.name]


def check_neutral(kind, N, schedule):
    """The neutral-input test of every kind (each kind's module has it over NEUTRAL_CASES under its own name).  Every record = the handle's config, every normal e_z, a zero wrench: the same QPs as a KERNEL_WRENCH solve without the input -- statuses identical,
    iteration counts, forces and roll-out within the kind's bars (identical counts and 1e-9; flat normals: si.NORMALS).  The record paths compute 1 / mass,
    fz / s, sqrt(q_diag), (r_diag s) s ... with the operations fill_args() uses on the host, so those results are bit-identical too:
    printed, then asserted where the kind says so.  After clearing, the handle launches wrench_f64_n<N> again and reproduces its earlier outputs bit for bit."""
    runs = _neutral_runs(kind)
    ref, out, back, names, check_every = runs[(N, schedule)]
    assert names == [f"wrench_f64_n{N}", f"wrench_f64_n{N}{kind.suffix}", f"wrench_f64_n{N}"], names
    du, dx, di = np.abs(out["u"] - ref["u"]).max(), np.abs(out["x"] - ref["x"]).max(), np.abs(out["iters"] - ref["iters"]).max()
    same = {c: all(np.array_equal(r[1][k], r[0][k]) for k in ("u", "x", "y")) for c, r in runs.items()}
    print(f"{kind.name} N={N} {schedule}: max |du| {du:.3e} N, max |dx| {dx:.3e}, max |d iters| {di}, bit-identical: {same[(N, schedule)]} "
          f"(all five cases: {all(same.values())})")
    assert np.array_equal(out["status"], ref["status"])
    assert kind.neutral_iters in (0, check_every) and di <= kind.neutral_iters
    assert du <= kind.neutral_tol and dx <= kind.neutral_tol, (du, dx)
    if kind.neutral_bits == "always" or (kind.neutral_bits == "where all five cases show it" and all(same.values())):
        assert same[(N, schedule)], f"{kind.name}: not bit-identical to the solve without the input"
    for k in si.KEYS:
        assert np.array_equal(back[k], ref[k]), k


@pytest.mark.parametrize("kind", [k for k in si.KINDS if k.hint_seed is not None], ids=lambda k: k.name)
def test_schedule_hint_keeps_inputs_by_qp_index(torch_first, built_lib, kind):
    """(Contact normals: test_gpu_contact_normals.py::test_block_b_belongs_to_qp_b_under_a_hint_and_a_deferred_tail.)"""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC
    B, N = 256, 10
    x0, xr, ft, ct = si.batch(B, N, 31, "mixed")
    rec = kind.draw(B, N, kind.hint_seed)
    t = to_dev(torch, x0, xr, ft, ct)
    with BatchMPC(horizon=N) as eng:
        getattr(eng, kind.setter)(rec)
        plain = device_solve(torch, eng, t, B)
        torch.cuda.synchronize()
        hint = torch.from_numpy(np.random.default_rng(5).integers(0, 250, B).astype(np.int32)).cuda()   # a hint that reorders
        eng.set_schedule_hint(hint.data_ptr(), B)
        hinted = device_solve(torch, eng, t, B)
        torch.cuda.synchronize()
        eng.set_schedule_hint(0, 0)
    for k in ("u", "x", "status", "iters"):
        assert torch.equal(plain[k], hinted[k]), k


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("kind", [k for k in si.KINDS if k.ragged_setter is not None], ids=lambda k: k.name)
def test_ragged_inputs_follow_the_callers_order(torch_first, built_lib, kind, defer):
    """Horizons {8, 12, 16}, the QPs shuffled across the buckets: QP b of the caller's order solves with record b (the wrench: the rows at its row offset),
    against the twin per QP; with SRBDQP_FLAG_DEFER_TAIL (the device setter: read in place, beside the deferred passes too) the same after the flush, and
    equal to the call without the flag bit for bit."""
    torch = torch_first
    from g1_locomotion_amd import RaggedMPC, _lib
    Nq, x0, xr, ft, ct, rec, off, refs, ps = si.ragged_case(kind)
    B, rows = len(Nq), int(off[-1])
    t = to_dev(torch, x0, xr, ft, ct)

    def run(flags, arg):
        rg = RaggedMPC(horizons=si.RAGGED_HORIZONS, flags=flags)
        try:
            getattr(rg, kind.ragged_setter)(arg)
            return ragged_device_solve(torch, rg, Nq, t, B, rows, flush=True)
        finally:
            rg.close()

    keep = _dev(torch, rec) if defer else rec
    out = run(_lib.FLAG_DEFER_TAIL if defer else 0, keep)
    assert all(p.check_every == 5 for p in ps)                       # (the iteration bar of this test has always been 5)
    si.check_ragged(out, refs, Nq, off, lambda b: ps[b])
    if defer:
        plain = run(0, rec)
        for k in ("u", "x", "status", "iters"):
            assert np.array_equal(out[k], plain[k]), k


@by_kind
def test_a_bad_device_record_stays_local_and_the_host_setter_names_it(torch_first, built_lib, kind):
    """Host and device setter agree; a device array with bad values ends its own QPs as SRBDQP_NUMERICAL (zero forces and duals, a finite roll-out) and leaves
    every other QP's outputs as they were; the host setter refuses the same array, names the first bad value and keeps the previous setting."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    (B, seed, make_bad), N = kind.bad, 12
    x0, xr, ft, ct = si.batch(B, N, 41, "mixed")
    rec = kind.draw(B, N, seed)
    bad, bad_qps, refused = make_bad(rec)
    set_ = lambda eng, a: getattr(eng, kind.setter)(a)
    with BatchMPC(horizon=N) as eng:
        plain = eng.solve(x0, xr, ft, ct)
        set_(eng, rec)
        host = eng.solve(x0, xr, ft, ct, want_y=True)
        set_(eng, _dev(torch, rec))
        good = eng.solve(x0, xr, ft, ct, want_y=True)
        dev_bad = _dev(torch, bad)
        set_(eng, dev_bad)
        out = eng.solve(x0, xr, ft, ct, want_y=True)
        for arg, text in refused:
            msg = refusal(lambda: set_(eng, arg))
            assert msg is not None and msg.startswith(f"srbdqp error {_lib.E_INVALID}: ") and re.search(text, msg), (text, msg)
        again = eng.solve(x0, xr, ft, ct, want_y=True)               # the previous setting (the device array) was kept
    for k in si.KEYS:
        assert np.array_equal(host[k], good[k]), k
        assert np.array_equal(again[k], out[k]), k
    for b in range(B):
        if b in bad_qps:
            assert out["status"][b] == _lib.NUMERICAL and out["iters"][b] == 0, (b, out["status"][b])
            assert np.all(out["u"][b] == 0.0) and np.all(out["y"][b] == 0.0) and np.all(np.isfinite(out["x"][b]))
            assert plain["status"][b] != _lib.NUMERICAL
            if kind is si.EXT_WRENCH:                                # the roll-out of zero forces and no wrench
                zero = si.twin(si.params(N), x0[b], xr[b], ft[b], np.zeros_like(ct[b]), ext_wrench=np.zeros((N, 6)))
                assert np.abs(out["x"][b] - zero["x"]).max() <= 1e-9
        else:
            for k in si.KEYS:
                assert np.array_equal(out[k][b], good[k][b]), (b, k)


@pytest.mark.parametrize("kind", [k for k in si.KINDS if k.bound is not None], ids=lambda k: k.name)
def test_the_host_setter_and_the_kernel_share_one_bound(torch_first, built_lib, kind):
    """The bound of the kind (si._weights_bound, si._wrench_bound) holds on both sides: a value the host setter refuses ends the QP as SRBDQP_NUMERICAL in the
    kernel, and a value at a bound that is valid passes both."""
    torch = torch_first
    from g1_locomotion_amd import BatchMPC, _lib
    B, N = 4, 4
    x0, xr, ft, ct = si.batch(B, N, 51, "double")
    valid, bad, refused = kind.bound(kind.draw(B, N, 53))
    with BatchMPC(horizon=N) as eng:
        if valid is not None:
            getattr(eng, kind.setter)(valid)
        for arg, text in refused:
            msg = refusal(lambda: getattr(eng, kind.setter)(arg))
            assert msg is not None and re.search(text, msg), (text, msg)
        getattr(eng, kind.setter)(_dev(torch, bad))
        out = eng.solve(x0, xr, ft, ct)
    assert out["status"].tolist()[2:] == [_lib.NUMERICAL, _lib.NUMERICAL] and np.all(out["u"][2:] == 0.0)
    assert all(s in (orc.STATUS_SOLVED, orc.STATUS_MAX_ITER) for s in out["status"][:2])


@pytest.mark.parametrize("N", [10, 16])
def test_records_weights_and_wrench_combine(torch_first, built_lib, N):
    """Records and weights, then all three, on one handle, the setters in two orders: per QP against the twin with what is set; clearing one leaves the others,
    and the kernel names follow."""
    from g1_locomotion_amd import BatchMPC
    B = si.B16
    x0, xr, ft, ct = si.batch(B, N, si.batch_seed(N, "mixed"), "mixed")
    rec, w = si.draw_weights(B, si.weights_seed(N)), si.draw_wrench(B, N, si.wrench_seed(N))
    rob = si.draw_robots(B, 3900 + N)                                # (3900 + N: no QP of the oracle at the 250 cap with both records)
    solve = lambda eng: eng.solve(x0, xr, ft, ct, want_y=True)
    name = lambda suffix: f"wrench_f64_n{N}{suffix}"
    with BatchMPC(horizon=N) as eng:
        eng.set_robots(rob)
        rb_only = solve(eng)
        assert eng.kernel_name() == name("_rb")
        eng.set_weights(rec)                                         # records first, then weights
        rb_wt = solve(eng)
        assert eng.kernel_name() == name("_wt")
        eng.set_weights(None)
        back = solve(eng)                                            # weights cleared: the records stay in force
        assert eng.kernel_name() == name("_rb")
        eng.set_weights(rec); eng.set_external_wrench(w)             # ... then the wrench
        out = solve(eng)
        assert eng.kernel_name() == name("_ew")
        eng.set_weights(None)
        no_wt = solve(eng)                                           # weights cleared: records and wrench stay
        assert eng.kernel_name() == name("_ew")
        eng.set_external_wrench(None)
        rb_again = solve(eng)                                        # wrench cleared too: the records stay
        assert eng.kernel_name() == name("_rb")
    with BatchMPC(horizon=N) as eng:
        eng.set_weights(rec)                                         # weights first, then records
        eng.set_robots(rob)
        rb_wt2 = solve(eng)
        assert eng.kernel_name() == name("_wt")
        eng.set_robots(None)
        wt_only = solve(eng)                                         # records cleared: the weights stay in force
        assert eng.kernel_name() == name("_wt")
    with BatchMPC(horizon=N) as eng:
        eng.set_external_wrench(w); eng.set_weights(rec); eng.set_robots(rob)
        out2 = solve(eng)
        assert eng.kernel_name() == name("_ew")
        eng.set_robots(None)
        no_rb = solve(eng)                                           # records cleared: weights and wrench stay
        assert eng.kernel_name() == name("_ew")
        eng.set_external_wrench(None)
        wt_only2 = solve(eng)
        assert eng.kernel_name() == name("_wt")
        eng.set_weights(None)
        eng.set_robots(rob)
        ref_rb = solve(eng)
    for k in si.KEYS:
        assert np.array_equal(rb_wt[k], rb_wt2[k]), k
        assert np.array_equal(back[k], rb_only[k]), k
        assert np.array_equal(out[k], out2[k]), k
        assert np.array_equal(rb_again[k], ref_rb[k]), k
    for b in range(B):
        q = (x0[b], xr[b], ft[b], ct[b])
        p = si.params(N, rob[b], rec[b])
        si.check_qp(rb_wt, b, N, p, si.twin(p, *q), ct[b])
        si.check_qp(out, b, N, p, si.twin(p, *q, ext_wrench=w[b]), ct[b])
        p = si.params(N, rob[b])
        si.check_qp(no_wt, b, N, p, si.twin(p, *q, ext_wrench=w[b]), ct[b])
        p = si.params(N, weights=rec[b])
        si.check_qp(no_rb, b, N, p, si.twin(p, *q, ext_wrench=w[b]), ct[b])
        ref = si.twin(p, *q)
        si.check_qp(wt_only, b, N, p, ref, ct[b])
        si.check_qp(wt_only2, b, N, p, ref, ct[b])
