"""Which C-ABI call has a form for which variant of the general kernel (srbdqp.hip, `kFormRows`, `state_of` and the sets of `require_form`): a handle is plain, or has robot
records set, or cost weights set, or contact normals set, or an external wrench set, or a live horizon (SRBDQP_FLAG_ANY_HORIZON), or rank-aware steps
(SRBDQP_FLAG_RANK_AWARE) -- never two of them, except robot records, cost weights and the wrench beside one another (the four combined states have a walk of
their own below; what only weights or only the wrench show is in test_gpu_weights.py and test_gpu_ext_wrench.py).  Through the
Python bindings, on one handle per variant, every entry point of the table below either returns SRBDQP_E_INVALID with a message that names the call and ends in
the variant's fixed text, or returns SRBDQP_OK.  Nothing here looks at numbers: the variants' own suites do (test_gpu_side_inputs.py, test_gpu_contact_normals.py,
test_gpu_any_horizon.py, test_gpu_rank_aware.py).  The smallest shapes that reach every branch: N = 4 (a live horizon: 3, which runs on N* = 4), two QPs of full
double support."""
import numpy as np
import pytest

import srbd_oracle as orc
import side_inputs as si
from gpu_helpers import refusal as _refusal, torch_first  # noqa: F401  (torch_first: the fixture)

pytestmark = pytest.mark.gpu
B = 2
VARIANTS = ("robots", "weights", "normals", "ext_wrench", "live", "rank_aware")
# the suffix of the kernel a variant's fp64 batch solves launch
SUFFIX = dict(robots="_rb", weights="_wt", normals="_cn", ext_wrench="_ew")

# the fixed text behind "<call>: " in a refusal, per variant of the handle
TAIL = dict(
    robots="refused while per-QP robot records are set (srbdqp_set_robots): only the fp64 batch and ragged solves on the general kernel read them "
           "-- one robot for every QP goes in srbdqp_config",
    weights="refused while per-QP cost weights are set (srbdqp_set_weights): only the fp64 batch and ragged solves on the general kernel read them "
            "-- one pair of weights for every QP goes in srbdqp_config",
    normals="refused while contact normals are set (srbdqp_set_contact_normals): only the fp64 batch solves on the general kernel read them "
            "-- srbdqp_set_contact_normals(h, NULL, 0) goes back to flat ground",
    ext_wrench="refused while an external wrench is set (srbdqp_set_external_wrench): only the fp64 batch and ragged solves on the general kernel read it "
               "-- srbdqp_set_external_wrench(h, NULL, 0) goes back to no wrench",
    live="refused on a handle whose horizon 3 was admitted by SRBDQP_FLAG_ANY_HORIZON: only the fp64 batch, ragged and staged solves run a live horizon "
         "(the general kernel's fp64 batch instantiation for N = 4)",
    rank_aware="refused on a handle created with SRBDQP_FLAG_RANK_AWARE: only the fp64 batch and staged solves have rank-aware wrench steps "
               "(the general kernel's fp64 batch instantiation, flat ground, srbdqp_config's single robot)")
# (the normals setters say why records and normals do not combine, not what reads the records)
NORMALS_ON_ROBOTS = "refused while per-QP robot records are set (srbdqp_set_robots): no instantiation reads both (DESIGN.md section 13)"

ALL = frozenset(VARIANTS)
# call -> the variants whose handle it refuses; every other variant's handle it accepts.  In the order the calls are made (prepare before solve_prepared).
REFUSES = {
    "srbdqp_solve_batch_f64": frozenset(),
    "srbdqp_solve_batch_device_f64": frozenset(),
    "srbdqp_solve_staged_f64": frozenset({"robots", "weights", "normals", "ext_wrench"}),
    "srbdqp_update_f64": frozenset({"robots", "weights", "normals", "ext_wrench"}),
    "srbdqp_prepare_staged_f64": frozenset({"robots", "weights", "normals", "ext_wrench", "live"}),
    "srbdqp_solve_prepared_f64": frozenset({"robots", "weights", "normals", "ext_wrench", "live"}),
    "srbdqp_solve_batch_f32": ALL,
    "srbdqp_solve_batch_device_f32": ALL,
    "srbdqp_assemble_f64": frozenset({"robots", "weights", "normals", "ext_wrench", "live"}),
    "srbdqp_assemble_wrench_f64": ALL,
    "srbdqp_set_robots": frozenset({"normals", "live", "rank_aware"}),
    "srbdqp_set_robots_device": frozenset({"normals", "live", "rank_aware"}),
    "srbdqp_set_weights": frozenset({"normals", "live", "rank_aware"}),
    "srbdqp_set_weights_device": frozenset({"normals", "live", "rank_aware"}),
    "srbdqp_set_contact_normals": frozenset({"robots", "weights", "ext_wrench", "live", "rank_aware"}),
    "srbdqp_set_contact_normals_device": frozenset({"robots", "weights", "ext_wrench", "live", "rank_aware"}),
    "srbdqp_set_external_wrench": frozenset({"normals", "live", "rank_aware"}),
    "srbdqp_set_external_wrench_device": frozenset({"normals", "live", "rank_aware"}),
}
# variant -> the setters its handle accepts that would add another kind of input: made as set-then-clear, so that the walk leaves the handle's state alone
_RB, _WT, _EW = (tuple(f"srbdqp_set_{k}{d}" for d in ("", "_device")) for k in ("robots", "weights", "external_wrench"))
SET_THEN_CLEAR = dict(robots=_WT + _EW, weights=_RB + _EW, ext_wrench=_RB + _WT)


def _engine(variant):
    """-> (engine, its horizon); records and normals are set by the test."""
    from g1_locomotion_amd import BatchMPC
    if variant == "live":
        return BatchMPC(horizon=3), 3
    return BatchMPC(horizon=4, rank_aware=(variant == "rank_aware")), 4


def _calls(torch, eng, N, then_clear=()):
    """call name -> a function that makes the call on eng with two QPs of full double support (raises SrbdqpError unless the call returns SRBDQP_OK); the
    setters named in then_clear clear again what they set."""
    from g1_locomotion_amd import _lib
    from g1_locomotion_amd.mpc import robots_array, weights_array
    x0, xr, ft, ct = orc.synthetic_batch(B, N, seed=610 + N, schedule="double")
    assert ct.all()
    ct8 = np.ascontiguousarray(ct != 0, dtype=np.uint8)
    st = eng.stage()
    st["x0"][:B], st["x_ref"][:B], st["foot"][:B], st["contact"][:B] = x0, xr, ft, ct8
    dev = {dt: [torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda() for a in (x0, xr, ft)] + [torch.from_numpy(ct8).cuda(),
                torch.empty((B, N, 12), dtype=getattr(torch, np.dtype(dt).name), device="cuda")] for dt in (np.float64, np.float32)}
    rb, nr, ew = robots_array(B, mass=[30.0, 40.0]), si.wedge_normals(B, N), si.draw_wrench(B, N, 71)
    wr = weights_array(B, r_diag=[1e-4, 3e-4])
    rb_dev, nr_dev, wr_dev, ew_dev = (torch.from_numpy(a).cuda() for a in (rb, nr, wr, ew))
    raw = _lib.load()

    def device(dt):
        a = [t.data_ptr() for t in dev[dt]]
        eng.solve_device(B, a[0], a[1], a[2], a[3], a[4], f32=(dt == np.float32))
        eng.synchronize()

    def update():
        u0 = np.zeros(12)
        _lib.check(raw.srbdqp_update_f64(eng._h, x0[0].ctypes.data, xr[0].ctypes.data, ft[0].ctypes.data, ct8[0].ctypes.data, None, u0.ctypes.data,
                                         None, None, None, None), eng._h)

    def setter(name, method, arg):
        return (lambda: (method(arg), method(None))) if name in then_clear else (lambda: method(arg))

    return {
        "srbdqp_solve_batch_f64": lambda: eng.solve(x0, xr, ft, ct),
        "srbdqp_solve_batch_device_f64": lambda: device(np.float64),
        "srbdqp_solve_staged_f64": lambda: eng.solve_staged(B),
        "srbdqp_update_f64": update,
        "srbdqp_prepare_staged_f64": lambda: eng.prepare_staged(B),
        "srbdqp_solve_prepared_f64": lambda: eng.solve_prepared(B),
        "srbdqp_solve_batch_f32": lambda: eng.solve(x0, xr, ft, ct, dtype=np.float32),
        "srbdqp_solve_batch_device_f32": lambda: device(np.float32),
        "srbdqp_assemble_f64": lambda: eng.assemble(x0, xr, ft, ct),
        "srbdqp_assemble_wrench_f64": lambda: eng.assemble_wrench(x0, xr, ft, ct),
        "srbdqp_set_robots": setter("srbdqp_set_robots", eng.set_robots, rb),
        "srbdqp_set_robots_device": setter("srbdqp_set_robots_device", eng.set_robots, rb_dev),
        "srbdqp_set_weights": setter("srbdqp_set_weights", eng.set_weights, wr),
        "srbdqp_set_weights_device": setter("srbdqp_set_weights_device", eng.set_weights, wr_dev),
        "srbdqp_set_contact_normals": lambda: eng.set_contact_normals(nr),
        "srbdqp_set_contact_normals_device": lambda: eng.set_contact_normals(nr_dev),
        "srbdqp_set_external_wrench": setter("srbdqp_set_external_wrench", eng.set_external_wrench, ew),
        "srbdqp_set_external_wrench_device": setter("srbdqp_set_external_wrench_device", eng.set_external_wrench, ew_dev),
    }


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_call_refuses_or_accepts_the_variant(torch_first, built_lib, variant):
    from g1_locomotion_amd import _lib
    eng, N = _engine(variant)
    with eng:
        calls = _calls(torch_first, eng, N, SET_THEN_CLEAR.get(variant, ()))
        assert list(calls) == list(REFUSES)
        if variant == "robots":
            calls["srbdqp_set_robots"]()
        if variant == "weights":
            calls["srbdqp_set_weights"]()
        if variant == "normals":
            calls["srbdqp_set_contact_normals"]()
        if variant == "ext_wrench":
            calls["srbdqp_set_external_wrench"]()
        for name, refusing in REFUSES.items():
            msg = _refusal(calls[name])
            print(f"{variant:10s} {name:34s} -> {msg or 'SRBDQP_OK'}")
            if variant in refusing:
                tail = NORMALS_ON_ROBOTS if (variant == "robots" and "contact_normals" in name) else TAIL[variant]
                assert msg == f"srbdqp error {_lib.E_INVALID}: {name}: {tail}", (variant, name, msg)
            else:
                assert msg is None, (variant, name, msg)
                if name in ("srbdqp_solve_batch_f64", "srbdqp_solve_batch_device_f64") and variant in SUFFIX:
                    assert eng.kernel_name() == f"wrench_f64_n4{SUFFIX[variant]}", (variant, name, eng.kernel_name())
        if variant == "live":
            return
        # the clearing calls succeed on every handle, and leave it in its base state: plain (what records, weights, normals or a wrench refused runs again, and another
        # setter is accepted), or rank-aware still
        eng.set_robots(None)
        eng.set_weights(None)
        eng.set_contact_normals(None)
        eng.set_external_wrench(None)
        eng.set_robots(torch_first.empty((0, 8), dtype=torch_first.float64, device="cuda"))
        eng.set_weights(torch_first.empty((0, 16), dtype=torch_first.float64, device="cuda"))
        eng.set_contact_normals(torch_first.empty((0, N, 12), dtype=torch_first.float64, device="cuda"))
        eng.set_external_wrench(torch_first.empty((0, N, 6), dtype=torch_first.float64, device="cuda"))
        if variant == "rank_aware":
            assert _refusal(calls["srbdqp_solve_batch_f32"]) == f"srbdqp error {_lib.E_INVALID}: srbdqp_solve_batch_f32: {TAIL[variant]}"
            assert _refusal(calls["srbdqp_set_robots"]) == f"srbdqp error {_lib.E_INVALID}: srbdqp_set_robots: {TAIL[variant]}"
        else:
            for name in ("srbdqp_solve_staged_f64", "srbdqp_solve_batch_f32", "srbdqp_assemble_wrench_f64"):
                assert _refusal(calls[name]) is None, (variant, name)
            other = "srbdqp_set_robots" if variant == "normals" else "srbdqp_set_contact_normals"
            assert _refusal(calls[other]) is None
            assert _refusal(calls["srbdqp_solve_batch_f64"]) is None and eng.kernel_name() == ("wrench_f64_n4_rb" if variant == "normals" else "wrench_f64_n4_cn")
        assert _refusal(calls["srbdqp_solve_batch_f64"]) is None


# The four states with more than one side input, and what every call of REFUSES answers on a handle in each: None = SRBDQP_OK, a key of TAIL, or NOR =
# NORMALS_ON_ROBOTS.  Printed by the library of the commit before the forms became one table (SRBDQP_LIB) and pasted in: a refusal names the first input
# present in the order records, weights, wrench; the normals setters answer records in their own words; a solve runs the wrench's kernel if a wrench is set.
COMBINED = (("robots", "weights"), ("robots", "ext_wrench"), ("weights", "ext_wrench"), ("robots", "weights", "ext_wrench"))
COMBINED_KERNEL = ("wrench_f64_n4_wt", "wrench_f64_n4_ew", "wrench_f64_n4_ew", "wrench_f64_n4_ew")
NOR = "normals_on_robots"
_OK4, _FIRST = (None, None, None, None), ("robots", "robots", "weights", "robots")
ANSWERS = {
    "srbdqp_solve_batch_f64": _OK4,
    "srbdqp_solve_batch_device_f64": _OK4,
    "srbdqp_solve_staged_f64": _FIRST,
    "srbdqp_update_f64": _FIRST,
    "srbdqp_prepare_staged_f64": _FIRST,
    "srbdqp_solve_prepared_f64": _FIRST,
    "srbdqp_solve_batch_f32": _FIRST,
    "srbdqp_solve_batch_device_f32": _FIRST,
    "srbdqp_assemble_f64": _FIRST,
    "srbdqp_assemble_wrench_f64": _FIRST,
    "srbdqp_set_robots": _OK4,
    "srbdqp_set_robots_device": _OK4,
    "srbdqp_set_weights": _OK4,
    "srbdqp_set_weights_device": _OK4,
    "srbdqp_set_contact_normals": (NOR, NOR, "weights", NOR),
    "srbdqp_set_contact_normals_device": (NOR, NOR, "weights", NOR),
    "srbdqp_set_external_wrench": _OK4,
    "srbdqp_set_external_wrench_device": _OK4,
}


@pytest.mark.parametrize("state", COMBINED, ids="+".join)
def test_every_call_on_combined_side_inputs(torch_first, built_lib, state):
    """One handle with two or three side inputs set: every call of REFUSES, in its order, answers exactly what ANSWERS says, and each fp64 batch solve reports
    the kernel of COMBINED_KERNEL.  The setters of an input the state lacks are made as set-then-clear, so the state holds through the walk."""
    from g1_locomotion_amd import _lib
    own = dict(robots=_RB, weights=_WT, ext_wrench=_EW)
    col = COMBINED.index(state)
    eng, N = _engine("plain")
    with eng:
        calls = _calls(torch_first, eng, N, sum((own[k] for k in own if k not in state), ()))
        assert list(calls) == list(REFUSES) == list(ANSWERS)
        for k in state:
            calls[own[k][0]]()
        for name, answers in ANSWERS.items():
            msg = _refusal(calls[name])
            print(f"{'+'.join(state):26s} {name:34s} -> {msg or 'SRBDQP_OK'}")
            if answers[col] is None:
                assert msg is None, (state, name, msg)
                if name in ("srbdqp_solve_batch_f64", "srbdqp_solve_batch_device_f64"):
                    print(f"{'+'.join(state):26s} {'kernel_name':34s} -> {eng.kernel_name()}")
                    assert eng.kernel_name() == COMBINED_KERNEL[col], (state, name, eng.kernel_name())
            else:
                tail = NORMALS_ON_ROBOTS if answers[col] == NOR else TAIL[answers[col]]
                assert msg == f"srbdqp error {_lib.E_INVALID}: {name}: {tail}", (state, name, msg)


def test_ragged_objects(torch_first, built_lib):
    """The ragged rows of the table: no fp32 solve and no robot records with a live bucket, no records with an N = 24 bucket, no rank-aware object."""
    from g1_locomotion_amd import RaggedMPC, SrbdqpError, _lib
    from g1_locomotion_amd.mpc import robots_array
    rb = robots_array(B)
    with pytest.raises(SrbdqpError, match="SRBDQP_FLAG_RANK_AWARE: ragged objects have no rank-aware form"):
        RaggedMPC(horizons=(4, 8), flags=_lib.FLAG_RANK_AWARE)
    rag = RaggedMPC(horizons=(3, 4))
    try:
        qp = [orc.synthetic_batch(1, n, seed=620 + n, schedule="double") for n in (3, 4)]
        packed = ([3, 4], np.concatenate([q[0] for q in qp]), np.concatenate([q[1][0] for q in qp]), np.concatenate([q[2][0] for q in qp]),
                  np.concatenate([q[3][0] for q in qp]))
        assert _refusal(lambda: rag.solve_packed(*packed, dtype=np.float32)) == f"srbdqp error {_lib.E_INVALID}: an fp32 ragged solve: {TAIL['live']}"
        for arg in (rb, torch_first.from_numpy(rb).cuda()):
            assert _refusal(lambda: rag.set_robots(arg)) == f"srbdqp error {_lib.E_INVALID}: per-QP robot records on a ragged object: {TAIL['live']}"
        rag.set_robots(None)
        rag.solve_packed(*packed)
    finally:
        rag.close()
    rag = RaggedMPC(horizons=(4, 24))
    try:
        for arg in (rb, torch_first.from_numpy(rb).cuda()):
            msg = _refusal(lambda: rag.set_robots(arg))
            assert msg is not None and msg.startswith(f"srbdqp error {_lib.E_INVALID}: bucket N=24: per-QP robot records: not at N = 24"), msg
        rag.set_robots(None)
    finally:
        rag.close()
