"""CPU-side tests of the Python binding's shared pieces (g1_locomotion_amd/mpc.py): the config from keyword overrides, the engine base's lifetime, the closed-engine
guard of the staged calls, and MPC's one path from a call's outcome to its warning.  No call reaches the GPU: engines are built through __new__ or replaced by a
fake that answers SRBDQP_MAX_ITER."""
import ctypes as C

import numpy as np
import pytest


def test_config_from_overrides(built_lib):
    from g1_locomotion_amd import _lib, mpc
    cfg = mpc._apply_overrides(_lib.default_config(), dict(max_iter=77, mu=0.5, q_diag=range(1, 14), inertia=(1.0, 2.0, 3.0)))
    assert cfg.max_iter == 77 and cfg.mu == 0.5 and list(cfg.q_diag) == [float(i) for i in range(1, 14)] and list(cfg.inertia) == [1.0, 2.0, 3.0]
    rest = _lib.default_config()
    for name, _ in _lib.Config._fields_:
        if name not in ("max_iter", "mu", "q_diag", "inertia"):
            a, b = getattr(cfg, name), getattr(rest, name)
            assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), name
    with pytest.raises(ValueError, match=r"^q_diag: expected 13 values$"):
        mpc._apply_overrides(_lib.default_config(), dict(q_diag=[1.0] * 12))
    with pytest.raises(ValueError, match=r"^inertia: expected 3 values$"):
        mpc._apply_overrides(_lib.default_config(), dict(inertia=[1.0] * 4))
    with pytest.raises(TypeError, match=r"^unknown srbdqp_config field 'q_diagonal'$"):
        mpc._apply_overrides(_lib.default_config(), dict(q_diagonal=1.0))


def test_both_engines_share_one_lifetime():
    from g1_locomotion_amd import mpc
    for cls in (mpc.BatchMPC, mpc.RaggedMPC):
        assert issubclass(cls, mpc._Engine) and not {"__del__", "__enter__", "__exit__", "_check"} & set(vars(cls)), cls
    assert "close" not in vars(mpc.RaggedMPC)
    eng = mpc.RaggedMPC.__new__(mpc.RaggedMPC)       # never created: close() has nothing to destroy
    eng._h = C.c_void_p()
    with eng as e:
        assert e is eng
    eng.close()


def test_staged_calls_on_a_closed_engine_raise_before_any_c_call(monkeypatch):
    from g1_locomotion_amd import SrbdqpError, mpc
    eng = mpc.BatchMPC.__new__(mpc.BatchMPC)
    eng._h, eng._fcb, eng._lib = C.c_void_p(), object(), None      # a null handle beside a capsule that still looks bound; no library to call into
    if mpc._fastcall is not None:
        monkeypatch.setattr(mpc._fastcall, "solve_staged", lambda *a: pytest.fail("_fastcall.solve_staged called on a closed engine"))
    for call in (eng.solve_staged, eng.stage, eng.prepare_staged, eng.solve_prepared):
        with pytest.raises(SrbdqpError, match=r"^engine is closed$"):
            call()
    eng.close()
    assert eng._fcb is None and eng._stage is None


N = 10


class _CappedEngine:
    """What MPC uses of a BatchMPC, without a library: every solve ends with status 2 (SRBDQP_MAX_ITER) after 100 iterations."""
    _h = C.c_void_p(0)
    _fcb = None

    def __init__(self):
        z = np.zeros
        self._st = dict(capacity=1, x0=z((1, 13)), x_ref=z((1, N, 13)), foot=z((1, N, 12)), contact=z((1, N, 4), np.uint8), pcom=z((1, N, 3)),
                        u=z((1, N, 12)), x=z((1, N + 1, 13)), status=np.full(1, 2, np.int32), iters=np.full(1, 100, np.int32))

    def stage(self):
        return self._st

    def solve_staged(self, *a, **k):
        pass

    prepare_staged = solve_prepared = set_external_wrench = solve_staged

    def solve(self, *a, **k):
        return dict(u=self._st["u"].copy(), x=self._st["x"].copy(), status=self._st["status"], iters=self._st["iters"])

    def close(self):
        pass


FOOT, CONTACT = np.zeros((N, 12)), np.ones((N, 4))
ENTRY_POINTS = {
    "solve": lambda m: m.solve(m.x0, m.x_ref_hor, FOOT, CONTACT),
    "update_prepared": lambda m: m.update_prepared(),
    "update, general path": lambda m: m.update(CONTACT, FOOT, None, x_current=[0.0] * 13),       # (a list is no (13, 1) column: the NumPy arm hands it on)
    "update, host-batch path": lambda m: m.update(CONTACT, FOOT, None, external_wrench=np.zeros((N, 6))),
}


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_capped_solve_warns_at_the_callers_line(built_lib, name):
    from g1_locomotion_amd import mpc
    m = mpc.MPC(dt=0.04, horizon=N)
    m._engine = _CappedEngine()
    call = ENTRY_POINTS[name]
    with pytest.warns(RuntimeWarning, match=r"stopped at the iteration cap \(100 iterations\)") as rec:
        u0, x1 = call(m)
    assert len(rec) == 1 and (rec[0].filename, rec[0].lineno) == (call.__code__.co_filename, call.__code__.co_firstlineno), (rec[0].filename, rec[0].lineno)
    assert (m.status, m.iters) == (2, 100) and m.u_opt.shape == (N, 12) and m.x_opt.shape == (N + 1, 13)
    assert (u0.shape, x1.shape) == (((N, 12), (N + 1, 13)) if name == "solve" else ((12, 1), (N + 1, 13)))


def test_mpc_close_drops_what_bind_made(built_lib):
    from g1_locomotion_amd import mpc
    m = mpc.MPC(dt=0.04, horizon=N)
    m._engine = _CappedEngine()
    m._bind()
    assert m._upd is not None and hasattr(m, "_s_x0") and hasattr(m, "_args_pcom")
    m.close()
    assert m._upd is None and m._fcb is None and m._engine is None
    assert not [k for k in vars(m) if k.startswith(("_s_", "_args_"))]
