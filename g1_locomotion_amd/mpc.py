"""Host-side mirror of the reference's MPC object for the hot path, over the C-ABI HIP library.

``MPC`` keeps the duck-typed surface the reference's callers use
(g1_mujoco_sim/src/run_simulation.py:169-170,73-82,96,103,106):

    MPC = mpc.MPC(dt=0.04); MPC.init_matrices()
    MPC.x0[...] ; MPC.x_ref_hor[...] ; MPC.g ; MPC.HORIZON_LENGTH
    u_opt0, x_opt1 = MPC.update(contact_horizon, c_horizon, p_com_horizon, x_current=MPC.x0, one_rollout=True)

``solve()`` (named by BASELINE.json, no call site in the reference tree) is this build's assemble+solve step
that ``update()`` calls.  ``BatchMPC`` is the same operation for B independent QPs (NumPy host arrays, or
device pointers of HBM-resident buffers).  All compute happens in libsrbdqp.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
import time
import warnings
from typing import Optional, Sequence

import numpy as np

from . import _lib
try:                                    # CPython binding of the two batch-1 calls (csrc/fastcall.c, built by __graft_entry__.build()); optional: ctypes otherwise
    from . import _fastcall
except ImportError:                     # pragma: no cover
    _fastcall = None
from ._lib import NX, NU, NC, SrbdqpError, robots_array, weights_array, contact_frames  # noqa: F401  (robots_array, weights_array: the rows of set_robots, set_weights; contact_frames: set_contact_normals' convention)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_p = _ptr


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _side_arg(setter, a, trailing, hint="", read="it is"):
    """A per-QP side input as `setter` (set_robots, set_weights, set_contact_normals) takes it -> (address or None, length, object to keep alive or None,
    is_device).  trailing: the accepted shapes behind the leading L.  A NumPy array goes to the host setter (checked and copied), a CUDA float64 torch tensor
    to the device setter (read at every solve: the engine holds a reference to it), None clears."""
    if a is None:
        return None, 0, None, False
    shapes = " or ".join("(L, " + ", ".join(map(str, t)) + ")" for t in trailing)
    if hasattr(a, "data_ptr") and hasattr(a, "is_cuda"):
        import torch
        shp = tuple(a.shape)
        if not a.is_cuda or a.dtype != torch.float64 or shp[1:] not in trailing:
            raise ValueError(f"{setter}: a torch tensor must be CUDA float64 of shape {shapes}, got {a.dtype} {shp} on {a.device}")
        if not a.is_contiguous():
            raise ValueError(f"{setter}: the tensor must be contiguous ({read} read in place)")
        return (C.c_void_p(a.data_ptr()) if shp[0] else None), int(shp[0]), a, True
    arr = np.asarray(a)
    if arr.shape[1:] not in trailing:
        raise ValueError(f"{setter}: expected shape {shapes}{hint}, got {arr.shape}")
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    return (_ptr(arr) if arr.shape[0] else None), int(arr.shape[0]), arr, False


def _robots_arg(robots):
    return _side_arg("set_robots", robots, ((_lib.ROBOT_DOUBLES,),), " (robots_array())", "its rows are")


def _weights_arg(weights):
    return _side_arg("set_weights", weights, ((_lib.WEIGHTS_DOUBLES,),), " (weights_array())", "its rows are")


def _normals_arg(normals, N):
    return _side_arg("set_contact_normals", normals, ((N, NU), (N, NC, 3)))


def _ext_wrench_arg(w, trailing):
    return _side_arg("set_external_wrench", w, (trailing,))


def _set_side(eng, fn, attr, arg):
    """The body of every set_* method of BatchMPC and RaggedMPC: the host or the device form of the C-ABI setter `fn`, and in eng.<attr> what was set (None once
    cleared) -- a device tensor stays referenced while the library reads it.  One rule for the three kinds, the one solve(normals=) needs to restore a
    setting: a host array is kept too, until the next call of its setter, though the library has copied it."""
    ptr, n, keep, dev = arg
    eng._check(getattr(eng._lib, fn + "_device" if dev else fn)(eng._h, ptr, n))
    setattr(eng, attr, keep if n else None)


def _as(a, dtype, shape, name):
    arr = np.ascontiguousarray(a, dtype=dtype)
    if arr.shape != tuple(shape):
        try:
            arr = arr.reshape(shape)
        except ValueError as e:
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {np.shape(a)}") from e
    return arr


def _apply_overrides(cfg, overrides):
    """Keyword overrides of srbdqp_config fields, written into cfg: a scalar in the field's own type, q_diag (13) and inertia (3) element by element."""
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise TypeError(f"unknown srbdqp_config field {k!r}")
        if k in ("q_diag", "inertia"):
            arr = getattr(cfg, k)
            if len(v) != len(arr):
                raise ValueError(f"{k}: expected {len(arr)} values")
            for i, x in enumerate(v):
                arr[i] = float(x)
        else:
            setattr(cfg, k, type(getattr(cfg, k))(v))
    return cfg


class _Engine:
    """What BatchMPC and RaggedMPC share: the handle and its lifetime.  _CREATE, _DESTROY, _LAST_ERROR: the C names that differ between the two."""
    _CREATE = _DESTROY = _LAST_ERROR = None

    def _create(self, cfg, *args):
        """<_CREATE>(&cfg, *args, &self._h), or SrbdqpError with the library's reason."""
        self._lib = _lib.load()
        self._h = C.c_void_p()
        rc = getattr(self._lib, self._CREATE)(C.byref(cfg), *args, C.byref(self._h))
        if rc != _lib.OK:
            msg = getattr(self._lib, self._LAST_ERROR)(None)
            self._h = C.c_void_p()
            raise SrbdqpError(f"{self._CREATE} failed ({rc}): {msg.decode() if msg else '?'}")

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._DESTROY)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != _lib.OK:
            msg = getattr(self._lib, self._LAST_ERROR)(self._h)
            raise SrbdqpError(f"srbdqp error {rc}: {msg.decode() if msg else '?'}")


class BatchMPC(_Engine):
    """B independent SRBD convex-MPC QPs per call.  One instance <-> one HIP stream <-> one thread."""
    _CREATE, _DESTROY, _LAST_ERROR = "srbdqp_create", "srbdqp_destroy", "srbdqp_last_error"
    _stage = _fcb = None                    # stage(): NumPy views of the staging arrays, and the CPython binding's capsule on them
    _stage_side = None                      # stage_ext_wrench(), stage_contact_normals(): kind -> the view of that staged array, once made
    # the side input a staged call can carry, by kind: its three C calls and its doubles per horizon step
    _STAGED_SIDE = {"wrench": ("srbdqp_stage_ext_wrench", "srbdqp_solve_staged_wrench_f64", "srbdqp_update_wrench_f64", 6),
                    "normals": ("srbdqp_stage_contact_normals", "srbdqp_solve_staged_normals_f64", "srbdqp_update_normals_f64", NU)}

    def __init__(self, horizon: int = 10, dt: float = 0.04, device: int = 0, kernel: int = _lib.KERNEL_AUTO,
                 timing: bool = False, rank_aware: bool = False, **overrides):
        """rank_aware=True sets SRBDQP_FLAG_RANK_AWARE (include/srbdqp.h): on the general kernel, steps whose stance contact points lie on or near one line --
        feet in tandem, point feet -- are solved in rank-aware coordinates instead of ending the QP with status -1 (fp64 solves, N <= 20, flat ground, one
        robot).  flags=_lib.FLAG_RANK_AWARE does the same."""
        cfg = _lib.default_config()
        cfg.horizon = int(horizon)
        cfg.dt = float(dt)
        cfg.device = int(device)
        cfg.kernel = int(kernel)
        cfg.flags = _lib.FLAG_TIMING if timing else 0
        _apply_overrides(cfg, overrides)
        if cfg.horizon not in _lib.HORIZONS:        # any other horizon 1 ... 24: the general kernel's live-horizon mode (include/srbdqp.h, SRBDQP_FLAG_ANY_HORIZON)
            cfg.flags |= _lib.FLAG_ANY_HORIZON
        if rank_aware:                              # (after the overrides: flags= and the keyword add up)
            cfg.flags |= _lib.FLAG_RANK_AWARE
        self.cfg = cfg
        self._create(cfg)
        self.N = int(horizon)
        self.n = NU * self.N
        self.m = _lib.ROWS_PER_STEP * self.N

    def close(self):
        self._stage = self._fcb = self._stage_side = None   # the views and the capsule point into memory the library is about to free
        super().close()

    def _open(self):
        """The staged calls' guard: their views and the bound capsule hold addresses that close() has freed."""
        if not self._h:
            raise SrbdqpError("engine is closed")

    def _qp_inputs(self, x0, x_ref, foot, contact, pcom, dt=np.float64):
        """The QP inputs of solve() and the two assembly dumps as contiguous arrays of their shapes -> (B, x0, x_ref, foot, contact, pcom)."""
        N = self.N
        x0 = np.ascontiguousarray(x0, dtype=dt)
        B = x0.size // NX
        return (B, _as(x0, dt, (B, NX), "x0"), _as(x_ref, dt, (B, N, NX), "x_ref"), _as(foot, dt, (B, N, NU), "foot"),
                _as(np.asarray(contact) != 0, np.uint8, (B, N, NC), "contact"), None if pcom is None else _as(pcom, dt, (B, N, 3), "pcom"))

    # -- host-buffer API -------------------------------------------------------------------------------
    def solve(self, x0, x_ref, foot, contact, pcom=None, warm_u=None, warm_y=None, want_x=True, want_y=False,
              dtype=np.float64, normals=None):
        """Solve B QPs.  Returns dict(u (B,N,12) [N], x (B,N+1,13), y (B,20N), status (B,), iters (B,)).
        dtype=np.float32 goes through srbdqp_solve_batch_f32: fp32 buffers and fp32 ADMM iterations (fp64 set-up).
        normals: contact normals for this call alone (set_contact_normals' argument); the engine's previous setting is restored afterwards."""
        if normals is not None:
            prev = getattr(self, "_normals_set", None)
            self.set_contact_normals(normals)
            try:
                return self.solve(x0, x_ref, foot, contact, pcom, warm_u, warm_y, want_x, want_y, dtype)
            finally:
                self.set_contact_normals(prev)
        N, n, m = self.N, self.n, self.m
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError("dtype must be float64 or float32")
        B, x0, x_ref, foot, contact, pcom = self._qp_inputs(x0, x_ref, foot, contact, pcom, dt)
        warm_u = None if warm_u is None else _as(warm_u, dt, (B, n), "warm_u")
        warm_y = None if warm_y is None else _as(warm_y, dt, (B, m), "warm_y")
        u = np.empty((B, N, NU), dt)
        x = np.empty((B, N + 1, NX), dt) if want_x else None
        y = np.empty((B, m), dt) if want_y else None
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        fn = self._lib.srbdqp_solve_batch_f64 if dt == np.dtype(np.float64) else self._lib.srbdqp_solve_batch_f32
        rc = fn(self._h, B, _ptr(x0), _ptr(x_ref), _ptr(foot), _ptr(contact), _ptr(pcom), _ptr(warm_u), _ptr(warm_y),
                _ptr(u), _ptr(x), _ptr(y), _ptr(status), _ptr(iters))
        self._check(rc)
        return dict(u=u, x=x, y=y, status=status, iters=iters)

    def assemble(self, x0, x_ref, foot, contact, pcom=None):
        """QP data in the scaled variables as the shipped compact / one-wave kernel builds it (srbdqp_assemble_f64):
        dict(P (B,n,n), q (B,n), l (B,m), u (B,m)); rows / columns of swing-contact variables are 0 (presolve)."""
        N, n, m = self.N, self.n, self.m
        B, x0, x_ref, foot, contact, pcom = self._qp_inputs(x0, x_ref, foot, contact, pcom)
        P = np.empty((B, n, n)); q = np.empty((B, n)); lo = np.empty((B, m)); hi = np.empty((B, m))
        rc = self._lib.srbdqp_assemble_f64(self._h, B, _ptr(x0), _ptr(x_ref), _ptr(foot), _ptr(contact), _ptr(pcom),
                                           _ptr(P), _ptr(q), _ptr(lo), _ptr(hi))
        self._check(rc)
        return dict(P=P, q=q, l=lo, u=hi)

    def assemble_wrench(self, x0, x_ref, foot, contact, pcom=None):
        """What the general kernel builds before its factorisation (srbdqp_assemble_wrench_f64): dict(T (B,6N,6N), q (B,12N),
        Bd (B,12N,12), Vcol (B,12N,6), Vrow (B,12N,6), goff (B,N+1) int)."""
        N, n = self.N, self.n
        B, x0, x_ref, foot, contact, pcom = self._qp_inputs(x0, x_ref, foot, contact, pcom)
        T = np.empty((B, 6 * N, 6 * N)); q = np.empty((B, n)); bl = np.empty((B, n, 24)); go = np.empty((B, N + 1))
        rc = self._lib.srbdqp_assemble_wrench_f64(self._h, B, _ptr(x0), _ptr(x_ref), _ptr(foot), _ptr(contact), _ptr(pcom),
                                                  _ptr(T), _ptr(q), _ptr(bl), _ptr(go))
        self._check(rc)
        return dict(T=T, q=q, Bd=bl[:, :, 0:12].copy(), Vcol=bl[:, :, 12:18].copy(), Vrow=bl[:, :, 18:24].copy(), goff=go.astype(int))

    # -- device-buffer API -----------------------------------------------------------------------------
    def solve_device(self, B, x0, x_ref, foot, contact, u_out, x_out=0, y_out=0, status=0, iters=0, pcom=0,
                     warm_u=0, warm_y=0, stream=0, f32=False):
        """Enqueue a solve on HBM-resident buffers.  Every argument is a raw device address (int), e.g.
        ``tensor.data_ptr()``; 0 = absent.  ``stream`` is a hipStream_t address (0 = the handle's own stream).
        f32=True: the buffers hold float32 (srbdqp_solve_batch_device_f32).  Does not synchronise."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        fn = self._lib.srbdqp_solve_batch_device_f32 if f32 else self._lib.srbdqp_solve_batch_device_f64
        rc = fn(self._h, int(B), v(x0), v(x_ref), v(foot), v(contact), v(pcom), v(warm_u), v(warm_y), v(u_out), v(x_out),
                v(y_out), v(status), v(iters), v(stream))
        self._check(rc)

    def set_schedule_hint(self, iters_prev_ptr=0, length=0):
        """Device address and length of the previous step's iters[] (or 0): longest-first dispatch for the next device
        solves of at most `length` QPs.  A hint without a length is an error (it would silently never apply)."""
        if iters_prev_ptr and int(length) <= 0:
            raise ValueError("set_schedule_hint: pass the number of entries of iters_prev (length > 0) with the pointer")
        self._check(self._lib.srbdqp_set_schedule_hint(self._h, C.c_void_p(int(iters_prev_ptr)) if iters_prev_ptr else None,
                                                       int(length) if iters_prev_ptr else 0))

    def set_robots(self, robots):
        """One robot per QP (include/srbdqp.h srbdqp_set_robots): robots = robots_array(...) rows (NumPy, copied by the library), a CUDA float64 torch
        tensor (L, 8) (kept and read at every solve: leave it untouched until those solves have completed), or None (back to the config's robot).
        While set, QP b of a solve uses row b; the fp64 solves run on the general kernel, wbid_reference() uses each robot's mass and inertia, and the
        fp32, staged and assembly calls raise SrbdqpError."""
        _set_side(self, "srbdqp_set_robots", "_robots", _robots_arg(robots))

    def set_weights(self, weights):
        """One pair of cost weights (q_diag, r_diag) per QP (include/srbdqp.h srbdqp_set_weights): weights = weights_array(...) rows (NumPy, checked and
        copied by the library), a CUDA float64 torch tensor (L, 16) (kept and read at every solve: leave it untouched until those solves have completed), or
        None (back to the config's weights).  While set, QP b of a solve uses row b; the fp64 solves run on the general kernel (wrench_f64_n<N>_wt), with
        or without set_robots() records, and the fp32, staged and assembly calls raise SrbdqpError."""
        _set_side(self, "srbdqp_set_weights", "_weights", _weights_arg(weights))

    def set_contact_normals(self, normals):
        """Friction pyramids on sloped ground (include/srbdqp.h srbdqp_set_contact_normals): normals (L, N, 12) or (L, N, 4, 3), the world-frame surface normal
        under contact i of step k of QP b -- a NumPy array (checked and copied by the library), a CUDA float64 torch tensor (kept and read at every solve: leave
        it untouched until those solves have completed), or None (flat ground again).  While set, the five cone rows of a contact act on R' f with R =
        contact_frames(normal); forces, states and duals keep their frames and units; the fp64 solves run on the general kernel (wrench_f64_n<N>_cn), and
        the fp32, staged and assembly calls raise SrbdqpError."""
        _set_side(self, "srbdqp_set_contact_normals", "_normals_set", _normals_arg(normals, self.N))   # (_normals_set: what solve(normals=) restores)

    def set_external_wrench(self, w):
        """A known wrench on the body per horizon step (include/srbdqp.h srbdqp_set_external_wrench): w (L, N, 6), [b, k, 0:3] a world-frame torque about
        the CoM in N m and [b, k, 3:6] a world-frame force in N acting on QP b during step k -- a NumPy array (checked and copied by the library), a CUDA
        float64 torch tensor (kept and read at every solve: leave it untouched until those solves have completed), or None (no wrench again).  While set,
        the fp64 solves run on the general kernel (wrench_f64_n<N>_ew), with or without set_robots() records and set_weights() weights, and the fp32,
        staged and assembly calls raise SrbdqpError."""
        _set_side(self, "srbdqp_set_external_wrench", "_ext_wrench", _ext_wrench_arg(w, (self.N, 6)))

    def flush(self, stream=0):
        """FLAG_DEFER_TAIL: enqueue the continuations no later solve has picked up (srbdqp_flush); stream = a hipStream_t address, 0 = every
        stream this engine has launched on.  Does not synchronise.  Until the flush has completed in stream order the device arrays of the earlier
        solve_device() calls -- their OUTPUTS and their INPUTS (a continuation rebuilds its QP from the pointers of the launch it came from) -- must
        stay untouched (include/srbdqp.h, SRBDQP_FLAG_DEFER_TAIL)."""
        self._check(self._lib.srbdqp_flush(self._h, C.c_void_p(int(stream)) if stream else None))

    # -- low-latency staged API (small batches; the single-robot control loop) --------------------------
    def stage(self):
        """NumPy views of the library's pinned, GPU-mapped staging arrays (dict; first axis = capacity)."""
        self._open()
        if self._stage is None:
            st = _lib.Stage()
            self._check(self._lib.srbdqp_stage_ptrs(self._h, C.byref(st)))
            cap, N, n, m = st.capacity, self.N, self.n, self.m

            def view(addr, ctype, shape):
                cnt = int(np.prod(shape))
                return np.ctypeslib.as_array((ctype * cnt).from_address(addr)).reshape(shape)
            d, u8, i32 = C.c_double, C.c_uint8, C.c_int32
            self._stage = dict(
                capacity=cap, x0=view(st.x0, d, (cap, NX)), x_ref=view(st.x_ref, d, (cap, N, NX)),
                foot=view(st.foot, d, (cap, N, NU)), contact=view(st.contact, u8, (cap, N, NC)),
                pcom=view(st.pcom, d, (cap, N, 3)), warm_u=view(st.warm_u, d, (cap, n)), warm_y=view(st.warm_y, d, (cap, m)),
                u=view(st.u, d, (cap, N, NU)), x=view(st.x, d, (cap, N + 1, NX)), y=view(st.y, d, (cap, m)),
                status=view(st.status, i32, (cap,)), iters=view(st.iters, i32, (cap,)))
            if _fastcall is not None:       # the same two C entry points through their function pointers (no ctypes trampoline per call)
                raw = _lib.load_raw()
                addr = lambda f: C.cast(f, C.c_void_p).value
                self._fcb = _fastcall.bind(addr(raw.srbdqp_update_f64), addr(raw.srbdqp_solve_staged_f64), self._h.value, N, st.x0, st.x_ref, st.foot,
                                           st.contact, st.pcom, st.u, st.x, st.status, st.iters)
        return self._stage

    def solve_staged(self, B=1, use_pcom=False, use_warm=False, want_x=True, want_y=False):
        """One kernel launch over the first B staged QPs; inputs are read and outputs written in the staging arrays."""
        if not self._h:                     # (_open(), in line: this call is the control loop's)
            raise SrbdqpError("engine is closed")
        fcb = self._fcb
        if fcb is not None:
            rc = _fastcall.solve_staged(fcb, int(B), int(use_pcom), int(use_warm), int(want_x), int(want_y))
            if rc:
                self._check(rc)
            return
        self._check(self._lib.srbdqp_solve_staged_f64(self._h, int(B), int(use_pcom), int(use_warm), int(want_x), int(want_y)))

    def _stage_side_view(self, kind):
        """NumPy view (capacity, N, width) of the staged array of side input `kind` (a row of _STAGED_SIDE), made at the first call and kept until close()."""
        self._open()
        views = self._stage_side = self._stage_side or {}
        if kind not in views:
            stage, _, _, width = self._STAGED_SIDE[kind]
            p = C.c_void_p()
            self._check(getattr(self._lib, stage)(self._h, C.byref(p)))
            shape = (self.stage()["capacity"], self.N, width)
            views[kind] = np.ctypeslib.as_array((C.c_double * int(np.prod(shape))).from_address(p.value)).reshape(shape)
        return views[kind]

    def _solve_staged_side(self, kind, B, use_pcom, use_warm, want_x, want_y):
        self._open()
        self._check(getattr(self._lib, self._STAGED_SIDE[kind][1])(self._h, int(B), int(use_pcom), int(use_warm), int(want_x), int(want_y)))

    def _bind_update_side(self, kind):
        """The update call of side input `kind` for the QP in row 0 of the staging arrays with every argument bound once, as MPC binds the plain call: inputs,
        side input and outputs ARE the staging arrays, so the C side copies nothing -> (fn, arguments with pcom, arguments without); rc = fn(*arguments)."""
        st, side = self.stage(), self._stage_side_view(kind)
        P = lambda a: C.c_void_p(a.ctypes.data)
        ins = (C.c_void_p(self._h.value), P(st["x0"][0]), P(st["x_ref"][0]), P(st["foot"][0]), P(st["contact"][0]))
        outs = (P(side[0]), P(st["u"][0]), None, P(st["x"][0]), None, None)
        return getattr(_lib.load_raw(), self._STAGED_SIDE[kind][2]), ins + (P(st["pcom"][0]),) + outs, ins + (None,) + outs

    def stage_ext_wrench(self):
        """NumPy view (capacity, N, 6) of the staged wrench array (srbdqp_stage_ext_wrench): [b, k, 0:3] a world-frame torque about the CoM in N m and
        [b, k, 3:6] a world-frame force in N on QP b during step k, as set_external_wrench() takes them.  Pinned and GPU-mapped like the arrays of stage(),
        zero-filled, allocated by the library at the first call."""
        return self._stage_side_view("wrench")

    def solve_staged_wrench(self, B=1, use_pcom=False, use_warm=False, want_x=True, want_y=False):
        """solve_staged() with QP b under block b of stage_ext_wrench(), for this call alone (srbdqp_solve_staged_wrench_f64): nothing is set on the engine,
        and the next solve_staged() is what it would have been.  The general kernel for every contact pattern: its low-latency external-wrench
        instantiation (wrench_f64_n<N>_lat_ew) at N <= 10 and B <= 8, the batch one (wrench_f64_n<N>_ew) otherwise.  A value that is not finite or above
        1e6 raises SrbdqpError before anything is launched."""
        self._solve_staged_side("wrench", B, use_pcom, use_warm, want_x, want_y)

    def bind_update_wrench(self):
        """srbdqp_update_wrench_f64 for the QP in row 0 of the staging arrays with every argument bound once, as MPC binds the plain call: inputs, wrench and
        outputs ARE the staging arrays, so the C side copies nothing -> (fn, arguments with pcom, arguments without); rc = fn(*arguments)."""
        return self._bind_update_side("wrench")

    def stage_contact_normals(self):
        """NumPy view (capacity, N, 12) of the staged normals array (srbdqp_stage_contact_normals): [b, k, 3 i : 3 i + 3] the world-frame surface normal under
        contact i of step k of QP b, as set_contact_normals() takes them (swing contacts included).  Pinned and GPU-mapped like the arrays of stage(), filled
        with (0, 0, 1) -- a block nobody wrote is flat ground --, allocated by the library at the first call."""
        return self._stage_side_view("normals")

    def solve_staged_normals(self, B=1, use_pcom=False, use_warm=False, want_x=True, want_y=False):
        """solve_staged() with QP b under block b of stage_contact_normals(), for this call alone (srbdqp_solve_staged_normals_f64): nothing is set on the
        engine, and the next solve_staged() is what it would have been.  The general kernel for every contact pattern: its low-latency contact-normals
        instantiation (wrench_f64_n<N>_lat_cn) at N <= 10 and B <= 8, the batch one (wrench_f64_n<N>_cn) otherwise.  A normal that is not finite, has a
        length outside [0.5, 2] or n_z < 0.5 after normalising raises SrbdqpError before anything is launched."""
        self._solve_staged_side("normals", B, use_pcom, use_warm, want_x, want_y)

    def bind_update_normals(self):
        """srbdqp_update_normals_f64 for the QP in row 0 of the staging arrays with every argument bound once, as bind_update_wrench() binds the wrench call:
        inputs, normals and outputs ARE the staging arrays, so the C side copies nothing -> (fn, arguments with pcom, arguments without); rc = fn(*arguments)."""
        return self._bind_update_side("normals")

    def prepare_staged(self, B=1, use_pcom=False):
        """Two-phase call, phase 1 (srbdqp_prepare_staged_f64): set-up of the first B staged QPs from a PREDICTED x0 (whatever the
        staging x0 holds); asynchronous."""
        self._open()
        self._check(self._lib.srbdqp_prepare_staged_f64(self._h, int(B), int(use_pcom)))

    def solve_prepared(self, B=1, want_x=True, want_y=False):
        """Two-phase call, phase 2 (srbdqp_solve_prepared_f64): x0 is read from the staging arrays again, the rest is as prepared."""
        self._open()
        self._check(self._lib.srbdqp_solve_prepared_f64(self._h, int(B), int(want_x), int(want_y)))

    def synchronize(self):
        self._check(self._lib.srbdqp_synchronize(self._h))

    # -- the steps either side of the QP (include/srbdqp_cascade.h) ----------------------------------------
    def swing(self, p_start, p_final, z_middle, progress, final_velocity_z=-0.02, first_half_share=0.80, want_coeff=False):
        """Batched swing-foot trajectory (swing_trajectory.py:38-89): p_start, p_final (B,3); z_middle, progress (B,).
        Returns dict(pos (B,3), vel_z (B,), acc_z (B,)[, coeff (B,7)])."""
        ps, pf = _c(p_start, np.float64).reshape(-1, 3), _c(p_final, np.float64).reshape(-1, 3)
        B = ps.shape[0]
        zm = np.ascontiguousarray(np.broadcast_to(np.asarray(z_middle, np.float64).reshape(-1), (B,)))
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(progress, np.float64).reshape(-1), (B,)))
        if pf.shape[0] != B:
            raise ValueError("p_start and p_final must have the same number of rows")
        pos, vz, az = np.empty((B, 3)), np.empty(B), np.empty(B)
        co = np.empty((B, 7)) if want_coeff else None
        rc = self._lib.srbdqp_swing_f64(self._h, B, _p(ps), _p(pf), _p(zm), _p(t), float(final_velocity_z),
                                        float(first_half_share), _p(pos), _p(vz), _p(az), _p(co))
        self._check(rc)
        out = dict(pos=pos, vel_z=vz, acc_z=az)
        if want_coeff:
            out["coeff"] = co
        return out

    def wbid_reference(self, x_next, u0, foot, as_written=True):
        """Batched MPC -> WBID reference mapping (wbid.py:243-296): x_next (B,13), u0 (B,12), foot (B,12) or (B,4,3).
        Returns dict(R (B,3,3), base_vel (B,6), base_acc (B,6), com_acc (B,3), com_pos (B,3), com_vel (B,3), wrench (B,4,3))."""
        x, u, f = _c(x_next, np.float64).reshape(-1, NX), _c(u0, np.float64).reshape(-1, NU), _c(foot, np.float64).reshape(-1, NU)
        B = x.shape[0]
        if u.shape[0] != B or f.shape[0] != B:
            raise ValueError("x_next, u0 and foot must have the same number of rows")
        R, bv, ba, ca = np.empty((B, 3, 3)), np.empty((B, 6)), np.empty((B, 6)), np.empty((B, 3))
        rc = self._lib.srbdqp_wbid_reference_f64(self._h, B, _p(x), _p(u), _p(f), int(bool(as_written)), _p(R), _p(bv), _p(ba), _p(ca))
        self._check(rc)
        return dict(R=R, base_vel=bv, base_acc=ba, com_acc=ca, com_pos=x[:, 3:6].copy(), com_vel=x[:, 9:12].copy(),
                    wrench=u.reshape(B, 4, 3).copy())

    def _gait_struct(self, period_steps, double_support_steps, com_target, hip_offset_y):
        g = _lib.Gait()
        g.struct_size = C.sizeof(_lib.Gait)
        g.period_steps, g.double_support_steps = int(period_steps), int(double_support_steps)
        for i in range(3):
            g.com_target[i] = float(com_target[i])
        g.hip_offset_y = float(hip_offset_y)
        return g

    def mpc_inputs(self, x0, feet, stamp, v_ref, com_target, standing=None, period_steps=6, double_support_steps=1,
                   hip_offset_y=0.0645):
        """The step before the QP for B robots (msgs.MpcNode.step + msgs.AlternatingGait for one robot):
        x0 (B,13), feet (B,12) or (B,4,3), stamp (B,), v_ref (B,2), standing (B,) flags or None.
        Returns dict(x_ref (B,N,13), foot (B,N,12), contact (B,N,4) uint8, pcom (B,N,3), landing (B,3)) -- the arrays
        solve() / solve_device() take."""
        return self._mpc_inputs("srbdqp_mpc_inputs_f64", x0, feet, stamp, lambda B: [_c(v_ref, np.float64).reshape(B, 2)], standing,
                                (period_steps, double_support_steps, com_target, hip_offset_y))

    def _mpc_inputs(self, fn, x0, feet, stamp, vel, standing, gait, track=None, preview=None):
        """The host form `fn` of the inputs: the marshalling of x0, feet, stamp and standing, the gait struct and the outputs, once for mpc_inputs(),
        mpc_inputs_steered(), mpc_inputs_tracked() and mpc_inputs_previewed().  vel(B): the call's own arrays as it marshals them, v_ref or command first and
        behind a command the pose, which goes in and out.  gait: _gait_struct()'s arguments.  track: track_settings()' keywords in a tracked call.  preview:
        preview_settings()' keywords in a previewed call, which takes the track settings and the pose too (None each: its steered form)."""
        x = _c(x0, np.float64).reshape(-1, NX)
        B, N = x.shape[0], self.N
        f = _c(feet, np.float64).reshape(B, NU)
        t = _c(stamp, np.float64).reshape(B)
        v, *po = vel(B)
        sd = None if standing is None else _c(standing, np.uint8).reshape(B)
        g = self._gait_struct(*gait)
        tail = () if track is None else (C.byref(self.track_settings(**track)), _p(po[0]))
        xr, ft, ct = np.empty((B, N, NX)), np.empty((B, N, NU)), np.empty((B, N, NC), dtype=np.uint8)
        out = dict(x_ref=xr, foot=ft, contact=ct, pcom=np.empty((B, N, 3)), landing=np.empty((B, 3)))
        if v.shape[1] == 3:       # under a command: the heading the next foot lands with
            out["landing_yaw"] = np.empty(B)
        more = {}
        if preview is not None:   # (behind the tracked call's arguments, which are null in the steered form)
            more["previewed"] = np.empty((B, N, NC), dtype=np.uint8)
            tail = (tail or (None, None)) + (C.byref(self.preview_settings(**preview)), _p(more["previewed"]))
        rc = getattr(self._lib, fn)(self._h, B, _p(x), _p(f), _p(t), _p(v), _p(sd), C.byref(g), *(_p(o) for o in out.values()), *tail)
        self._check(rc)
        out.update(more)
        return dict(out, pose=po[0]) if po else out

    def mpc_inputs_device(self, B, x0, feet, stamp, v_ref, com_target, x_ref, foot, contact, pcom, landing=0, standing=0,
                          period_steps=6, double_support_steps=1, hip_offset_y=0.0645, stream=0):
        """Device-pointer form of mpc_inputs(): raw addresses in, launch enqueued behind `stream`, returns at once."""
        v = lambda q: C.c_void_p(int(q)) if q else None
        g = self._gait_struct(period_steps, double_support_steps, com_target, hip_offset_y)
        rc = self._lib.srbdqp_mpc_inputs_device_f64(self._h, int(B), v(x0), v(feet), v(stamp), v(v_ref), v(standing), C.byref(g),
                                                    v(x_ref), v(foot), v(contact), v(pcom), v(landing), v(stream))
        self._check(rc)

    def mpc_inputs_steered(self, x0, feet, stamp, command, com_target, standing=None, period_steps=6, double_support_steps=1, hip_offset_y=0.0645):
        """mpc_inputs() under command (B,3) = (vx, vy, wz) -- planar velocity in the robot's heading frame and yaw rate -- in place of v_ref
        (srbdqp_mpc_inputs_steered_f64): the references turn with the commanded heading, the landing point's hip offset with the heading
        at mid-swing.  A command that is not finite raises SrbdqpError.
        Returns mpc_inputs()' dict and landing_yaw (B,), the heading the next foot lands with: fleet_advance(landing_yaw=)'s argument."""
        return self._mpc_inputs("srbdqp_mpc_inputs_steered_f64", x0, feet, stamp, lambda B: [_as(command, np.float64, (B, 3), "command")], standing,
                                (period_steps, double_support_steps, com_target, hip_offset_y))

    def mpc_inputs_steered_device(self, B, x0, feet, stamp, command, com_target, x_ref, foot, contact, pcom, landing=0, landing_yaw=0, standing=0,
                                  period_steps=6, double_support_steps=1, hip_offset_y=0.0645, stream=0):
        """Device-pointer form of mpc_inputs_steered(): raw addresses in, launch enqueued behind `stream`, returns at once.  A command that is not finite
        gives that robot references that are not numbers, which its solve answers with status -1 and zero forces."""
        v = lambda q: C.c_void_p(int(q)) if q else None
        g = self._gait_struct(period_steps, double_support_steps, com_target, hip_offset_y)
        rc = self._lib.srbdqp_mpc_inputs_steered_device_f64(self._h, int(B), v(x0), v(feet), v(stamp), v(command), v(standing), C.byref(g),
                                                            v(x_ref), v(foot), v(contact), v(pcom), v(landing), v(landing_yaw), v(stream))
        self._check(rc)

    # -- a fleet that follows its path: the inputs from a carried reference pose (include/srbdqp_cascade.h) ------
    def track_settings(self, lead_max=0.1, yaw_lead_max=0.3):
        """srbdqp_track_settings for mpc_inputs_tracked() / rollout(track=): how far the reference pose may lie from the measured position (m) and from the
        measured yaw (rad) before it is pulled back; both finite and positive."""
        s = _lib.TrackSettings()
        s.struct_size = C.sizeof(_lib.TrackSettings)
        s.lead_max, s.yaw_lead_max = float(lead_max), float(yaw_lead_max)
        return s

    def _track_arg(self, track):
        """rollout()'s track=: True (the defaults), a dict of track_settings()' keywords, or a TrackSettings."""
        if isinstance(track, _lib.TrackSettings):
            return track
        return self.track_settings(**({} if track is True else dict(track)))

    def mpc_inputs_tracked(self, x0, feet, stamp, command, pose, com_target, standing=None, period_steps=6, double_support_steps=1, hip_offset_y=0.0645,
                           **track):
        """mpc_inputs_steered() with the references taken from pose (B,3) = (qx, qy, th), a reference position and an unwrapped reference heading that the
        caller carries from step to step (srbdqp_mpc_inputs_tracked_f64): the pose is first bounded to within lead_max and yaw_lead_max
        of the measured state, the references start from it whether the robot moves or not, and it moves on by one control step under the command.  pcom,
        foot, contact, landing and landing_yaw are mpc_inputs_steered()'s.  track: track_settings()' keywords.  pose is not modified; a pose or a command
        that is not finite raises SrbdqpError.
        Returns mpc_inputs_steered()'s dict and pose (B,3), the pose behind the step: the next call's argument."""
        return self._mpc_inputs("srbdqp_mpc_inputs_tracked_f64", x0, feet, stamp,
                                lambda B: [_as(command, np.float64, (B, 3), "command"), np.array(_as(pose, np.float64, (B, 3), "pose"))], standing,
                                (period_steps, double_support_steps, com_target, hip_offset_y), track)

    def mpc_inputs_tracked_device(self, B, x0, feet, stamp, command, pose, com_target, x_ref, foot, contact, pcom, landing=0, landing_yaw=0, standing=0,
                                  period_steps=6, double_support_steps=1, hip_offset_y=0.0645, stream=0, **track):
        """Device-pointer form of mpc_inputs_tracked(): raw addresses in, pose (B,3) updated in place, launch enqueued behind `stream`, returns at once.  A
        state or a pose that is not finite clamps nothing; a pose or a command that is not finite gives that robot references that are not numbers and leaves
        its pose where the bound left it."""
        v = lambda q: C.c_void_p(int(q)) if q else None
        g = self._gait_struct(period_steps, double_support_steps, com_target, hip_offset_y)
        k = self.track_settings(**track)
        rc = self._lib.srbdqp_mpc_inputs_tracked_device_f64(self._h, int(B), v(x0), v(feet), v(stamp), v(command), v(standing), C.byref(g),
                                                            v(x_ref), v(foot), v(contact), v(pcom), v(landing), v(landing_yaw), C.byref(k), v(pose), v(stream))
        self._check(rc)

    # -- a fleet that previews its footholds along the horizon (include/srbdqp_cascade.h) -----------------------
    def preview_settings(self, foot_half_length=0.085):
        """srbdqp_preview_settings for mpc_inputs_previewed() / rollout(preview=): how far heel and toe of a previewed foothold lie behind and ahead of its
        landing point -- the plant's fleet_settings() value; finite and positive."""
        s = _lib.PreviewSettings()
        s.struct_size = C.sizeof(_lib.PreviewSettings)
        s.foot_half_length = float(foot_half_length)
        return s

    def mpc_inputs_previewed(self, x0, feet, stamp, command, com_target, pose=None, standing=None, period_steps=6, double_support_steps=1,
                             hip_offset_y=0.0645, foot_half_length=0.085, **track):
        """mpc_inputs_steered() -- with pose (B,3), mpc_inputs_tracked(), track: track_settings()' keywords -- whose foot (B,N,12) previews the footholds
        along the horizon (srbdqp_mpc_inputs_previewed_f64): from the step at which a foot touches down under the gait, its two contacts
        stand on the heel and toe the plant will put down there -- the landing point and the heading at mid-swing of the state predicted for that step.  Every
        other output is the steered or tracked call's, bit for bit.
        Returns that call's dict and previewed (B,N,4) uint8: 1 where foot holds a previewed point."""
        vel = (lambda B: [_as(command, np.float64, (B, 3), "command")]) if pose is None else \
              (lambda B: [_as(command, np.float64, (B, 3), "command"), np.array(_as(pose, np.float64, (B, 3), "pose"))])
        return self._mpc_inputs("srbdqp_mpc_inputs_previewed_f64", x0, feet, stamp, vel, standing, (period_steps, double_support_steps, com_target, hip_offset_y),
                                None if pose is None else track, dict(foot_half_length=foot_half_length))

    def mpc_inputs_previewed_device(self, B, x0, feet, stamp, command, com_target, x_ref, foot, contact, pcom, landing=0, landing_yaw=0, standing=0, pose=0,
                                    previewed=0, period_steps=6, double_support_steps=1, hip_offset_y=0.0645, foot_half_length=0.085, stream=0, **track):
        """Device-pointer form of mpc_inputs_previewed(): raw addresses in, launch enqueued behind `stream`, returns at once.  pose: the address of (B,3) poses,
        updated in place -- the tracked form --, or 0 for the steered form; previewed: the address of (B,N,4) bytes, or 0."""
        v = lambda q: C.c_void_p(int(q)) if q else None
        g = self._gait_struct(period_steps, double_support_steps, com_target, hip_offset_y)
        k = self.track_settings(**track) if pose else None
        pr = self.preview_settings(foot_half_length)
        rc = self._lib.srbdqp_mpc_inputs_previewed_device_f64(self._h, int(B), v(x0), v(feet), v(stamp), v(command), v(standing), C.byref(g), v(x_ref), v(foot),
                                                              v(contact), v(pcom), v(landing), v(landing_yaw), C.byref(k) if pose else None, v(pose), C.byref(pr),
                                                              v(previewed), v(stream))
        self._check(rc)

    # -- from step t to step t + 1: the fleet's plant step and the K-step loop (include/srbdqp_cascade.h) --------
    def fleet_settings(self, com_target=(0.0, 0.0, 0.0), substeps=10, foot_half_length=0.085, z_min=0.3, tilt_max=1.0, period_steps=6,
                       double_support_steps=1, hip_offset_y=0.0645):
        """srbdqp_fleet_settings for fleet_advance() / rollout(): the plant's substeps, the touchdown's heel / toe spacing, the fallen thresholds and the gait
        (mpc_inputs()' schedule; com_target matters to the roll-out alone)."""
        s = _lib.FleetSettings()
        s.struct_size = C.sizeof(_lib.FleetSettings)
        s.substeps = int(substeps)
        s.foot_half_length, s.z_min, s.tilt_max = float(foot_half_length), float(z_min), float(tilt_max)
        s.gait = self._gait_struct(period_steps, double_support_steps, com_target, hip_offset_y)
        return s

    def fleet_advance(self, x, feet, stamp, u0, landing, standing=None, push=None, alive=None, landing_yaw=None, **settings):
        """One control period of B robots between two solves (srbdqp_fleet_advance_f64): the nonlinear SRBD plant under the first-step forces u0 (B,12) at
        the contact points feet (B,12) or (B,4,3), the gait clock, the touchdown of the foot that lands around landing (B,3) (mpc_inputs()' output), the
        robots that fell.  standing (B,) flags, push (B,6) world wrench on the body during the period (torque first; the MPC does not know it), alive (B,)
        flags: each or None.  settings: fleet_settings()' keywords.  The inputs are not modified.  With a map set (set_terrain()) a foot that touches
        down stands on the map, heel and toe each at the height under it, and "fallen" compares the CoM's height over the ground under it with z_min
        (kernel_name() "fleet_advance_terrain_f64").  landing_yaw (B,) (mpc_inputs_steered()'s output) or None: heel and toe of a foot that touches down
        lie along that heading (srbdqp_fleet_advance_steered_f64) where they lie along the world's x axis without it.
        Returns dict(x (B,13), feet (B,12), stamp (B,), alive (B,) uint8)."""
        x = np.array(x, dtype=np.float64).reshape(-1, NX)
        B = x.shape[0]
        f = np.array(feet, dtype=np.float64).reshape(B, NU)
        t = np.array(stamp, dtype=np.float64).reshape(B)
        u = _as(u0, np.float64, (B, NU), "u0")
        lp = _as(landing, np.float64, (B, 3), "landing")
        sd = None if standing is None else _as(np.asarray(standing) != 0, np.uint8, (B,), "standing")
        pu = None if push is None else _as(push, np.float64, (B, 6), "push")
        al = np.ones(B, np.uint8) if alive is None else np.array(np.asarray(alive) != 0, dtype=np.uint8).reshape(B)
        s = self.fleet_settings(**settings)
        ly = None if landing_yaw is None else _as(landing_yaw, np.float64, (B,), "landing_yaw")
        # (the steered call takes landing_yaw behind landing)
        fn, yaw = (self._lib.srbdqp_fleet_advance_f64, ()) if ly is None else (self._lib.srbdqp_fleet_advance_steered_f64, (_p(ly),))
        self._check(fn(self._h, B, _p(x), _p(f), _p(t), _p(u), NU, _p(lp), *yaw, _p(sd), _p(pu), _p(al), C.byref(s)))
        return dict(x=x, feet=f, stamp=t, alive=al)

    def fleet_advance_device(self, B, x, feet, stamp, u0, landing, u0_stride=NU, standing=0, push=0, alive=0, stream=0, landing_yaw=0, **settings):
        """Device-pointer form of fleet_advance(): raw addresses, x / feet / stamp / alive updated in place, launch enqueued behind `stream`, returns at once.
        u0_stride (doubles between the forces of consecutive robots): 12 N reads u_out[b][0] of a solve_device() in place.  landing_yaw: the address of
        (B,) headings, or 0 for the unsteered step."""
        v = lambda q: C.c_void_p(int(q)) if q else None
        s = self.fleet_settings(**settings)
        fn, yaw = (self._lib.srbdqp_fleet_advance_steered_device_f64, (v(landing_yaw),)) if landing_yaw else (self._lib.srbdqp_fleet_advance_device_f64, ())
        self._check(fn(self._h, int(B), v(x), v(feet), v(stamp), v(u0), int(u0_stride), v(landing), *yaw, v(standing), v(push), v(alive), C.byref(s), v(stream)))

    # -- a fleet that feels its pushes: the momentum observer (include/srbdqp_cascade.h) -------------------------
    def observer_settings(self, gain=0.5, horizon_decay=1.0, torque_max=50.0, force_max=200.0):
        """srbdqp_observer_settings for wrench_observer() / rollout(observer=): the filter's gain in (0, 1], the estimate's decay along the horizon in
        [0, 1], the clamps of its torque (N m) and force (N) components."""
        s = _lib.ObserverSettings()
        s.struct_size = C.sizeof(_lib.ObserverSettings)
        s.gain, s.horizon_decay, s.torque_max, s.force_max = float(gain), float(horizon_decay), float(torque_max), float(force_max)
        return s

    def _observer_arg(self, observer):
        """rollout()'s observer=: True (the defaults), a dict of observer_settings()' keywords, or an ObserverSettings."""
        if isinstance(observer, _lib.ObserverSettings):
            return observer
        return self.observer_settings(**({} if observer is True else dict(observer)))

    def wrench_observer(self, x_prev, x_next, feet_prev, u0, w_est, alive=None, want_ew=True, **settings):
        """The momentum observer over one control period of B robots (srbdqp_wrench_observer_f64): from the states before and behind the period (B,13),
        the contact points the forces acted at, feet_prev (B,12) or (B,4,3) -- the feet BEFORE any touchdown --, and the held first-step forces u0 (B,12),
        the wrench on the body that the forces do not explain, filtered into w_est (B,6) ([torque about the CoM, force], world frame; not modified).
        alive (B,) flags as they stand behind the period, or None: a robot that is down, or whose states are not finite, keeps its estimate.  Robot records
        set on the engine (set_robots()) give robot b's own mass and inertia.  settings: observer_settings()' keywords.
        Returns dict(w_est (B,6), ew (B,N,6) = w_est decay^k: set_external_wrench()'s argument for the next solve, or None without want_ew)."""
        x0 = _c(x_prev, np.float64).reshape(-1, NX)
        B = x0.shape[0]
        x1 = _as(x_next, np.float64, (B, NX), "x_next")
        f = _as(feet_prev, np.float64, (B, NU), "feet_prev")
        u = _as(u0, np.float64, (B, NU), "u0")
        al = None if alive is None else _as(np.asarray(alive) != 0, np.uint8, (B,), "alive")
        w = np.array(w_est, dtype=np.float64).reshape(B, 6)
        ew = np.empty((B, self.N, 6)) if want_ew else None
        s = self.observer_settings(**settings)
        self._check(self._lib.srbdqp_wrench_observer_f64(self._h, B, _p(x0), _p(x1), _p(f), _p(u), NU, _p(al), C.byref(s), _p(w), _p(ew)))
        return dict(w_est=w, ew=ew)

    def wrench_observer_device(self, B, x_prev, x_next, feet_prev, u0, w_est, ew=0, u0_stride=NU, alive=0, stream=0, **settings):
        """Device-pointer form of wrench_observer(): raw addresses, w_est updated in place, ew (B,N,6) written where given, launch enqueued behind `stream`,
        returns at once.  u0_stride: 12 N reads u_out[b][0] of a solve_device() in place."""
        v = lambda q: C.c_void_p(int(q)) if q else None
        s = self.observer_settings(**settings)
        self._check(self._lib.srbdqp_wrench_observer_device_f64(self._h, int(B), v(x_prev), v(x_next), v(feet_prev), v(u0), int(u0_stride), v(alive),
                                                                C.byref(s), v(w_est), v(ew), v(stream)))

    def rollout(self, x0, feet, stamp, v_ref, steps, com_target, standing=None, push=None, alive=None, observer=None, w_est=None, command=None, track=None,
                pose=None, preview=None, **settings):
        """`steps` control steps of B robots on the device (srbdqp_fleet_rollout_f64): per step mpc_inputs -> the solve -> fleet_advance, without a host
        round trip in between.  x0 (B,13), feet (B,12) or (B,4,3), stamp (B,), v_ref (B,2) and standing (B,) flags or None (both constant over the call),
        push (steps,B,6) world wrenches or None, alive (B,) flags or None.  settings: fleet_settings()' keywords.  Robot records and weights set on the
        engine are honoured; an external wrench or contact normals set on it raise SrbdqpError.  A second call from the returned x, feet, stamp and alive
        continues the first one bit for bit.  With a map set (set_terrain()) the fleet walks on it: per step mpc_inputs -> terrain_inputs -> the solve
        on the general kernel with those normals as the normals of the call -> the terrain plant step; robot records, weights, a wrench or normals set
        on the engine, a live horizon, rank-aware steps, N = 24 and a kernel= that bars the general kernel then raise SrbdqpError ("while a terrain is
        set").
        observer=True or a dict of observer_settings()' keywords: the observed roll-out (srbdqp_fleet_rollout_observed_f64, flat ground): behind every
        plant step the momentum observer estimates the push from what the plant did, and the next solve reads the estimate as its external wrench
        (wrench_f64_n<N>_ew) -- the estimate of period t serves solve t + 1.  w_est (B,6): the estimate to start from (None: zeros); carried from one
        call to the next, chunks compose bit for bit.  The result then has w_est (B,6) and w_log (steps,B,6), the estimate behind every period.
        Contact normals, a wrench or a terrain set on the engine, a live horizon, rank-aware steps, N = 24 and a kernel= that bars the general kernel
        raise SrbdqpError; robot records and weights are honoured.  observer=None is the call without an observer.
        command (B,3) or (steps,B,3), with v_ref=None: the steered roll-out (srbdqp_fleet_rollout_steered_f64) -- (vx, vy, wz), planar
        velocity in each robot's heading frame and yaw rate, held over the call or a row per step; per step mpc_inputs_steered -> the solve ->
        fleet_advance(landing_yaw=), on flat ground, on a map, or with observer=.  command=None is the call as it was.
        track=True or a dict of track_settings()' keywords, with command=: the tracked roll-out (srbdqp_fleet_rollout_tracked_f64) --
        mpc_inputs_tracked in place of mpc_inputs_steered: the references come from a pose (B,3) = (qx, qy, th) that moves on with the commands and is kept
        within lead_max and yaw_lead_max of the robot, so that the fleet ends where its commands lead.  pose=None starts on the measured (x0[3:5], x0[2]);
        carried from one call to the next, chunks compose bit for bit.  The result then has pose (B,3) and pose_log (steps,B,3), the pose behind every
        step.  track=None is the call as it was.
        preview=True, with command=: the previewed roll-out (srbdqp_fleet_rollout_previewed_f64) -- mpc_inputs_previewed in place of the
        steered or tracked inputs, and on a map terrain_inputs_previewed: every solve reads the footholds its robot will stand on along the horizon, with the
        plant's own foot_half_length.  It works with track=, observer= and a map as the steered roll-out does.  preview=None is the call as it was.
        Returns dict(x (steps+1,B,13), u0 (steps,B,12), feet (steps+1,B,12), status (steps,B), iters (steps,B), alive (B,) uint8, stamp (B,))."""
        x = np.array(x0, dtype=np.float64).reshape(-1, NX)
        B, T = x.shape[0], int(steps)
        f = np.array(feet, dtype=np.float64).reshape(B, NU)
        t = np.array(stamp, dtype=np.float64).reshape(B)
        if command is not None:
            if v_ref is not None:
                raise ValueError("rollout: command= replaces v_ref (pass v_ref=None): a steered roll-out takes its velocity in the heading frame")
            cm = np.asarray(command, dtype=np.float64)
            cm = _as(cm, np.float64, (B, 3) if cm.ndim < 3 else (max(T, 0), B, 3), "command")
        else:
            v = _as(v_ref, np.float64, (B, 2), "v_ref")
        sd = None if standing is None else _as(np.asarray(standing) != 0, np.uint8, (B,), "standing")
        pu = None if push is None else _as(push, np.float64, (max(T, 0), B, 6), "push")
        al = np.ones(B, np.uint8) if alive is None else np.array(np.asarray(alive) != 0, dtype=np.uint8).reshape(B)
        s = self.fleet_settings(com_target, **settings)
        n = max(T, 0)
        xl, ul, fl = np.empty((n + 1, B, NX)), np.empty((n, B, NU)), np.empty((n + 1, B, NU))
        sl, il = np.empty((n, B), np.int32), np.empty((n, B), np.int32)
        observed = observer is not None and observer is not False
        if w_est is not None and not observed:
            raise ValueError("rollout: w_est belongs to an observed roll-out (observer=)")
        tracked = track is not None and track is not False
        if tracked and command is None:
            raise ValueError("rollout: track= follows a command schedule (command=): there is no path without one")
        if pose is not None and not tracked:
            raise ValueError("rollout: pose belongs to a tracked roll-out (track=)")
        previewed = preview is not None and preview is not False
        if previewed and command is None:
            raise ValueError("rollout: preview= previews the footholds of a commanded roll-out (command=)")
        out = dict(x=xl, u0=ul, feet=fl, status=sl, iters=il, alive=al, stamp=t)
        obs = ()
        if observed:
            o = self._observer_arg(observer)
            out.update(w_est=np.zeros((B, 6)) if w_est is None else np.array(w_est, dtype=np.float64).reshape(B, 6), w_log=np.empty((n, B, 6)))
            obs = (C.byref(o), _p(out["w_est"]), _p(out["w_log"]))
        if command is not None:     # (one steered call, with its observer or without)
            fn, vel, obs = self._lib.srbdqp_fleet_rollout_steered_f64, (_p(cm), 1 if cm.ndim == 2 else T), obs or (None, None, None)
            if tracked:             # (... and the tracked call takes its settings, pose and pose_log behind the observer's)
                k = self._track_arg(track)
                po = np.concatenate([x[:, 3:5], x[:, 2:3]], axis=1) if pose is None else np.array(_as(pose, np.float64, (B, 3), "pose"))
                out.update(pose=np.ascontiguousarray(po), pose_log=np.empty((n, B, 3)))
                fn, obs = self._lib.srbdqp_fleet_rollout_tracked_f64, obs + (C.byref(k), _p(out["pose"]), _p(out["pose_log"]))
            if previewed:           # (... and the previewed call its settings behind the tracked call's, which are null in its steered form)
                pr = self.preview_settings(s.foot_half_length)
                fn, obs = self._lib.srbdqp_fleet_rollout_previewed_f64, (obs if tracked else obs + (None, None, None)) + (C.byref(pr),)
        else:
            fn, vel = self._lib.srbdqp_fleet_rollout_observed_f64 if observed else self._lib.srbdqp_fleet_rollout_f64, (_p(v),)
        self._check(fn(self._h, B, T, _p(x), _p(f), _p(t), *vel, _p(sd), _p(pu), C.byref(s), _p(al), _p(xl), _p(ul), _p(fl), _p(sl), _p(il), *obs))
        return out

    def rollout_device(self, B, steps, x, feet, stamp, v_ref, com_target, standing=0, push=0, alive=0, x_log=0, u0_log=0, feet_log=0, status_log=0,
                       iters_log=0, stream=0, observer=None, w_est=0, w_log=0, command=0, command_steps=1, track=None, pose=0, pose_log=0, preview=None,
                       **settings):
        """Device-pointer form of rollout(): raw addresses (0 = absent), x / feet / stamp / alive updated in place, every launch enqueued behind `stream`
        (0 = the engine's own), returns at once without synchronising.  Logs as in include/srbdqp_cascade.h.  observer= as in rollout(): w_est (B,6),
        required then, is updated in place; w_log (steps,B,6) or 0.  command: the address of (B,3) commands (command_steps=1) or of (steps,B,3)
        (command_steps=steps) -- the steered roll-out, v_ref 0 then; 0: the call as it was.  track= as in rollout(), with command: pose (B,3), required
        then, is updated in place; pose_log (steps,B,3) or 0.  preview= as in rollout(), with command."""
        v = lambda q: C.c_void_p(int(q)) if q else None
        s = self.fleet_settings(com_target, **settings)
        if command and v_ref:
            raise ValueError("rollout_device: command= replaces v_ref (pass v_ref=0)")
        observed = observer is not None and observer is not False
        if (w_est or w_log) and not observed:
            raise ValueError("rollout_device: w_est and w_log belong to an observed roll-out (observer=)")
        obs = ()
        if observed:
            o = self._observer_arg(observer)
            obs = (C.byref(o), v(w_est), v(w_log))
        tracked = track is not None and track is not False
        if tracked and not command:
            raise ValueError("rollout_device: track= follows a command schedule (command=): there is no path without one")
        if (pose or pose_log) and not tracked:
            raise ValueError("rollout_device: pose and pose_log belong to a tracked roll-out (track=)")
        previewed = preview is not None and preview is not False
        if previewed and not command:
            raise ValueError("rollout_device: preview= previews the footholds of a commanded roll-out (command=)")
        if command:     # (one steered call, with its observer or without)
            fn, vel, obs = self._lib.srbdqp_fleet_rollout_steered_device_f64, (v(command), int(command_steps)), obs or (None, None, None)
            if tracked:
                k = self._track_arg(track)
                fn, obs = self._lib.srbdqp_fleet_rollout_tracked_device_f64, obs + (C.byref(k), v(pose), v(pose_log))
            if previewed:
                pr = self.preview_settings(s.foot_half_length)
                fn, obs = self._lib.srbdqp_fleet_rollout_previewed_device_f64, (obs if tracked else obs + (None, None, None)) + (C.byref(pr),)
        else:
            fn, vel = self._lib.srbdqp_fleet_rollout_observed_device_f64 if observed else self._lib.srbdqp_fleet_rollout_device_f64, (v(v_ref),)
        self._check(fn(self._h, int(B), int(steps), v(x), v(feet), v(stamp), *vel, v(standing), v(push), C.byref(s), v(alive), v(x_log), v(u0_log), v(feet_log),
                       v(status_log), v(iters_log), *obs, v(stream)))

    # -- the ground under the fleet (include/srbdqp_cascade.h) ---------------------------------------------------
    def set_terrain(self, heights, origin=(0.0, 0.0), cell=None):
        """A height map for fleet_advance() and rollout() (srbdqp_set_terrain): heights (ny, nx), node (i, j) = heights[j, i] at (origin[0] + i cell,
        origin[1] + j cell); checked and copied by the library -- finite, at least 2 x 2, neighbouring nodes at most 1.2 cell apart in height.  None
        clears it (flat ground again).  Every solve of the engine is untouched."""
        if heights is None:
            self._check(self._lib.srbdqp_set_terrain(self._h, None, None))
            return
        if cell is None:
            raise ValueError("set_terrain: pass cell, the node spacing in metres")
        hm = np.ascontiguousarray(heights, dtype=np.float64)
        if hm.ndim != 2:
            raise ValueError(f"set_terrain: expected heights of shape (ny, nx), got {hm.shape}")
        t = _lib.Terrain()
        t.struct_size = C.sizeof(_lib.Terrain)
        t.ny, t.nx = (min(int(n), 2 ** 31 - 1) for n in hm.shape)
        t.x0, t.y0, t.cell = float(origin[0]), float(origin[1]), float(cell)
        self._check(self._lib.srbdqp_set_terrain(self._h, C.byref(t), _p(hm)))

    def terrain_sample(self, xy, want_normal=True):
        """The map at M points (srbdqp_terrain_sample_f64): xy (M,2) -> dict(z (M,)[, normal (M,3)]): bilinear height and unit normal; a point off the
        map is the clamped point, a non-finite coordinate gives z = NaN and the normal (0, 0, 1)."""
        p = _c(xy, np.float64).reshape(-1, 2)
        M = p.shape[0]
        z = np.empty(M)
        n = np.empty((M, 3)) if want_normal else None
        self._check(self._lib.srbdqp_terrain_sample_f64(self._h, M, _p(p), _p(z), _p(n)))
        return dict(z=z, normal=n) if want_normal else dict(z=z)

    def terrain_sample_device(self, M, xy, z, normal=0, stream=0):
        """Device-pointer form of terrain_sample(): raw addresses, launch enqueued behind `stream`, returns at once."""
        v = lambda q: C.c_void_p(int(q)) if q else None
        self._check(self._lib.srbdqp_terrain_sample_device_f64(self._h, int(M), v(xy), v(z), v(normal), v(stream)))

    def terrain_inputs(self, feet, x_ref):
        """Between mpc_inputs() and the solve on a map (srbdqp_terrain_inputs_f64): feet (B,12) or (B,4,3), x_ref (B,N,13) (not modified).
        Returns dict(x_ref (B,N,13): column 5 raised by the mean height of the robot's four contact points, normals (B,N,12): the map's normal under
        every contact point at every step -- what set_contact_normals() / solve(normals=) take)."""
        f = _c(feet, np.float64).reshape(-1, NU)
        B, N = f.shape[0], self.N
        xr = np.array(x_ref, dtype=np.float64).reshape(B, N, NX)
        cn = np.empty((B, N, NU))
        self._check(self._lib.srbdqp_terrain_inputs_f64(self._h, B, _p(f), _p(xr), _p(cn)))
        return dict(x_ref=xr, normals=cn)

    def terrain_inputs_device(self, B, feet, x_ref, normals, stream=0):
        """Device-pointer form of terrain_inputs(): raw addresses, x_ref updated in place, launch enqueued behind `stream`, returns at once."""
        v = lambda q: C.c_void_p(int(q)) if q else None
        self._check(self._lib.srbdqp_terrain_inputs_device_f64(self._h, int(B), v(feet), v(x_ref), v(normals), v(stream)))

    def terrain_inputs_previewed(self, foot, previewed, x_ref):
        """terrain_inputs() between mpc_inputs_previewed() and the solve (srbdqp_terrain_inputs_previewed_f64): foot (B,N,12),
        previewed (B,N,4) or None, x_ref (B,N,13); none is modified.
        Returns dict(foot (B,N,12): every previewed point at the map's height under it, x_ref (B,N,13): column 5 of step k raised by the mean height of
        foot[:, k], normals (B,N,12): the map's normal under every contact point of every step)."""
        N = self.N
        fo = np.array(foot, dtype=np.float64).reshape(-1, N, NU)
        B = fo.shape[0]
        pv = None if previewed is None else _as(np.asarray(previewed) != 0, np.uint8, (B, N, NC), "previewed")
        xr = np.array(x_ref, dtype=np.float64).reshape(B, N, NX)
        cn = np.empty((B, N, NU))
        self._check(self._lib.srbdqp_terrain_inputs_previewed_f64(self._h, B, _p(fo), _p(pv), _p(xr), _p(cn)))
        return dict(foot=fo, x_ref=xr, normals=cn)

    def terrain_inputs_previewed_device(self, B, foot, previewed, x_ref, normals, stream=0):
        """Device-pointer form of terrain_inputs_previewed(): raw addresses, foot and x_ref updated in place, launch enqueued behind `stream`, returns at once."""
        v = lambda q: C.c_void_p(int(q)) if q else None
        self._check(self._lib.srbdqp_terrain_inputs_previewed_device_f64(self._h, int(B), v(foot), v(previewed), v(x_ref), v(normals), v(stream)))

    def last_kernel_ms(self) -> float:
        return float(self._lib.srbdqp_last_kernel_ms(self._h))

    def last_kernel_parts_ms(self):
        """(set-up ms, ADMM ms) of the last timed solve when it ran as the split pipeline, else None."""
        a, b = C.c_double(), C.c_double()
        if self._lib.srbdqp_last_kernel_parts_ms(self._h, C.byref(a), C.byref(b)) != _lib.OK:
            return None
        return float(a.value), float(b.value)

    def kernel_name(self) -> str:
        return self._lib.srbdqp_kernel_name(self._h).decode()

    def batch1_launch_path(self) -> str:
        """"aql" (the library's own HSA queue) or "hip: <why>" for the staged one-QP call; "undecided" before the first one."""
        return self._lib.srbdqp_batch1_launch_path(self._h).decode()


class RaggedMPC(_Engine):
    """Mixed-horizon batches (BASELINE.json configs[4]) over srbdqp_solve_ragged_*: QPs in any order, each with its own
    horizon and contact schedule; the library sorts them into horizon buckets and launches every bucket on its own HIP
    stream, all in flight together."""
    _CREATE, _DESTROY, _LAST_ERROR = "srbdqp_ragged_create", "srbdqp_ragged_destroy", "srbdqp_ragged_last_error"

    def __init__(self, horizons=(8, 12, 16, 24), dt: float = 0.04, device: int = 0, **overrides):
        cfg = _lib.default_config()
        cfg.dt = float(dt)
        cfg.device = int(device)
        _apply_overrides(cfg, overrides)
        self.horizons = tuple(int(h) for h in horizons)
        if any(h not in _lib.HORIZONS for h in self.horizons):   # buckets at any horizon 1 ... 24 (SRBDQP_FLAG_ANY_HORIZON)
            cfg.flags |= _lib.FLAG_ANY_HORIZON
        hz = np.ascontiguousarray(self.horizons, dtype=np.int32)
        self._create(cfg, _ptr(hz), len(hz))

    def solve_packed(self, N_per_qp, x0, x_ref, foot, contact, want_x=True, dtype=np.float64):
        """Step-major packed host arrays (include/srbdqp.h): x0 (B,13), x_ref (sum N,13), foot (sum N,12), contact (sum N,4).
        Returns dict(u (sum N,12), x (sum N + B,13), status (B,), iters (B,), off (B+1,) row offsets).
        dtype=np.float32: fp32 buffers and iterations (srbdqp_solve_ragged_f32)."""
        dt = np.dtype(dtype)
        Nq = np.ascontiguousarray(N_per_qp, dtype=np.int32)
        B, rows = Nq.size, int(Nq.sum())
        x0 = _as(x0, dt, (B, NX), "x0")
        x_ref = _as(x_ref, dt, (rows, NX), "x_ref")
        foot = _as(foot, dt, (rows, NU), "foot")
        contact = _as(np.asarray(contact) != 0, np.uint8, (rows, NC), "contact")
        u = np.empty((rows, NU), dt); x = np.empty((rows + B, NX), dt) if want_x else None
        status = np.empty(B, np.int32); iters = np.empty(B, np.int32)
        fn = self._lib.srbdqp_solve_ragged_f64 if dt == np.dtype(np.float64) else self._lib.srbdqp_solve_ragged_f32
        self._check(fn(self._h, B, _ptr(Nq), _ptr(x0), _ptr(x_ref), _ptr(foot), _ptr(contact), _ptr(u), _ptr(x), _ptr(status), _ptr(iters)))
        return dict(u=u, x=x, status=status, iters=iters, off=np.concatenate([[0], np.cumsum(Nq)]))

    def solve_device(self, B, N_per_qp, x0, x_ref, foot, contact, u_out, x_out=0, status=0, iters=0, stream=0, f32=False,
                     warm_u=0, warm_y=0, y_out=0):
        """Packed arrays resident in HBM (raw device addresses); N_per_qp is a HOST int32 array.  Does not synchronise.
        f32=True: float32 buffers and iterations.  warm_u (sum N,12) [N] / warm_y (sum N,20) / y_out (sum N,20): warm start in,
        dual solution out (srbdqp_solve_ragged_warm_device_*)."""
        Nq = np.ascontiguousarray(N_per_qp, dtype=np.int32)
        v = lambda p: C.c_void_p(int(p)) if p else None
        if warm_u or warm_y or y_out:
            fn = self._lib.srbdqp_solve_ragged_warm_device_f32 if f32 else self._lib.srbdqp_solve_ragged_warm_device_f64
            self._check(fn(self._h, int(B), _ptr(Nq), v(x0), v(x_ref), v(foot), v(contact), v(warm_u), v(warm_y), v(u_out), v(x_out),
                           v(y_out), v(status), v(iters), v(stream)))
        else:
            fn = self._lib.srbdqp_solve_ragged_device_f32 if f32 else self._lib.srbdqp_solve_ragged_device_f64
            self._check(fn(self._h, int(B), _ptr(Nq), v(x0), v(x_ref), v(foot), v(contact), v(u_out), v(x_out), v(status), v(iters), v(stream)))

    def set_robots(self, robots):
        """One robot per QP, in the CALLER's QP order (srbdqp_ragged_set_robots): as BatchMPC.set_robots."""
        _set_side(self, "srbdqp_ragged_set_robots", "_robots", _robots_arg(robots))

    def set_weights(self, weights):
        """One pair of cost weights per QP, in the CALLER's QP order (srbdqp_ragged_set_weights): as BatchMPC.set_weights."""
        _set_side(self, "srbdqp_ragged_set_weights", "_weights", _weights_arg(weights))

    def set_external_wrench(self, w):
        """A known wrench per horizon row, (rows, 6), packed step-major like x_ref in the CALLER's QP order (srbdqp_ragged_set_external_wrench): as
        BatchMPC.set_external_wrench."""
        _set_side(self, "srbdqp_ragged_set_external_wrench", "_ext_wrench", _ext_wrench_arg(w, (6,)))

    def flush(self, stream=0):
        """flags=FLAG_DEFER_TAIL: make `stream` (0 = the object's own) wait for the restart passes still running on the buckets' tail streams
        (srbdqp_ragged_flush).  Does not synchronise.  The input and output arrays of the earlier solve_device() calls must stay untouched until the
        flush has completed in stream order (the passes read the former and write the latter)."""
        self._check(self._lib.srbdqp_ragged_flush(self._h, C.c_void_p(int(stream)) if stream else None))

    def solve(self, problems):
        """problems: sequence of dicts(x0 (13,), x_ref (N,13), foot (N,12), contact (N,4)) with per-QP N.
        Returns a list of dicts(u (N,12), x (N+1,13), status, iters) in the input order."""
        Nq = [int(np.asarray(pr["x_ref"]).shape[0]) for pr in problems]
        for N in Nq:
            if N not in self.horizons:
                raise ValueError(f"no engine for horizon {N} (have {sorted(self.horizons)})")
        if any("pcom" in pr for pr in problems):
            raise ValueError("the ragged path takes the CoM horizon from x_ref (no separate pcom)")
        res = self.solve_packed(Nq, np.stack([pr["x0"] for pr in problems]), np.concatenate([pr["x_ref"] for pr in problems]),
                                np.concatenate([pr["foot"] for pr in problems]), np.concatenate([pr["contact"] for pr in problems]))
        off = res["off"]
        return [dict(u=res["u"][off[i]:off[i + 1]], x=res["x"][off[i] + i:off[i + 1] + i + 1], status=int(res["status"][i]),
                     iters=int(res["iters"][i])) for i in range(len(problems))]


class MPC:
    """Drop-in for ``srbd_mpc.mpc.MPC`` on the hot path (run_simulation.py:169-170,73-82,96,103,106)."""

    def __init__(self, dt: float = 0.04, horizon: int = 10, device: int = 0, strict: bool = True, rank_aware: bool = False, staged_wrench: bool = False,
                 staged_normals: bool = False, **overrides):
        """staged_normals=True: update(..., contact_normals=n) stays on the staged batch-1 path -- one srbdqp_update_normals_f64 call over the staging arrays, on
        the general kernel's low-latency contact-normals instantiation at N <= 10 -- instead of the host-batch route (the default, False: that route, exactly).
        For the robot on sloped ground whose foothold normals change at every control step.
        staged_wrench=True: update(..., external_wrench=w) stays on the staged batch-1 path -- one srbdqp_update_wrench_f64 call over the staging arrays, on
        the general kernel's low-latency external-wrench instantiation at N <= 10 -- instead of the host-batch route with its two setter calls (the default,
        False: that route, exactly).  For the robot whose wrench estimate changes at every control step.
        rank_aware=True: the engine is created with SRBDQP_FLAG_RANK_AWARE (BatchMPC) -- a horizon with feet in tandem or point feet on every step gets an
        answer from update() (the general kernel's batch instantiation through the HIP launch, at its latency) instead of status -1.
        Every solve starts from zero.  (Rounds 1-4 had `warm_start=True`: the previous plan and duals shifted by one step.  Removed in round 5 -- on this
        ADMM (sigma -> 0, alpha = 1.6) an error of the starting point decays by |1 - alpha| = 0.6 per iteration whatever else happens, and the dual residual
        sees it through P: the shifted plan is 0.2 |x*| from the new optimum but ~400 |q| from it through P (zero: 1 |q|), i.e. log(400) / log(1 / 0.6) = 12
        iterations WORSE than zero: 41 against 30 on closed loops, profiles/r05_warm_start_sweep.txt, DESIGN.md section 2.  The C-ABI keeps warm_u / warm_y.)
        strict=True (default): a solve that ends with a negative status (SRBDQP_NUMERICAL, SRBDQP_CONTACT_BOUND: the kernel
        returned all-zero forces) raises SrbdqpError instead of handing zeros to the WBID step; a solve that stops at the
        iteration cap (SRBDQP_MAX_ITER) returns its best iterate with a RuntimeWarning.  strict=False returns whatever came
        back; ``status`` / ``iters`` / ``solve_time`` always hold the outcome of the last call."""
        self.dt = float(dt)
        self.HORIZON_LENGTH = int(horizon)
        self.g = -9.80665                       # ros_run_simulation.py:58
        self.x0 = np.zeros((NX, 1))
        self.x0[12] = self.g
        self.x_ref_hor = np.zeros((self.HORIZON_LENGTH, NX))
        self.x_ref_hor[:, 12] = self.g
        if "warm_start" in overrides:
            raise TypeError("MPC(warm_start=...) was removed in round 5: a shift-based start costs this ADMM 10 iterations instead of saving any "
                            "(profiles/r05_warm_start_sweep.txt); BatchMPC.solve(warm_u=, warm_y=) remains for callers with a better start")
        self.strict = bool(strict)
        self._solve_time = 0.0                  # seconds spent in the last solve (the node's solve-time statistic)
        self._fcb = None                        # the CPython binding of srbdqp_update_f64 (csrc/fastcall.c), once bound
        self._device = device
        self._overrides = dict(overrides, rank_aware=True) if rank_aware else overrides
        self._engine: Optional[BatchMPC] = None
        self._u_opt = None
        self._x_opt = None
        self._status = 0
        self._iters = 0
        self._last_fc = False                   # ... through the CPython binding (solve_time is read from it)
        self._last_fast = False                 # the last call went through update()'s bound fast path: results are read from the staging arrays
        self._upd = None                        # srbdqp_update_f64 with every argument bound (see _bind)
        self.staged_wrench = bool(staged_wrench)
        self.staged_normals = bool(staged_normals)
        self._side_calls = {}                   # kind -> (srbdqp_update_wrench_f64 / _normals_f64, its arguments with pcom, without, row 0 of the staged array, its width): see _update_staged_side

    # outcome of the last call.  The fast path of update() leaves everything in the library's staging arrays and these read it there on demand.
    @property
    def solve_time(self) -> float:
        """seconds inside the library during the last call"""
        return _fastcall.solve_time(self._fcb) if (self._last_fc and self._fcb is not None) else self._solve_time

    @property
    def status(self) -> int:
        return int(self._s_status[0]) if self._last_fast else self._status

    @property
    def iters(self) -> int:
        return int(self._s_iters[0]) if self._last_fast else self._iters

    @property
    def u_opt(self):
        """(N, 12) last optimal forces [N]"""
        return self._s_u.copy() if self._last_fast else self._u_opt

    @property
    def x_opt(self):
        """(N+1, 13) last roll-out"""
        return self._s_x.copy() if self._last_fast else self._x_opt

    def init_matrices(self):
        """Allocate the engine (stream + device workspace).  run_simulation.py:170."""
        if self._engine is None:
            self._engine = BatchMPC(horizon=self.HORIZON_LENGTH, dt=self.dt, device=self._device, **self._overrides)
        return self

    def _bind(self):
        """Bind srbdqp_update_f64 once: NumPy views of the staging arrays for this robot's QP and the eleven arguments of the call as
        ctypes objects (inputs and outputs ARE the staging arrays, so the C side copies nothing).  A call is then
        ``self._upd(*self._args)``: no boxing, no argument conversion."""
        if self._engine is None:
            self.init_matrices()
        eng = self._engine
        st = eng.stage()
        self._s_x0, self._s_xref, self._s_pcom = st["x0"][0], st["x_ref"][0], st["pcom"][0]
        self._s_x0c = st["x0"][0].reshape(NX, 1)        # the reference passes MPC.x0, a (13, 1) column (run_simulation.py:73-77,106): same-shape assignment is the cheapest copy
        self._s_foot2, self._s_ct2 = st["foot"][0], st["contact"][0]
        self._s_foot, self._s_ct = st["foot"][0].reshape(-1), st["contact"][0].reshape(-1)
        self._s_u, self._s_x = st["u"][0], st["x"][0]
        self._s_u0, self._s_x01 = st["u"][0][0].reshape(NU, 1), st["x"][0][:2]
        self._s_status, self._s_iters = st["status"], st["iters"]
        P = lambda a: C.c_void_p(a.ctypes.data)
        h = C.c_void_p(eng._h.value)
        ins = (h, P(self._s_x0), P(self._s_xref), P(self._s_foot), P(self._s_ct))
        outs = (P(self._s_u), None, P(self._s_x), None, None)         # u0_out = the staging u (in place), no second plan copy, x in place
        self._args_pcom = ins + (P(self._s_pcom),) + outs
        self._args_nopcom = ins + (None,) + outs
        self._upd = _lib.load_raw().srbdqp_update_f64
        self._fcb = getattr(eng, "_fcb", None)
        return self._upd

    def _write_staged(self, x0, x_ref_hor, c_horizon, contact_horizon, p_com_horizon):
        """One QP into row 0 of the engine's staging arrays (no hipMemcpy on this path) -> (the arrays, whether pcom was written)."""
        N = self.HORIZON_LENGTH
        st = self._engine.stage()
        st["x0"][0] = np.asarray(x0, dtype=np.float64).reshape(NX)
        st["x_ref"][0] = np.asarray(x_ref_hor, dtype=np.float64).reshape(N, NX)
        # the reference passes per-step lists (run_simulation.py:94-101): concatenating straight into the staging
        # arrays is ~1 us cheaper than np.asarray(list) + copy; anything irregular takes the general path
        try:
            np.concatenate(c_horizon, out=st["foot"][0].reshape(-1))
            np.concatenate(contact_horizon, out=st["contact"][0].reshape(-1), casting="unsafe")   # 0 / non-zero flags
        except (ValueError, TypeError):
            st["foot"][0] = np.asarray(c_horizon, dtype=np.float64).reshape(N, NU)
            st["contact"][0] = np.asarray(contact_horizon).reshape(N, NC) != 0
        if p_com_horizon is not None:
            st["pcom"][0] = np.asarray(p_com_horizon, dtype=np.float64).reshape(N, 3)
        return st, p_com_horizon is not None

    def _outcome(self, status, iters, u, x, one_rollout, stacklevel):
        """The outcome of every call but update()'s bound fast path: status and iters kept, a solve that is not SOLVED raised or warned about (stacklevel as
        warnings.warn counts it from the method that calls this one: 2 = that method's caller), the plan u (N,12) and roll-out x (N+1,13) kept as u_opt /
        x_opt.  Returns what update() returns."""
        self._status, self._iters = int(status), int(iters)
        if self._status != _lib.SOLVED:
            self._not_solved(self._status, self._iters, stacklevel + 2)
        self._u_opt, self._x_opt = u, x
        return u[0].reshape(NU, 1).copy(), (x.copy() if one_rollout else x[:2].copy())

    def _solve(self, x_current, x_ref_hor, c_horizon, contact_horizon, p_com_horizon, one_rollout, stacklevel):
        """One QP through the staging arrays and srbdqp_solve_staged_f64: the body of solve() and of update()'s general path."""
        if self._engine is None:
            self.init_matrices()
        self._last_fast = self._last_fc = False
        st, use_pcom = self._write_staged(x_current, x_ref_hor, c_horizon, contact_horizon, p_com_horizon)
        t0 = time.perf_counter()
        self._engine.solve_staged(1, use_pcom=use_pcom, use_warm=False, want_x=True, want_y=False)
        self._solve_time = time.perf_counter() - t0
        return self._outcome(st["status"][0], st["iters"][0], st["u"][0].copy(), st["x"][0].copy(), one_rollout, stacklevel + 1)

    def solve(self, x_current, x_ref_hor, c_horizon, contact_horizon, p_com_horizon=None):
        """Assemble + solve one QP on the GPU; returns (u (N,12) newtons, x (N+1,13)).
        Inputs are written straight into the library's pinned staging arrays (no hipMemcpy on this path)."""
        self._solve(x_current, x_ref_hor, c_horizon, contact_horizon, p_com_horizon, True, 2)
        return self._u_opt, self._x_opt

    def _not_solved(self, status, iters, stacklevel):
        """strict mode: a failed solve raises, a stop at the iteration cap warns (the reference's consumer has no status handling,
        ros_run_simulation.py:188-218: without this a zero-force plan would go straight to the WBID step)"""
        if not self.strict:
            return
        if status < 0:
            raise SrbdqpError(f"MPC solve failed with status {status} "
                              f"({'non-finite inputs or a singular contact geometry' if status == _lib.NUMERICAL else 'more stance contacts in a step than max_contacts_per_step'}); "
                              "the kernel returned zero forces")
        if status == _lib.MAX_ITER:
            warnings.warn(f"MPC solve stopped at the iteration cap ({iters} iterations): best iterate returned", RuntimeWarning, stacklevel=stacklevel)

    def prepare(self, contact_horizon: Sequence, c_horizon: Sequence, p_com_horizon=None, x_predicted=None):
        """Two-phase form of update() for loops that know the contact schedule, the contact points and x_ref_hor before the state
        estimate arrives (NOT the reference's call pattern, which measures the feet with the state: run_simulation.py:94-97):
        the factorisation runs now, asynchronously; update_prepared(x_current) then only patches the gradient and iterates.
        x_predicted: any finite guess of the state (default: self.x0)."""
        if self._engine is None:
            self.init_matrices()
        _, use_pcom = self._write_staged(self.x0 if x_predicted is None else x_predicted, self.x_ref_hor, c_horizon, contact_horizon, p_com_horizon)
        self._engine.prepare_staged(1, use_pcom=use_pcom)

    def update_prepared(self, x_current=None, one_rollout: bool = True):
        """Second phase of prepare(): returns what update() returns, for the measured state x_current (default: self.x0)."""
        eng = self._engine
        st = eng.stage()
        self._last_fast = self._last_fc = False
        st["x0"][0] = np.asarray(self.x0 if x_current is None else x_current, dtype=np.float64).reshape(NX)
        t0 = time.perf_counter()
        eng.solve_prepared(1, want_x=True)
        self._solve_time = time.perf_counter() - t0
        return self._outcome(st["status"][0], st["iters"][0], st["u"][0].copy(), st["x"][0].copy(), one_rollout, 2)

    def update(self, contact_horizon: Sequence, c_horizon: Sequence, p_com_horizon, x_current=None,
               one_rollout: bool = True, contact_normals=None, external_wrench=None):
        """run_simulation.py:106.  Returns (u_opt0 (12,1), x_opt1) where x_opt1[1] is the next state.
        one_rollout=True -> x_opt1 has the whole roll-out (N+1, 13); False -> only rows 0..1.
        contact_normals: (N, 12) / (N, 4, 3) array or a per-step list of world-frame surface normals (BatchMPC.set_contact_normals): the friction pyramids
        of sloped ground.  Such a call goes through the host-batch solve with B = 1 -- or, on an object made with staged_normals=True, through the staged call
        srbdqp_update_normals_f64 (_update_staged_side).
        external_wrench: (N, 6) world-frame [torque, force] on the body per horizon step (BatchMPC.set_external_wrench), for this call alone; it goes the
        same way, through the host setter (set before the solve, cleared after it: two waits for the handle's streams per call) -- or, on an object made with
        staged_wrench=True, through the staged call srbdqp_update_wrench_f64 (_update_staged_side).  Both together raise ValueError: no instantiation reads both.

        One C call (srbdqp_update_f64) with every argument bound once: the inputs go straight into the library's pinned staging arrays,
        the results are copied out of them once.  What Python adds to the C call is what NumPy needs to gather the reference's per-step
        lists (two np.concatenate of N small arrays: ~2.4 us of ~4.5 us in total); (N, 12) / (N, 4) arrays instead of lists cost
        ~2 us less."""
        if contact_normals is not None and external_wrench is not None:
            raise ValueError("update: contact_normals and external_wrench together are not supported (no instantiation of the general kernel reads both)")
        if external_wrench is not None and self.staged_wrench:
            return self._update_staged_side("wrench", contact_horizon, c_horizon, p_com_horizon, x_current, one_rollout, external_wrench)
        if contact_normals is not None and self.staged_normals:
            return self._update_staged_side("normals", contact_horizon, c_horizon, p_com_horizon, x_current, one_rollout, contact_normals)
        if contact_normals is not None or external_wrench is not None:
            return self._update_via_batch(contact_horizon, c_horizon, p_com_horizon, x_current, one_rollout, contact_normals, external_wrench)
        # From here to the end of the method: the measured ~4.5 us of Python around srbdqp_update_f64.  Its two arms keep their own copy of "write one QP" and of
        # "take the outcome" on purpose (results stay in the staging arrays, nothing is boxed): _write_staged and _outcome serve every other call, not this one.
        upd = self._upd
        if upd is None:
            upd = self._bind()
        fcb = self._fcb
        if fcb is not None:                        # csrc/fastcall.c: the lists walked with the C API, straight into the staging arrays, results as fresh arrays
            r = _fastcall.update(fcb, contact_horizon, c_horizon, p_com_horizon, self.x0 if x_current is None else x_current, self.x_ref_hor, one_rollout)
            if r is not NotImplemented:            # (anything it does not recognise -- other dtypes, shapes, nested lists -- takes the NumPy path below)
                u0, x1, st, rc = r
                self._last_fast = self._last_fc = True
                if rc:
                    _lib.check(rc, self._engine._h)
                if st != 1:                        # (_lib.SOLVED)
                    self._not_solved(st, int(self._s_iters[0]), 3)
                return u0, x1
        self._last_fc = False
        try:
            x_cur = self.x0 if x_current is None else x_current
            try:
                self._s_x0c[...] = x_cur
            except ValueError:                     # not a (13, 1) column: (13,) and the like
                self._s_x0[:] = x_cur.reshape(NX)
            self._s_xref[:] = self.x_ref_hor
            if type(c_horizon) is np.ndarray:
                self._s_foot2[:] = c_horizon
            else:                                  # the reference passes per-step lists (run_simulation.py:94-101)
                np.concatenate(c_horizon, out=self._s_foot)
            if type(contact_horizon) is np.ndarray:
                self._s_ct2[:] = contact_horizon
            else:
                np.concatenate(contact_horizon, out=self._s_ct, casting="unsafe")   # 0 / non-zero flags
            if p_com_horizon is None:
                args = self._args_nopcom
            else:
                self._s_pcom[:] = p_com_horizon
                args = self._args_pcom
        except (ValueError, TypeError, AttributeError):   # anything irregular (nested lists, other shapes): the general path
            return self._update_general(contact_horizon, c_horizon, p_com_horizon, x_current, one_rollout)
        t0 = time.perf_counter()
        rc = upd(*args)
        self._solve_time = time.perf_counter() - t0
        self._last_fast = True
        if rc:
            _lib.check(rc, self._engine._h)
        if self._s_status[0] != 1:                 # (_lib.SOLVED)
            self._not_solved(int(self._s_status[0]), int(self._s_iters[0]), 3)
        return self._s_u0.copy(), (self._s_x.copy() if one_rollout else self._s_x01.copy())

    def _update_general(self, contact_horizon, c_horizon, p_com_horizon, x_current, one_rollout):
        return self._solve(self.x0 if x_current is None else x_current, self.x_ref_hor, c_horizon, contact_horizon, p_com_horizon, one_rollout, 3)

    def _update_via_batch(self, contact_horizon, c_horizon, p_com_horizon, x_current, one_rollout, contact_normals=None, external_wrench=None):
        """update() with contact normals or an external wrench (at most one of them): the host-batch solve with B = 1.  The wrench is set through the host
        setter before the solve and cleared after it, and each of the two calls waits for every stream of the handle first: fine for one QP per control
        step, and a fleet sets its wrenches once per solve on a BatchMPC instead."""
        if self._engine is None:
            self.init_matrices()
        eng, N = self._engine, self.HORIZON_LENGTH
        self._last_fast = self._last_fc = False
        x_cur = np.asarray(self.x0 if x_current is None else x_current, dtype=np.float64).reshape(1, NX)
        pc = None if p_com_horizon is None else np.asarray(p_com_horizon, dtype=np.float64).reshape(1, N, 3)
        nr = None if contact_normals is None else np.asarray(contact_normals, dtype=np.float64).reshape(1, N, NU)
        t0 = time.perf_counter()
        if external_wrench is not None:            # for this call alone: cleared again below, whatever the solve does
            eng.set_external_wrench(np.asarray(external_wrench, dtype=np.float64).reshape(1, N, 6))
        try:
            out = eng.solve(x_cur, np.asarray(self.x_ref_hor, dtype=np.float64).reshape(1, N, NX), np.asarray(c_horizon, dtype=np.float64).reshape(1, N, NU),
                            np.asarray(contact_horizon).reshape(1, N, NC), pcom=pc, normals=nr)
        finally:
            if external_wrench is not None:
                eng.set_external_wrench(None)
        self._solve_time = time.perf_counter() - t0
        return self._outcome(out["status"][0], out["iters"][0], out["u"][0], out["x"][0], one_rollout, 3)

    def _update_staged_side(self, kind, contact_horizon, c_horizon, p_com_horizon, x_current, one_rollout, side):
        """update() with an external wrench on a staged_wrench=True object (kind "wrench"), or with contact normals on a staged_normals=True one ("normals"):
        the QP and its side input into row 0 of the staging arrays, then ONE C call (srbdqp_update_wrench_f64 / srbdqp_update_normals_f64) whose arguments were
        bound once (BatchMPC.bind_update_wrench / bind_update_normals).  The side input is the call's: the next update() without one is the plain staged call,
        unchanged."""
        if self._engine is None:
            self.init_matrices()
        eng, N = self._engine, self.HORIZON_LENGTH
        rec = self._side_calls.get(kind)
        if rec is None:
            bind, view = {"wrench": ("bind_update_wrench", "stage_ext_wrench"), "normals": ("bind_update_normals", "stage_contact_normals")}[kind]
            row = getattr(eng, view)()[0]
            rec = self._side_calls[kind] = getattr(eng, bind)() + (row, row.shape[1])
        upd, args_pcom, args_nopcom, row, width = rec
        self._last_fast = self._last_fc = False
        st, use_pcom = self._write_staged(self.x0 if x_current is None else x_current, self.x_ref_hor, c_horizon, contact_horizon, p_com_horizon)
        row[:] = np.asarray(side, dtype=np.float64).reshape(N, width)     # (two integers: a shape tuple costs reshape 0.1 us more)
        t0 = time.perf_counter()
        rc = upd(*(args_pcom if use_pcom else args_nopcom))
        self._solve_time = time.perf_counter() - t0
        if rc:
            _lib.check(rc, eng._h)
        return self._outcome(st["status"][0], st["iters"][0], st["u"][0].copy(), st["x"][0].copy(), one_rollout, 3)

    def close(self):
        self._upd = self._fcb = None
        self._side_calls = {}                   # (bound calls on, and views of, the staged side arrays)
        self._last_fast = self._last_fc = False
        for k in [k for k in vars(self) if k.startswith(("_s_", "_args_"))]:    # what _bind() made: views of, and addresses in, memory the library is about to free
            delattr(self, k)
        if self._engine is not None:
            self._engine.close()
            self._engine = None
