"""What the GPU suites share: the torch_first fixture (imported by name), device copies of a batch, a device-buffer solve into fresh outputs -- batch and
ragged --, and the message of a refused call."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def torch_first():
    import torch  # load torch's HIP runtime before libsrbdqp.so so both share one
    assert torch.cuda.is_available()
    return torch


def to_dev(torch, x0, xr, ft, ct):
    return dict(x0=torch.from_numpy(x0).cuda(), xr=torch.from_numpy(xr).cuda(), ft=torch.from_numpy(ft).cuda(), ct=torch.from_numpy(ct.astype(np.uint8)).cuda())


def device_solve(torch, eng, t, B, stream=None):
    """solve_device of the B QPs in t = to_dev(...) on `stream` (torch's current one by default); -> dict(u, x, status, iters) of device tensors.  Does not synchronise."""
    o = dict(u=torch.empty((B, eng.N, 12), dtype=torch.float64, device="cuda"), x=torch.empty((B, eng.N + 1, 13), dtype=torch.float64, device="cuda"),
             status=torch.empty(B, dtype=torch.int32, device="cuda"), iters=torch.empty(B, dtype=torch.int32, device="cuda"))
    eng.solve_device(B, t["x0"].data_ptr(), t["xr"].data_ptr(), t["ft"].data_ptr(), t["ct"].data_ptr(), o["u"].data_ptr(), o["x"].data_ptr(),
                     status=o["status"].data_ptr(), iters=o["iters"].data_ptr(), stream=stream or torch.cuda.current_stream().cuda_stream)
    return o


def sentinel_solve(torch, eng, d, sentinel, isentinel, f32=False, pcom=None, warm_u=None, warm_y=None, flush=False, sync=True):
    """solve_device of the host batch d = dict(x0, x_ref, foot, contact) (fp32 buffers and srbdqp_solve_batch_device_f32 where f32) into device outputs
    PREFILLED with a finite sentinel -- u, x, y with `sentinel`, status and iters with `isentinel` -- so that an entry the kernel never wrote shows; pcom,
    warm_u, warm_y: host arrays or None.  The engine's flush() where asked, a synchronise unless sync=False (then the device tensors come back, with the
    inputs under "_in": a deferred pass may still read them); -> dict(u, x, y, status, iters) of host arrays."""
    fl, tfl = (np.float32, torch.float32) if f32 else (np.float64, torch.float64)
    B, N = d["x0"].shape[0], eng.N
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, fl)).cuda()
    t = dict(x0=dev(d["x0"]), xr=dev(d["x_ref"]), ft=dev(d["foot"]), ct=torch.from_numpy(np.ascontiguousarray(d["contact"], np.uint8)).cuda(),
             pc=dev(pcom), wu=dev(warm_u), wy=dev(warm_y))
    ptr = lambda v: 0 if v is None else v.data_ptr()
    o = dict(u=torch.full((B, N, 12), sentinel, dtype=tfl, device="cuda"), x=torch.full((B, N + 1, 13), sentinel, dtype=tfl, device="cuda"),
             y=torch.full((B, 20 * N), sentinel, dtype=tfl, device="cuda"), status=torch.full((B,), isentinel, dtype=torch.int32, device="cuda"),
             iters=torch.full((B,), isentinel, dtype=torch.int32, device="cuda"))
    st = torch.cuda.current_stream().cuda_stream
    eng.solve_device(B, ptr(t["x0"]), ptr(t["xr"]), ptr(t["ft"]), ptr(t["ct"]), o["u"].data_ptr(), x_out=o["x"].data_ptr(), y_out=o["y"].data_ptr(),
                     status=o["status"].data_ptr(), iters=o["iters"].data_ptr(), pcom=ptr(t["pc"]), warm_u=ptr(t["wu"]), warm_y=ptr(t["wy"]), stream=st, f32=f32)
    if flush:
        eng.flush(st)
    if not sync:
        return dict(o, _in=t)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def sentinel_ragged_solve(torch, rg, Nq, x0, xr, ft, ct, sentinel, isentinel, f32=False):
    """The ragged twin of sentinel_solve: RaggedMPC.solve_device (srbdqp_solve_ragged_device_f64, or _f32 on float32 buffers) of the packed host arrays into device
    outputs prefilled with the sentinels, and a synchronise; -> dict(u (rows, 12), x (rows + B, 13), status, iters) of host arrays."""
    fl, tfl = (np.float32, torch.float32) if f32 else (np.float64, torch.float64)
    B, rows = len(Nq), int(np.sum(Nq))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, fl)).cuda()
    t = (dev(x0), dev(xr), dev(ft), torch.from_numpy(np.ascontiguousarray(ct, np.uint8)).cuda())
    o = dict(u=torch.full((rows, 12), sentinel, dtype=tfl, device="cuda"), x=torch.full((rows + B, 13), sentinel, dtype=tfl, device="cuda"),
             status=torch.full((B,), isentinel, dtype=torch.int32, device="cuda"), iters=torch.full((B,), isentinel, dtype=torch.int32, device="cuda"))
    rg.solve_device(B, Nq, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), o["u"].data_ptr(), x_out=o["x"].data_ptr(),
                    status=o["status"].data_ptr(), iters=o["iters"].data_ptr(), stream=torch.cuda.current_stream().cuda_stream, f32=f32)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def ragged_device_solve(torch, rg, Nq, t, B, rows, flush):
    """solve_device of the B packed QPs in t = to_dev(...) on the ragged object rg (`rows` horizon rows in all), its flush() where asked, and a
    synchronise; -> dict(u (rows, 12), x (rows + B, 13), status, iters) of host arrays."""
    u = torch.empty((rows, 12), dtype=torch.float64, device="cuda"); x = torch.empty((rows + B, 13), dtype=torch.float64, device="cuda")
    st = torch.empty(B, dtype=torch.int32, device="cuda"); it = torch.empty(B, dtype=torch.int32, device="cuda")
    rg.solve_device(B, Nq, t["x0"].data_ptr(), t["xr"].data_ptr(), t["ft"].data_ptr(), t["ct"].data_ptr(), u.data_ptr(), x.data_ptr(), st.data_ptr(),
                    it.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    if flush:
        rg.flush(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(u=u.cpu().numpy(), x=x.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy())


def refusal(fn):
    """The message of the SrbdqpError that fn() raises, or None when it returns."""
    from g1_locomotion_amd import SrbdqpError
    try:
        fn()
    except SrbdqpError as e:
        return str(e)
    return None
