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
