"""What the GPU suites of the per-QP side inputs share (test_gpu_robots.py, test_gpu_weights.py, test_gpu_contact_normals.py, test_gpu_variant_refusals.py):
device copies of a batch, a device-buffer solve into fresh outputs, and the message of a refused call."""
import numpy as np


def to_dev(torch, x0, xr, ft, ct):
    return dict(x0=torch.from_numpy(x0).cuda(), xr=torch.from_numpy(xr).cuda(), ft=torch.from_numpy(ft).cuda(), ct=torch.from_numpy(ct.astype(np.uint8)).cuda())


def device_solve(torch, eng, t, B, stream=None):
    """solve_device of the B QPs in t = to_dev(...) on `stream` (torch's current one by default); -> dict(u, x, status, iters) of device tensors.  Does not synchronise."""
    o = dict(u=torch.empty((B, eng.N, 12), dtype=torch.float64, device="cuda"), x=torch.empty((B, eng.N + 1, 13), dtype=torch.float64, device="cuda"),
             status=torch.empty(B, dtype=torch.int32, device="cuda"), iters=torch.empty(B, dtype=torch.int32, device="cuda"))
    eng.solve_device(B, t["x0"].data_ptr(), t["xr"].data_ptr(), t["ft"].data_ptr(), t["ct"].data_ptr(), o["u"].data_ptr(), o["x"].data_ptr(),
                     status=o["status"].data_ptr(), iters=o["iters"].data_ptr(), stream=stream or torch.cuda.current_stream().cuda_stream)
    return o


def refusal(fn):
    """The message of the SrbdqpError that fn() raises, or None when it returns."""
    from g1_locomotion_amd import SrbdqpError
    try:
        fn()
    except SrbdqpError as e:
        return str(e)
    return None
