// srbdqp_wrench_lat_ew.hpp -- the doors to the low-latency side-input kernels of the general kernel (srbdqp_wrench.hpp: MODE 7, srbdqp_wrench_ew_lat_kernel[_in],
// and MODE 4, srbdqp_wrench_cn_lat_kernel[_in]), which live in a translation unit of their own, srbdqp_wrench_lat_ew.hip.
//
// Why a second translation unit: every translation unit has its own gfx950 code object in the library's fat binary.  srbdqp.hip's holds the batch-1 kernels of
// the plain staged call, whose loop is known to care where it lies (profiles/r05_loop_alignment.txt).  With these twelve kernels here, srbdqp.hip's code object
// is what it was without them -- every kernel at its old address, the same text: the plain call cannot have changed on the device.
// srbdqp.hip comes FIRST on the compiler's command line: the library's own AQL loader (srbdqp_aql.hpp) and tests/test_aql_contract_cpu.py read the first bundle.
#pragma once
#include <hip/hip_runtime.h>
#include "srbdqp_common.hpp"

namespace srbdqp {

// One launch through HIP on st of the low-latency kernel of mode (kModeExtWrench: 6 N doubles a QP; kModeNormals: 12 N), N in {4, 8, 10} (anything else:
// hipErrorInvalidValue).
//   in == nullptr: the grid of a.B workgroups, QP b under block b of side_dev (a device address);
//   in != nullptr: ONE workgroup with *in = the StagedIn<N> of the QP and the doubles of its block at side_host behind it in the kernel-argument segment
//                  (a.inline_in set).
// set_attr: raise the kernel's dynamic-LDS limit first (once per kernel and device: the caller keeps the book, as it does for its own kernels).
hipError_t launch_wrench_side_lat(int mode, int N, bool set_attr, const KArgs& a, const void* in, const double* side_host, const double* side_dev, hipStream_t st);

}  // namespace srbdqp
