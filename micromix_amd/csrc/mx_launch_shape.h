// What a launch needs beside the kernel and its arguments: the grid, the workgroup, the dynamic LDS and the limit to raise the kernel's
// to (0: leave it).  Plain C++ without a HIP include: the host-only plan headers (mx_stream_plan.h, mx_quant_plan.h) fill one in, and
// launch_kernel (mx_kernels.h) takes it.
#pragma once

namespace mm {
struct LaunchShape { int grid_x, grid_y, threads, lds_bytes, raise_to; };
}  // namespace mm
