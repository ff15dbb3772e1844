// Host build of csrc/launch_grid.h for tests/test_launch_grid.py: the grid that grid_rows() gives for a lane count.  Built by
// g++ against the real <hip/hip_runtime.h> (-D__HIP_PLATFORM_AMD__): dim3 and hipError_t are HIP's own; nothing is launched and
// no HIP library is linked.
#include <cstdint>

#include "../../dxt-lossless-transform_amd/csrc/launch_grid.h"

extern "C" {

// 0 and (x, y, z) in out, or 1 when grid_rows refuses the count
int shim_grid_rows(uint64_t lanes, unsigned threads, uint32_t out[3])
{
    dim3 grid(0xDEADu, 0xDEADu, 0xDEADu);
    if (dxtlt::grid_rows(lanes, threads, grid) != hipSuccess)
        return 1;
    out[0] = grid.x, out[1] = grid.y, out[2] = grid.z;
    return 0;
}

uint64_t shim_grid_row() { return dxtlt::kGridRow; }

}  // extern "C"
