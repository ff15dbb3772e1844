// granule_launch.cpp -- the one place that picks a granule format's kernels (granule_launch.h): 7 = BC7
// (bc7_kernels.hip), 6 = BC6H (bc6h_kernels.hip).
#include "granule_launch.h"

#include <cstdio>

namespace dxtlt {
namespace granule {

const char* format_name(int format) { return format == 6 ? "BC6H" : "BC7"; }
const char* format_symbol(int format) { return format == 6 ? "bc6h" : "bc7"; }

const char* named(int format, const char* before, const char* after)
{
    thread_local char text[160];
    std::snprintf(text, sizeof text, "%s%s%s", before, format_name(format), after);
    return text;
}

hipError_t launch_range(int format, bool inverse, const void* src, void* dst, uint64_t total_blocks, uint64_t first_block,
                        uint64_t num_blocks, hipStream_t stream)
{
    return format == 6 ? bc6h::launch_range(inverse, src, dst, total_blocks, first_block, num_blocks, stream)
                       : bc7::launch_range(inverse, src, dst, total_blocks, first_block, num_blocks, stream);
}

hipError_t launch(int format, bool inverse, const void* src, void* dst, uint64_t n_blocks, hipStream_t stream)
{
    return launch_range(format, inverse, src, dst, n_blocks, 0, n_blocks, stream);
}

hipError_t launch_batch(int format, bool inverse, const BatchEntry* d_entries, const uint32_t* d_coarse, uint32_t n_entries,
                        uint32_t granule_wgs, const BatchEntry* d_tails, uint32_t n_tails, hipStream_t stream)
{
    return format == 6 ? bc6h::launch_batch(inverse, d_entries, d_coarse, n_entries, granule_wgs, d_tails, n_tails, stream)
                       : bc7::launch_batch(inverse, d_entries, d_coarse, n_entries, granule_wgs, d_tails, n_tails, stream);
}

}  // namespace granule
}  // namespace dxtlt
