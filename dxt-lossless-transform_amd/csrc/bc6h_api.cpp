// bc6h_api.cpp -- C ABI of the BC6H granule-sorted field split, layout version 1 (include/dxtlt_bc6h.h,
// docs/BC6H_FORMAT.md).  The host, device, range and sharded paths are the granule formats' (granule_host.cpp) with format
// code 6, which selects the BC6H kernels (granule_launch.h, bc6h_kernels.hip).
#include "../../include/dxtlt_bc6h.h"

#include "host_common.h"

namespace {
constexpr int kFormat = 6;
}

extern "C" {

int32_t dxtlt_transform_bc6h(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len)
{
    return dxtlt_host::granule_host_call(kFormat, false, input_ptr, output_ptr, len);
}
int32_t dxtlt_untransform_bc6h(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len)
{
    return dxtlt_host::granule_host_call(kFormat, true, input_ptr, output_ptr, len);
}
int32_t dxtlt_transform_bc6h_device(const void* d_input, void* d_output, size_t len, void* hip_stream)
{
    return dxtlt_host::granule_device_call(kFormat, false, d_input, d_output, len, hip_stream);
}
int32_t dxtlt_untransform_bc6h_device(const void* d_input, void* d_output, size_t len, void* hip_stream)
{
    return dxtlt_host::granule_device_call(kFormat, true, d_input, d_output, len, hip_stream);
}
int32_t dxtlt_transform_bc6h_range_device(bool inverse, const void* d_src, void* d_dst, uint64_t total_blocks,
                                          uint64_t first_block, uint64_t num_blocks, void* hip_stream)
{
    if (first_block > total_blocks || num_blocks > total_blocks - first_block)
        return dxtlt_host::fail(dxtlt_host::kInvalidArgument, "block range exceeds total_blocks");
    return dxtlt_host::granule_device_range(kFormat, inverse, d_src, d_dst, total_blocks, first_block, num_blocks, hip_stream);
}
uint32_t dxtlt_bc6h_sort_granule(void) { return 1024; }
int32_t dxtlt_transform_bc6h_sharded(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len, int32_t num_shards)
{
    return dxtlt_host::granule_sharded(kFormat, false, input_ptr, output_ptr, len, num_shards);
}
int32_t dxtlt_untransform_bc6h_sharded(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len, int32_t num_shards)
{
    return dxtlt_host::granule_sharded(kFormat, true, input_ptr, output_ptr, len, num_shards);
}
int32_t dxtlt_bc6h_shard_pieces(uint64_t total_blocks, uint64_t first_block, uint64_t num_blocks, uint64_t* global_off,
                                uint64_t* local_off, uint64_t* bytes)
{
    return dxtlt_host::granule_shard_pieces(kFormat, total_blocks, first_block, num_blocks, global_off, local_off, bytes);
}

}  // extern "C"
