// bc7_api.cpp -- C ABI of the BC7 granule-sorted field split, version 2 (include/dxtlt_bc7.h, docs/BC7_FORMAT.md).
// A format of this build's own: the reference has no BC7 transform; parity unpinned.  The host, device, range and sharded
// paths are the granule formats' (granule_host.cpp) with format code 7, which selects the BC7 kernels (granule_launch.h,
// bc7_kernels.hip).
#include "../../include/dxtlt_bc7.h"

#include "bc7_fields.h"
#include "host_common.h"

namespace {
constexpr int kFormat = 7;
}

extern "C" {

int32_t dxtlt_transform_bc7(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len)
{
    return dxtlt_host::granule_host_call(kFormat, false, input_ptr, output_ptr, len);
}
int32_t dxtlt_untransform_bc7(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len)
{
    return dxtlt_host::granule_host_call(kFormat, true, input_ptr, output_ptr, len);
}
size_t dxtlt_bc7_workspace_bytes(size_t len)
{
    (void)len;
    return 0;   // since version 1: a single pass with no device scratch
}
int32_t dxtlt_transform_bc7_device(const void* d_input, void* d_output, size_t len, void* d_workspace,
                                   size_t workspace_bytes, void* hip_stream)
{
    (void)d_workspace;
    (void)workspace_bytes;
    return dxtlt_host::granule_device_call(kFormat, false, d_input, d_output, len, hip_stream);
}
int32_t dxtlt_untransform_bc7_device(const void* d_input, void* d_output, size_t len, void* d_workspace,
                                     size_t workspace_bytes, void* hip_stream)
{
    (void)d_workspace;
    (void)workspace_bytes;
    return dxtlt_host::granule_device_call(kFormat, true, d_input, d_output, len, hip_stream);
}
int32_t dxtlt_transform_bc7_range_device(bool inverse, const void* d_src, void* d_dst, uint64_t total_blocks,
                                         uint64_t first_block, uint64_t num_blocks, void* hip_stream)
{
    if (first_block > total_blocks || num_blocks > total_blocks - first_block)
        return dxtlt_host::fail(dxtlt_host::kInvalidArgument, "block range exceeds total_blocks");
    return dxtlt_host::granule_device_range(kFormat, inverse, d_src, d_dst, total_blocks, first_block, num_blocks, hip_stream);
}
uint32_t dxtlt_bc7_sort_granule(void) { return (uint32_t)dxtlt::bc7::kGranule; }
int32_t dxtlt_transform_bc7_sharded(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len, int32_t num_shards)
{
    return dxtlt_host::granule_sharded(kFormat, false, input_ptr, output_ptr, len, num_shards);
}
int32_t dxtlt_untransform_bc7_sharded(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len, int32_t num_shards)
{
    return dxtlt_host::granule_sharded(kFormat, true, input_ptr, output_ptr, len, num_shards);
}
int32_t dxtlt_bc7_shard_pieces(uint64_t total_blocks, uint64_t first_block, uint64_t num_blocks, uint64_t* global_off,
                               uint64_t* local_off, uint64_t* bytes)
{
    return dxtlt_host::granule_shard_pieces(kFormat, total_blocks, first_block, num_blocks, global_off, local_off, bytes);
}

}  // extern "C"
