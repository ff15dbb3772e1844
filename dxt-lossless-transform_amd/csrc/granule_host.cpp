// granule_host.cpp -- what the two granule formats (7 = BC7, 6 = BC6H) share above their kernels: argument checks, the
// stream layout and launch they hand to the common host paths (host_staging.cpp, host_sharded.cpp), and the one notion
// that is theirs alone -- the tail part, the `blocks % 1024` blocks that form a buffer of their own behind the main
// streams.  bc7_api.cpp and bc6h_api.cpp are the C ABI on top.
#include <hip/hip_runtime_api.h>

#include <cstdio>

#include "bc7_fields.h"
#include "granule_launch.h"
#include "host_common.h"

namespace {

using namespace dxtlt_host;
using dxtlt::granule::named;

constexpr uint64_t kT = dxtlt::bc7::kGranule;

// `len` bytes of host or device memory as blocks: the checks every whole-buffer call starts with, in this order
int32_t check_buffers(int format, const void* in, const void* out, size_t len)
{
    if (len % 16 != 0)
        return fail(kInvalidLength, named(format, "len is not a multiple of 16 (", " block size)"));
    if (len > 0 && (in == nullptr || out == nullptr))
        return fail(kInvalidArgument, "NULL buffer with len > 0");
    return kOk;
}

Launch launch_of(int format)
{
    return [format](bool inverse, const void* src, void* dst, uint64_t total, uint64_t first, uint64_t count, hipStream_t stream) {
        return granule_device_range(format, inverse, src, dst, total, first, count, stream);
    };
}

}  // namespace

dxtlt_host::StreamLayout dxtlt_host::granule_layout(int format)
{
    StreamLayout L{format, dxtlt::granule::kStreams, {}, {}, 16, kT, kT};
    for (int s = 0; s < L.n; ++s) {
        L.off[s] = dxtlt::granule::kStreamOff[s];
        L.width[s] = dxtlt::granule::kStreamWidth[s];
    }
    return L;
}

int32_t dxtlt_host::granule_host_call(int format, bool inverse, const uint8_t* in, uint8_t* out, size_t len)
{
    if (int32_t rc = check_buffers(format, in, out, len); rc != kOk || len == 0)
        return rc;   // zero blocks: nothing to do, no device needed
    const StreamLayout L = granule_layout(format);
    const Launch launch = launch_of(format);
    uint64_t blocks = len / 16;
    const uint64_t main_blocks = blocks - blocks % kT;
    // The chunked pipeline moves stream slices, so a buffer large enough for it goes in two calls: the main part, then
    // the tail part as the small buffer of its own that it is.  Smaller buffers are one call: one launch covers both parts.
    if (main_blocks != 0 && main_blocks != blocks && pipeline_pays(len)) {
        if (int32_t rc = host_round_trip(L, launch, inverse, in, out, main_blocks); rc != kOk)
            return rc;
        in += main_blocks * 16, out += main_blocks * 16, blocks -= main_blocks;
    }
    return host_round_trip(L, launch, inverse, in, out, blocks);
}

int32_t dxtlt_host::granule_device_range(int format, bool inverse, const void* d_src, void* d_dst, uint64_t total, uint64_t first,
                                         uint64_t num, void* stream)
{
    if (num == 0)
        return kOk;
    if (d_src == nullptr || d_dst == nullptr)
        return fail(kInvalidArgument, "NULL device buffer");
    const hipError_t e = dxtlt::granule::launch_range(format, inverse, d_src, d_dst, total, first, num, (hipStream_t)stream);
    if (e == hipSuccess)
        return kOk;
    if (e == hipErrorInvalidValue)
        return fail(kInvalidArgument, named(format, "", ": a range starts on a sort granule (1024 blocks) and ends on one or at the end of the array"));
    return fail(kDevice, named(format, "", " kernel launch"), e);
}

int32_t dxtlt_host::granule_device_call(int format, bool inverse, const void* d_in, void* d_out, size_t len, void* stream)
{
    if (len % 16 != 0)
        return fail(kInvalidLength, named(format, "len is not a multiple of 16 (", " block size)"));
    return granule_device_range(format, inverse, d_in, d_out, len / 16, 0, len / 16, stream);
}

int32_t dxtlt_host::granule_sharded(int format, bool inverse, const uint8_t* in, uint8_t* out, size_t len, int32_t num_shards)
{
    if (int32_t rc = check_buffers(format, in, out, len); rc != kOk || len == 0)
        return rc;
    const uint64_t total = len / 16;
    // the per-shard records belong to dxtlt_transform_sharded alone: dxtlt_sharded_last_stats keeps reporting its last call
    return run_sharded(granule_layout(format), launch_of(format), inverse, in, out, total, total % kT, num_shards, nullptr);
}

// pieces 0..7: the shard's slice of every main stream; piece 8: the tail part (last shard only, else empty)
int32_t dxtlt_host::granule_shard_pieces(int format, uint64_t total_blocks, uint64_t first_block, uint64_t num_blocks,
                                         uint64_t* global_off, uint64_t* local_off, uint64_t* bytes)
{
    if (global_off == nullptr || local_off == nullptr || bytes == nullptr) {
        char text[64];
        std::snprintf(text, sizeof text, "dxtlt_%s_shard_pieces: NULL output array", dxtlt::granule::format_symbol(format));
        return fail(kInvalidArgument, text);
    }
    const uint64_t main_total = total_blocks - total_blocks % kT;
    if (first_block % kT != 0 || first_block > total_blocks || num_blocks > total_blocks - first_block ||
        ((first_block + num_blocks) % kT != 0 && first_block + num_blocks != total_blocks))
        return fail(kInvalidArgument, named(format, "", " shard: a shard starts on a sort granule (1024 blocks) and ends on one or at the end"));
    const uint64_t end = first_block + num_blocks;
    const uint64_t in_main = first_block >= main_total ? 0 : (end > main_total ? main_total : end) - first_block;
    Slice sl[9];
    shard_slices(granule_layout(format), main_total, first_block, in_main, num_blocks - in_main, sl);
    for (int p = 0; p < 9; ++p) {
        global_off[p] = sl[p].host_off;
        local_off[p] = sl[p].dev_off;
        bytes[p] = sl[p].bytes;
    }
    return kOk;
}
