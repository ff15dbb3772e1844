// bc7_image_batch_api.cpp -- dxtlt_untransform_decode_bc7_images_batch_device and its planning hook (include/dxtlt_bc7_image.h;
// docs/IMAGE_DECODE.md, "Many BC7 buffers in one call"): BC7 as a family of granule_image_batch_api.h, which has the bodies -- the
// checks, the plan, the staging of the tables -- and the two forwards.  The kernels are bc7_image_batch_kernels.hip's.
#include "../../include/dxtlt_bc7_image.h"
#include "../../include/dxtlt_gfx950.h"
#include "bc7_image_batch_launch.h"
#include "granule_image_batch_api.h"

namespace {

namespace api = dxtlt_host::granule_image_batch;

struct Bc7 {
    static constexpr dxtlt_host::PixelRule rule = dxtlt_host::kRgba8888;
    static constexpr const char* kName = "bc7";
    using Item = DxtltBc7ImageBatchItem;
    using DebugEntry = DxtltDebugBc7ImageBatchEntry;
    static constexpr auto& launch = dxtlt::bc7::launch_image_batch;
};

}  // namespace

extern "C" int32_t dxtlt_untransform_decode_bc7_images_batch_device(const DxtltBc7ImageBatchItem* items, size_t count, void* hip_stream)
{
    return api::untransform_decode_images_batch_device<Bc7>(items, count, hip_stream);
}

extern "C" int32_t dxtlt_debug_plan_bc7_image_batch(const DxtltBc7ImageBatchItem* items, size_t count, DxtltDebugBc7ImageBatchEntry* out,
                                                    size_t cap)
{
    return api::debug_plan<Bc7>(items, count, out, cap);
}
