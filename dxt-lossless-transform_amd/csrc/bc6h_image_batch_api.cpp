// bc6h_image_batch_api.cpp -- dxtlt_untransform_decode_bc6h_images_batch_device and its planning hook (include/dxtlt_bc6h_image.h;
// docs/IMAGE_DECODE.md, "Many BC6H buffers in one call"): BC6H as a family of granule_image_batch_api.h, which has the bodies -- the
// checks, the plan, the staging of the tables -- and the two forwards.  The kernels are bc6h_image_batch_kernels.hip's.
#include "../../include/dxtlt_bc6h_image.h"
#include "../../include/dxtlt_gfx950.h"
#include "bc6h_image_batch_launch.h"
#include "granule_image_batch_api.h"

namespace {

namespace api = dxtlt_host::granule_image_batch;

struct Bc6h {
    static constexpr dxtlt_host::PixelRule rule = dxtlt_host::kRgba16f;
    static constexpr const char* kName = "bc6h";
    using Item = DxtltBc6hImageBatchItem;
    using DebugEntry = DxtltDebugBc6hImageBatchEntry;
    static constexpr auto& launch = dxtlt::bc6h::launch_image_batch;
};

}  // namespace

extern "C" int32_t dxtlt_untransform_decode_bc6h_images_batch_device(const DxtltBc6hImageBatchItem* items, size_t count, void* hip_stream)
{
    return api::untransform_decode_images_batch_device<Bc6h>(items, count, hip_stream);
}

extern "C" int32_t dxtlt_debug_plan_bc6h_image_batch(const DxtltBc6hImageBatchItem* items, size_t count, DxtltDebugBc6hImageBatchEntry* out,
                                                     size_t cap)
{
    return api::debug_plan<Bc6h>(items, count, out, cap);
}
