// bc7_image_regions_kernels.hip -- several RGBA8888 images of one BC7 buffer in one call on gfx950 (include/dxtlt_bc7_image.h;
// docs/IMAGE_DECODE.md, "Several images of one BC7 buffer"): the region kernels and launchers of granule_image.h for Bc7Image.
// A translation unit of its own, beside bc7_image_kernels.hip, on purpose: with the full-granule kernels of one image and of a region
// table in ONE module the compiler emits another instruction stream for both (the same 95 / 96 VGPRs, 37 instructions fewer in
// 20 000), and the sinks' measured notes (bc7_image_sinks.h) are about the streams these two files give.  BC6H's kernels come out
// the same either way and share bc6h_image_kernels.hip.
#include "bc7_image_sinks.h"
#include "granule_image.h"

namespace dxtlt {

template hipError_t launch_decode_image_regions<bc7::Bc7Image>(const void*, uint64_t, const ImageRegionTable&, hipStream_t);
template hipError_t launch_untransform_decode_image_regions<bc7::Bc7Image>(const void*, uint64_t, const ImageRegionTable&, hipStream_t);

}  // namespace dxtlt
