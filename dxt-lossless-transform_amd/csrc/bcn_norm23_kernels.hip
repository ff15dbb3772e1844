// bcn_norm23_kernels.hip -- the BC2 / BC3 forward tile kernels with block normalisation fused in (include/dxtlt_bc23_normalize.h,
// dxtlt_transform_bc{2,3}_with_normalize_blocks): the tile bodies of bcn_device.h instantiated with NORM == kNormFromArgument.
//
// A lane's 16-byte vector is one block; normalize_block_bc23 (bc23_normalize.h) rewrites it in registers between the load and the
// LDS scatter, so the kernels move the plain transform's 2 * len bytes.  The modes are a wave-uniform kernel argument
// (alpha_mode << 2 | color_mode, in spare bits of fwd_tiled's `flags` and of Shifts::halo_vecs), not template parameters: BC3
// has 11 non-trivial mode pairs over 16 settings combinations.  One kernel set per (format, VARIANT, SA, SC): 8 for BC2, 16 for BC3,
// each with the members bc1_norm_kernels (bcn_kernels.hip) has.  launch_transform plans and launches them as it does the plain ones.
//
// A translation unit of its own: compiled together with the plain kernels, these instantiations make the compiler order four
// instructions of one plain halo kernel differently (profiles/normalize_fused_bc23_isa.txt).
#include "bcn_device.h"

namespace dxtlt {
namespace {

template <int FMT, int VARIANT, bool SA, bool SC>
FusedNormKernels kernels()
{
    FusedNormKernels k{};
    k.tiled = fwd_tiled<FMT, VARIANT, SA, SC, default_tile_threads(FMT, false), kNormFromArgument>;
    k.halo[0] = fwd_tiled_halo<FMT, VARIANT, SA, SC, kNormFromArgument, false, halo_tile_threads(FMT, SC)>;
    k.halo[1] = fwd_tiled_halo<FMT, VARIANT, SA, SC, kNormFromArgument, true, halo_tile_threads(FMT, SC)>;
    return k;
}

template <int FMT, int VARIANT>
FusedNormKernels pick_splits(bool sa, bool sc)
{
    if constexpr (FMT == kBc3) {
        if (sa)
            return sc ? kernels<FMT, VARIANT, true, true>() : kernels<FMT, VARIANT, true, false>();
    }
    return sc ? kernels<FMT, VARIANT, false, true>() : kernels<FMT, VARIANT, false, false>();
}

template <int FMT>
FusedNormKernels pick_variant(int variant, bool sa, bool sc)
{
    switch (variant) {
    case kNone: return pick_splits<FMT, kNone>(sa, sc);
    case kVar1: return pick_splits<FMT, kVar1>(sa, sc);
    case kVar2: return pick_splits<FMT, kVar2>(sa, sc);
    default: return pick_splits<FMT, kVar3>(sa, sc);
    }
}

}  // namespace

FusedNormKernels fused_norm_kernels_bc23(Format fmt, int variant, bool sa, bool sc)
{
    return fmt == kBc2 ? pick_variant<kBc2>(variant, false, sc) : pick_variant<kBc3>(variant, sa, sc);
}

}  // namespace dxtlt
