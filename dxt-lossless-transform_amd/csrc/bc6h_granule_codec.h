// bc6h_granule_codec.h -- BC6H's codec for the granule sort of granule_sort.h: the record codec of bc6h_fields.h over 15 classes
// -- the 14 modes, then the reserved mode encodings -- so all four class bits are matched by ballots in every segment.  Included
// by bc6h_kernels.hip (the transform) and, through bc6h_image_sinks.h, by the image kernels (the inverse with a pixel sink).
#pragma once
#include "bc6h_fields.h"
#include "granule_sort.h"

namespace dxtlt {
namespace bc6h {

struct Bc6hCodec {
    static constexpr int kClasses = bc6h::kClasses;
    static constexpr int kCountsSpare = 0;
    static constexpr auto& block_class = bc6h::block_class;
    static constexpr auto& byte0 = bc6h_byte0;
    static constexpr auto& record = bc6h_record_any;
    static constexpr auto& block = bc6h_block_any;
    template <bool TAIL>
    static __device__ __forceinline__ void rank_and_count(uint8_t* lds, int cls, int lane, int segment, int& rank)
    {
        granule::rank_by_ballots<Bc6hCodec>(lds, cls, lane, segment, rank);
    }
};

}  // namespace bc6h
}  // namespace dxtlt
