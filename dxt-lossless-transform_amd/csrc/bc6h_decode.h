// bc6h_decode.h -- BC6H block -> sixteen RGBA16F pixels, in registers; host and device code (docs/IMAGE_DECODE.md, "BC6H blocks to
// a row-major RGBA16F image").  The kernels of bc6h_image_kernels.hip and the host call dxtlt_decode_bc6h_blocks use it;
// tests/cpp/bc6h_decode_shim.cpp builds it with g++ for the comparison with the numpy statement (tests/bc6h_decode_ref.py).
//
// Definition: the Direct3D 11 BC6H decoder for the UNSIGNED format (UF16); signed blocks are not decoded here.  Class = the mode
// bits of byte 0 (bc6h_fields.h, block_class); the endpoint fields w, x, y, z of each channel from the mode table
// (bc6h_decode_fields.h).  In the transformed modes x, y, z are deltas: sign-extended from their own width and added to w, modulo
// the base width.  An endpoint of `bits` bits is unquantised as 0 -> 0, all ones -> 0xFFFF, else ((c << 16) + 0x8000) >> bits,
// the identity from 15 bits on.  Two-region modes (classes 0..9) have a 5-bit partition -- the first 32 two-subset partitions of
// BC7 with their anchors -- and 3-bit indices, one-region modes 4-bit indices; every subset's anchor pixel stores one index bit
// less.  A channel is ((64 - w) e0 + w e1 + 32) >> 6 with the weight w of the pixel's index, then (c * 31) >> 6: a half-float bit
// pattern of at most 0x7BFF.  Alpha is 0x3C00 (1.0).  The four reserved mode values decode to r = g = b = 0.
//
// How it maps to the machine.  The mode-dependent work and the pixel loop are apart.  prepare_mode<K> -- one instantiation per
// class, every field position a compile-time constant, the field arrays only ever indexed by constants -- ends in an Interp: the
// unquantised endpoints, two to a dword (6 registers), the index bits with the anchors' missing bits put in, so that pixel i's
// index sits at bit B i (2), and the partition's subset mask with the index width beside it (1).  row_pixels() interpolates four
// pixels of it and depends on the mode only through that index width, which it takes as data: no branch.  The plain decoders run
// both back to back; the fused kernel (bc6h_image_sinks.h) keeps the Interp of its four blocks in registers -- 36 where their
// pixels would be 96 -- and interpolates a pixel row at a time on the way into LDS.
#pragma once
#include "bc6h_decode_fields.h"
#include "bc6h_fields.h"
#include "bc7_decode.h"   // BC7_UNROLL, partition2_entry, with_zero_at, weight_of

namespace dxtlt {
namespace bc6h {

constexpr uint32_t kHalfOne = 0x3C00u;

struct Interp {
    uint32_t c[6];       // c[3 s + ch]: channel ch of subset s, unquantised, e0 | e1 << 16
    uint32_t idx[2];     // pixel i's index at bit B i of idx[0] | idx[1] << 32, B = 3 (two regions) or 4
    uint32_t part;       // bit i: subset of pixel i; bit 16: two regions
};

template <int K, int I>
BC7_HD void gather_fields(const B128& b, uint32_t (&f)[12])   // f[4 ch + e]
{
    if constexpr (I < n_field_runs<K>()) {
        constexpr FieldRun r = DecodeTab<K>::runs[I];
        f[4 * r.ch + r.e] |= bc7::get_bits<r.src, r.len>(b) << r.dst;
        gather_fields<K, I + 1>(b, f);
    }
}

template <int BITS>
BC7_HD uint32_t unquantize(uint32_t c)
{
    if constexpr (BITS >= 15)
        return c;
    else
        return c == 0u ? 0u : c == low_mask(BITS) ? 0xFFFFu : ((c << 16) + 0x8000u) >> BITS;
}

template <int W>
BC7_HD uint32_t sign_extend(uint32_t v)
{
    constexpr uint32_t top = 1u << (W - 1);
    return (v ^ top) - top;
}

// channel CH of class K: the four (two) endpoints from their fields, unquantised, into c[CH] and c[3 + CH]
template <int K, int CH>
BC7_HD void endpoints_of_channel(const uint32_t (&f)[12], uint32_t (&c)[6])
{
    using T = DecodeTab<K>;
    constexpr int W = T::delta[CH];
    constexpr uint32_t mask = low_mask(T::bits);
    const uint32_t w = f[4 * CH];
    uint32_t x = f[4 * CH + 1], y = f[4 * CH + 2], z = f[4 * CH + 3];
    if constexpr (T::transformed) {
        x = (w + sign_extend<W>(x)) & mask;
        y = (w + sign_extend<W>(y)) & mask;
        z = (w + sign_extend<W>(z)) & mask;
    }
    c[CH] = unquantize<T::bits>(w) | (unquantize<T::bits>(x) << 16);
    c[3 + CH] = T::two_regions ? unquantize<T::bits>(y) | (unquantize<T::bits>(z) << 16) : 0u;
}

// ---- one class: everything that depends on the mode ---------------------------------------------------------------------------
template <int K>
BC7_HD Interp prepare_mode(const B128& b)
{
    using T = DecodeTab<K>;
    uint32_t f[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // indexed by constants only
    gather_fields<K, 0>(b, f);
    Interp s;
    endpoints_of_channel<K, 0>(f, s.c);
    endpoints_of_channel<K, 1>(f, s.c);
    endpoints_of_channel<K, 2>(f, s.c);
    uint64_t x;
    if constexpr (T::two_regions) {
        // partition at block bits 77..81, 46 index bits from bit 82 on: 3 per pixel, pixel 0 and the anchor of subset 1 one less
        const uint32_t e = bc7::partition2_entry(bc7::get_bits<77, 5>(b));
        s.part = (e & 0xFFFFu) | 0x10000u;
        x = (uint64_t)bc7::get_bits<82, 32>(b) | ((uint64_t)bc7::get_bits<114, 14>(b) << 32);
        x = bc7::with_zero_at<uint64_t>(bc7::with_zero_at<uint64_t>(x, 2u), (e >> 16) * 3u + 2u);
    } else {
        // 63 index bits from bit 65 on: 4 per pixel, pixel 0 one less
        s.part = 0u;
        x = (uint64_t)bc7::get_bits<65, 32>(b) | ((uint64_t)bc7::get_bits<97, 31>(b) << 32);
        x = bc7::with_zero_at<uint64_t>(x, 3u);
    }
    s.idx[0] = (uint32_t)x, s.idx[1] = (uint32_t)(x >> 32);
    return s;
}

// the reserved mode values: sixteen pixels of r = g = b = 0
BC7_HD Interp prepare_reserved() { return Interp{{0u, 0u, 0u, 0u, 0u, 0u}, {0u, 0u}, 0u}; }

BC7_HD Interp prepare_bc6h_block(const B128& b)
{
    switch (block_class(b.d[0])) {
#define DXTLT_C(k) case k: return prepare_mode<k>(b);
    DXTLT_BC6H_CASES(DXTLT_C)
#undef DXTLT_C
    default: return prepare_reserved();
    }
}

// ---- the pixels: the same code for every mode ---------------------------------------------------------------------------------
// weight of index i of a block of two regions (3 bits: bc7::weight_of(3, i)) or of one (4 bits), the constants as data
BC7_HD uint32_t index_weight(uint32_t i, bool two) { return ((64u * i + (two ? 3u : 7u)) * (two ? 9363u : 4370u)) >> 16; }
constexpr bool index_weights_are_the_tables()
{
    for (uint32_t i = 0; i < 16; ++i)
        if ((i < 8 && ((64u * i + 3u) * 9363u) >> 16 != bc7::weight_of(3, i)) || ((64u * i + 7u) * 4370u) >> 16 != bc7::weight_of(4, i))
            return false;
    return true;
}
static_assert(index_weights_are_the_tables(), "{0,9,18,27,37,46,55,64} and the sixteen-entry table");

// e0 | e1 << 16 at weight w -> the half
BC7_HD uint32_t interpolate(uint32_t pair, uint32_t w) { return ((((64u - w) * (pair & 0xFFFFu) + w * (pair >> 16) + 32u) >> 6) * 31u) >> 6; }

// pixel row r of the block: out[2 c] = r | g << 16, out[2 c + 1] = b | 1.0 << 16 of pixel (c, r) -- its eight bytes
BC7_HD void row_pixels(const Interp& s, int r, uint32_t (&out)[8])
{
    const bool two = (s.part & 0x10000u) != 0u;
    const uint32_t width = two ? 3u : 4u, imask = two ? 7u : 15u;
    const uint64_t idx = (uint64_t)s.idx[0] | ((uint64_t)s.idx[1] << 32);
    BC7_UNROLL
    for (int c = 0; c < 4; ++c) {
        const uint32_t i = 4u * (uint32_t)r + (uint32_t)c;
        const uint32_t w = index_weight((uint32_t)(idx >> (width * i)) & imask, two);
        const bool second = ((s.part >> i) & 1u) != 0u;
        const uint32_t red = interpolate(second ? s.c[3] : s.c[0], w), green = interpolate(second ? s.c[4] : s.c[1], w);
        const uint32_t blue = interpolate(second ? s.c[5] : s.c[2], w);
        out[2 * c] = red | (green << 16);
        out[2 * c + 1] = blue | (kHalfOne << 16);
    }
}

// the block's sixteen pixels: px[2 (4 r + c)], px[2 (4 r + c) + 1] = the eight bytes of pixel (c, r) as two little-endian dwords
BC7_HD void decode_bc6h_block(const B128& b, uint32_t (&px)[32])
{
    const Interp s = prepare_bc6h_block(b);
    BC7_UNROLL
    for (int r = 0; r < 4; ++r) {
        uint32_t row[8];
        row_pixels(s, r, row);
        BC7_UNROLL
        for (int k = 0; k < 8; ++k)
            px[8 * r + k] = row[k];
    }
}

}  // namespace bc6h
}  // namespace dxtlt
