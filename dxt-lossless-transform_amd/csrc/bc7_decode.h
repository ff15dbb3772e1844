// bc7_decode.h -- BC7 block -> sixteen RGBA8888 pixels, in registers; host and device code (docs/IMAGE_DECODE.md, "BC7").
// The kernels of bc7_image_kernels.hip and the host call dxtlt_decode_bc7_blocks use it; tests/cpp/bc7_decode_shim.cpp builds it
// with g++ for the comparison with the numpy statement (tests/bc7_decode_ref.py) and with Pillow's decoder.
//
// Definition: the Direct3D 11 BC7 decoder.  Mode = trailing zeros of byte 0; fields in the order of docs/BC7_FORMAT.md section 1
// (bc7_fields.h has their positions): partition / rotation / index selector, the endpoints channel by channel, the p-bits, the
// indices.  A p-bit becomes the lowest bit of every channel of its endpoint(s); a channel of width w becomes 8 bits by
// (v << (8 - w)) | (v >> (2 w - 8)); modes 0..3 have alpha 255.  Every subset's anchor pixel stores one index bit less (implied
// high zero).  A channel is ((64 - w) e0 + w e1 + 32) >> 6 with the weight w of its index; rotation 1 / 2 / 3 swaps alpha with
// r / g / b afterwards.  The reserved encoding (byte 0 == 0) gives sixteen pixels of four zero bytes.
//
// How it maps to the machine.  Every mode is one instantiation of decode_mode<M>: all field positions are compile-time constants
// (v_bfe / v_alignbit on the four dwords), the pixel loop is unrolled, and the endpoint arrays are only ever indexed by
// constants, so nothing lives in scratch.  What varies per lane is the partition: its pixel -> subset map and its anchors come
// from three 64-entry tables of packed constants (constant memory: a 16-bit mask and a 4-bit anchor per two-subset partition, 32
// bits and two 4-bit anchors per three-subset partition), the anchors' missing bits are put into the index stream by one
// shift-and-mask each, so that pixel i's index sits at bit B i for every partition, and a pixel's endpoints are picked from its
// subset's by selects.  Two channels are interpolated at a time (r | b << 16 and g | a << 16: 64 * 255 + 32 < 2^16, no carry
// crosses).  decode_bc7_block's switch is over the lane's own mode: a wave whose 64 blocks are of one mode runs one arm.
#pragma once
#include "bc7_fields.h"

#if defined(__HIPCC__)
#define BC7_UNROLL _Pragma("unroll")
#else
#define BC7_UNROLL
#endif

namespace dxtlt {
namespace bc7 {

// subsets; partition, rotation and index-selector bits of the header; p-bits (0 none, 1 one per endpoint, 2 one per subset);
// index widths (the second set: modes 4 and 5)
struct DecodeDesc {
    int subsets, partition_bits, rotation_bits, selector_bits, pbits, index_bits, index2_bits;
};
constexpr DecodeDesc kDecodeDesc[8] = {
    {3, 4, 0, 0, 1, 3, 0}, {2, 6, 0, 0, 2, 3, 0}, {3, 6, 0, 0, 0, 2, 0}, {2, 6, 0, 0, 1, 2, 0},
    {1, 0, 2, 1, 0, 2, 3}, {1, 0, 2, 0, 0, 2, 2}, {1, 0, 0, 0, 1, 4, 0}, {2, 6, 0, 0, 1, 2, 0},
};
constexpr int n_pbits(int m) { return kDecodeDesc[m].pbits == 1 ? 2 * kDecodeDesc[m].subsets : kDecodeDesc[m].pbits == 2 ? kDecodeDesc[m].subsets : 0; }
constexpr int index_start(int m) { return endpoints_end(m) + n_pbits(m); }
constexpr int index_end(int m)
{
    return index_start(m) + 16 * kDecodeDesc[m].index_bits - kDecodeDesc[m].subsets +
           (kDecodeDesc[m].index2_bits != 0 ? 16 * kDecodeDesc[m].index2_bits - 1 : 0);
}
constexpr bool decode_desc_fits()
{
    for (int m = 0; m < 8; ++m) {
        const DecodeDesc d = kDecodeDesc[m];
        if (index_end(m) != 128 || kModeDesc[m].hdr != d.partition_bits + d.rotation_bits + d.selector_bits ||
            kModeDesc[m].n_rgb != 6 * d.subsets || (kModeDesc[m].n_a != 0 && kModeDesc[m].n_a != 2 * d.subsets))
            return false;
    }
    return true;
}
static_assert(decode_desc_fits(), "header, endpoints, p-bits and indices fill the 128 bits of every mode");

// weight of an index of `bits` bits: {0,21,43,64}, {0,9,18,27,37,46,55,64}, {0,4,9,13,...,60,64} = (64 i + n / 2) / n with
// n = 2^bits - 1, the division as a multiplication
constexpr uint32_t weight_of(int bits, uint32_t i)
{
    return bits == 2 ? ((64u * i + 1u) * 683u) >> 11 : bits == 3 ? ((64u * i + 3u) * 9363u) >> 16 : ((64u * i + 7u) * 4370u) >> 16;
}
constexpr bool weights_are_the_tables()
{
    constexpr uint32_t w2[4] = {0, 21, 43, 64}, w3[8] = {0, 9, 18, 27, 37, 46, 55, 64};
    constexpr uint32_t w4[16] = {0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64};
    for (uint32_t i = 0; i < 16; ++i)
        if ((i < 4 && weight_of(2, i) != w2[i]) || (i < 8 && weight_of(3, i) != w3[i]) || weight_of(4, i) != w4[i])
            return false;
    return true;
}
static_assert(weights_are_the_tables(), "the three weight tables of the format");

// ---- the partition tables, packed ------------------------------------------------------------------------------------------
// two subsets: bit i = subset of pixel i; bits 16..19 = anchor pixel of subset 1
BC7_HD uint32_t partition2_entry(uint32_t p)
{
    static constexpr uint32_t t[64] = {
        0xFCCCCu, 0xF8888u, 0xFEEEEu, 0xFECC8u, 0xFC880u, 0xFFEECu, 0xFFEC8u, 0xFEC80u, 0xFC800u, 0xFFFECu, 0xFFE80u, 0xFE800u,
        0xFFFE8u, 0xFFF00u, 0xFFFF0u, 0xFF000u, 0xFF710u, 0x2008Eu, 0x87100u, 0x208CEu, 0x2008Cu, 0x87310u, 0x83100u, 0xF8CCEu,
        0x2088Cu, 0x83110u, 0x26666u, 0x2366Cu, 0x817E8u, 0x80FF0u, 0x2718Eu, 0x2399Cu, 0xFAAAAu, 0xFF0F0u, 0x65A5Au, 0x833CCu,
        0x23C3Cu, 0x855AAu, 0xF9696u, 0xFA55Au, 0x273CEu, 0x813C8u, 0x2324Cu, 0x23BDCu, 0x26996u, 0xFC33Cu, 0xF9966u, 0x60660u,
        0x60272u, 0x204E4u, 0x64E40u, 0x82720u, 0xFC936u, 0xF936Cu, 0x239C6u, 0x2639Cu, 0xF9336u, 0xF9CC6u, 0xF817Eu, 0xFE718u,
        0xFCCF0u, 0x20FCCu, 0x27744u, 0xFEE22u,
    };
    return t[p];
}

// three subsets: bits 2 i, 2 i + 1 = subset of pixel i
BC7_HD uint32_t partition3_entry(uint32_t p)
{
    static constexpr uint32_t t[64] = {
        0xAA685050u, 0x6A5A5040u, 0x5A5A4200u, 0x5450A0A8u, 0xA5A50000u, 0xA0A05050u, 0x5555A0A0u, 0x5A5A5050u, 0xAA550000u, 0xAA555500u,
        0xAAAA5500u, 0x90909090u, 0x94949494u, 0xA4A4A4A4u, 0xA9A59450u, 0x2A0A4250u, 0xA5945040u, 0x0A425054u, 0xA5A5A500u, 0x55A0A0A0u,
        0xA8A85454u, 0x6A6A4040u, 0xA4A45000u, 0x1A1A0500u, 0x0050A4A4u, 0xAAA59090u, 0x14696914u, 0x69691400u, 0xA08585A0u, 0xAA821414u,
        0x50A4A450u, 0x6A5A0200u, 0xA9A58000u, 0x5090A0A8u, 0xA8A09050u, 0x24242424u, 0x00AA5500u, 0x24924924u, 0x24499224u, 0x50A50A50u,
        0x500AA550u, 0xAAAA4444u, 0x66660000u, 0xA5A0A5A0u, 0x50A050A0u, 0x69286928u, 0x44AAAA44u, 0x66666600u, 0xAA444444u, 0x54A854A8u,
        0x95809580u, 0x96969600u, 0xA85454A8u, 0x80959580u, 0xAA141414u, 0x96960000u, 0xAAAA1414u, 0xA05050A0u, 0xA0A5A5A0u, 0x96000000u,
        0x40804080u, 0xA9A8A9A8u, 0xAAAAAA44u, 0x2A4A5254u,
    };
    return t[p];
}

// three subsets: bits 0..3 = anchor pixel of subset 1, bits 4..7 = of subset 2
BC7_HD uint32_t anchors3_entry(uint32_t p)
{
    static constexpr uint8_t t[64] = {
        0xF3, 0x83, 0x8F, 0x3F, 0xF8, 0xF3, 0x3F, 0x8F, 0xF8, 0xF8, 0xF6, 0xF6, 0xF6, 0xF5, 0xF3, 0x83, 0xF3, 0x83, 0xF8, 0x3F,
        0xF3, 0x83, 0xF6, 0x8A, 0x35, 0xF8, 0x68, 0xA6, 0xF8, 0xF5, 0xAF, 0x8F, 0xF8, 0x3F, 0xF3, 0xA5, 0xA6, 0x8A, 0x98, 0xAF,
        0x6F, 0xF3, 0x8F, 0xF5, 0x3F, 0x6F, 0x6F, 0x8F, 0xF3, 0x3F, 0xF5, 0xF5, 0xF5, 0xF8, 0xF5, 0xFA, 0xF5, 0xFA, 0xF8, 0xFD,
        0x3F, 0xFC, 0xF3, 0x83,
    };
    return t[p];
}

template <int B>
struct IndexWord {
    using type = uint64_t;
};
template <>
struct IndexWord<2> {
    using type = uint32_t;
};

// ---- pieces ------------------------------------------------------------------------------------------------------------------
// a channel of W bits (5..8) as 8 bits
template <int W>
BC7_HD uint32_t to8(uint32_t v)
{
    static_assert(W >= 4 && W <= 8, "the shift right is by 2 W - 8");
    return ((v << (8 - W)) | (v >> (2 * W - 8))) & 0xFFu;
}

// endpoint E of the block (subset E / 2, end E % 2) as r | b << 16 and g | a << 16, 8 bits each
template <int M, int E>
BC7_HD void endpoint_8888(const B128& b, uint32_t& rb, uint32_t& ga)
{
    constexpr int NE = channel_fields(M), wc = kModeDesc[M].w_rgb, wa = kModeDesc[M].w_a, pm = kDecodeDesc[M].pbits;
    constexpr int np = pm != 0 ? 1 : 0;
    uint32_t r = get_bits<endpoint_pos(M, E), wc>(b), g = get_bits<endpoint_pos(M, NE + E), wc>(b);
    uint32_t bl = get_bits<endpoint_pos(M, 2 * NE + E), wc>(b), a = 0;
    if constexpr (wa != 0)
        a = get_bits<endpoint_pos(M, 3 * NE + E), wa>(b);
    if constexpr (pm != 0) {
        const uint32_t p = get_bits<endpoints_end(M) + (pm == 1 ? E : E / 2), 1>(b);
        r = (r << 1) | p, g = (g << 1) | p, bl = (bl << 1) | p, a = (a << 1) | p;
    }
    if constexpr (wa != 0)
        a = to8<wa + np>(a);
    else
        a = 255u;
    rb = to8<wc + np>(r) | (to8<wc + np>(bl) << 16);
    ga = to8<wc + np>(g) | (a << 16);
}

template <int M, int E>
BC7_HD void endpoints_8888(const B128& b, uint32_t (&rb)[6], uint32_t (&ga)[6])
{
    if constexpr (E < channel_fields(M)) {
        endpoint_8888<M, E>(b, rb[E], ga[E]);
        endpoints_8888<M, E + 1>(b, rb, ga);
    }
}

// x with a zero put in at bit p: the bits from p on move up by one
template <typename T>
BC7_HD T with_zero_at(T x, uint32_t p)
{
    const T low = (T)(((T)1 << p) - 1);
    return (T)((x & low) | ((x & (T)~low) << 1));
}

// The index set that starts at bit POS -- B bits per pixel, the NS anchors (pixel 0, a1, a2) one bit less -- as a regular array:
// pixel i's index at bit B i.  uint32_t for B == 2, uint64_t otherwise.
template <int POS, int B, int NS, typename T>
BC7_HD T index_array(const B128& b, uint32_t a1, uint32_t a2)
{
    constexpr int len = 16 * B - NS;
    T x = (T)get_bits<POS, (len < 32 ? len : 32)>(b);
    if constexpr (len > 32)
        x |= (T)((uint64_t)get_bits<POS + 32, len - 32>(b) << 32);
    x = with_zero_at<T>(x, B - 1);
    if constexpr (NS == 2)
        x = with_zero_at<T>(x, a1 * B + (B - 1));
    if constexpr (NS == 3) {   // in ascending order: a position counts the zeros put in below it
        const uint32_t first = a1 < a2 ? a1 : a2, second = a1 < a2 ? a2 : a1;
        x = with_zero_at<T>(with_zero_at<T>(x, first * B + (B - 1)), second * B + (B - 1));
    }
    return x;
}

// two 8-bit channels in the halves of a dword
BC7_HD uint32_t lerp_pair(uint32_t e0, uint32_t e1, uint32_t w) { return (((64u - w) * e0 + w * e1 + 0x00200020u) >> 6) & 0x00FF00FFu; }

// D.byte[i] = x.byte[sel.byte[i]]
BC7_HD uint32_t pick_bytes(uint32_t x, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0u, x, sel);
#else
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i)
        out |= ((x >> (8 * ((sel >> (8 * i)) & 3u))) & 0xFFu) << (8 * i);
    return out;
#endif
}

template <int B, typename T>
BC7_HD uint32_t index_of(T x, int i)
{
    return (uint32_t)(x >> (B * i)) & ((1u << B) - 1u);
}

// ---- one mode ----------------------------------------------------------------------------------------------------------------
// px[4 r + c] = pixel (c, r) as r | g << 8 | b << 16 | a << 24
template <int M>
BC7_HD void decode_mode(const B128& b, uint32_t (&px)[16])
{
    constexpr DecodeDesc d = kDecodeDesc[M];
    constexpr int NS = d.subsets, B = d.index_bits, B2 = d.index2_bits, hdr0 = M + 1;
    using Idx = typename IndexWord<B>::type;
    uint32_t rb[6] = {0, 0, 0, 0, 0, 0}, ga[6] = {0, 0, 0, 0, 0, 0};   // indexed by constants only
    endpoints_8888<M, 0>(b, rb, ga);

    uint32_t part = 0, a1 = 0, a2 = 0;
    if constexpr (NS == 2) {
        const uint32_t e = partition2_entry(get_bits<hdr0, d.partition_bits>(b));
        part = e & 0xFFFFu, a1 = e >> 16;
    }
    if constexpr (NS == 3) {
        const uint32_t p = get_bits<hdr0, d.partition_bits>(b), a = anchors3_entry(p);
        part = partition3_entry(p), a1 = a & 15u, a2 = a >> 4;
    }
    const Idx idx = index_array<index_start(M), B, NS, Idx>(b, a1, a2);

    if constexpr (B2 == 0) {
        BC7_UNROLL
        for (int i = 0; i < 16; ++i) {
            uint32_t rb0 = rb[0], rb1 = rb[1], ga0 = ga[0], ga1 = ga[1];
            if constexpr (NS == 2) {
                const bool s = ((part >> i) & 1u) != 0;
                rb0 = s ? rb[2] : rb0, rb1 = s ? rb[3] : rb1, ga0 = s ? ga[2] : ga0, ga1 = s ? ga[3] : ga1;
            }
            if constexpr (NS == 3) {
                const uint32_t s = (part >> (2 * i)) & 3u;
                rb0 = s == 1 ? rb[2] : s == 2 ? rb[4] : rb0, rb1 = s == 1 ? rb[3] : s == 2 ? rb[5] : rb1;
                ga0 = s == 1 ? ga[2] : s == 2 ? ga[4] : ga0, ga1 = s == 1 ? ga[3] : s == 2 ? ga[5] : ga1;
            }
            const uint32_t w = weight_of(B, index_of<B, Idx>(idx, i));
            px[i] = lerp_pair(rb0, rb1, w) | (lerp_pair(ga0, ga1, w) << 8);
        }
    } else {
        // modes 4 and 5: one subset, a second index set for alpha, a rotation; mode 4's selector exchanges the two sets
        using Idx2 = typename IndexWord<B2>::type;
        const Idx2 idx2 = index_array<index_start(M) + 16 * B - 1, B2, 1, Idx2>(b, 0, 0);
        const uint32_t rot = get_bits<hdr0, 2>(b);
        const bool exchanged = d.selector_bits != 0 && get_bits<hdr0 + 2, d.selector_bits>(b) != 0;
        // alpha <-> r, g, b: the byte that takes alpha's place
        const uint32_t sel = rot == 0 ? 0x03020100u : rot == 1 ? 0x00020103u : rot == 2 ? 0x01020300u : 0x02030100u;
        const uint32_t g0 = ga[0] & 0xFFFFu, g1 = ga[1] & 0xFFFFu, al0 = ga[0] >> 16, al1 = ga[1] >> 16;
        BC7_UNROLL
        for (int i = 0; i < 16; ++i) {
            const uint32_t w_first = weight_of(B, index_of<B, Idx>(idx, i)), w_second = weight_of(B2, index_of<B2, Idx2>(idx2, i));
            const uint32_t wc = exchanged ? w_second : w_first, wa = exchanged ? w_first : w_second;
            const uint32_t g = ((64u - wc) * g0 + wc * g1 + 32u) >> 6, a = ((64u - wa) * al0 + wa * al1 + 32u) >> 6;
            px[i] = pick_bytes(lerp_pair(rb[0], rb[1], wc) | (g << 8) | (a << 24), sel);
        }
    }
}

// the block's sixteen pixels: px[4 r + c] = pixel (c, r), bytes r, g, b, a (Decoded4x4Block)
BC7_HD void decode_bc7_block(const B128& b, uint32_t (&px)[16])
{
    switch (block_class(b.d[0])) {
    case 0: decode_mode<0>(b, px); break;
    case 1: decode_mode<1>(b, px); break;
    case 2: decode_mode<2>(b, px); break;
    case 3: decode_mode<3>(b, px); break;
    case 4: decode_mode<4>(b, px); break;
    case 5: decode_mode<5>(b, px); break;
    case 6: decode_mode<6>(b, px); break;
    case 7: decode_mode<7>(b, px); break;
    default:   // the reserved encoding
        for (int i = 0; i < 16; ++i)
            px[i] = 0;
    }
}

}  // namespace bc7
}  // namespace dxtlt
