// pixel_device.h -- the register-level pieces of the uncompressed-pixel kernels (pixel_kernels.hip; docs/PIXEL_FORMAT.md):
// byte-wise arithmetic on four bytes per dword, the (de)interleave of 16 pixels held in registers, the delta of a 16-byte
// run and its inverse, the in-lane prefix sum.  Plain C++ on dwords, so the same code runs on the host: every function is
// a pure function of its arguments.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DXTLT_PIXEL_FN __host__ __device__ __forceinline__
#else
#define DXTLT_PIXEL_FN inline
#endif

namespace dxtlt {
namespace pixels {

// a + b and a - b on each of the four bytes, modulo 256, no carry between bytes: the low seven bits are added (subtracted
// under a set guard bit) and the top bits put back by xor
DXTLT_PIXEL_FN uint32_t byte_add(uint32_t a, uint32_t b)
{
    return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u);
}
DXTLT_PIXEL_FN uint32_t byte_sub(uint32_t a, uint32_t b)
{
    return ((a | 0x80808080u) - (b & 0x7F7F7F7Fu)) ^ ((a ^ ~b) & 0x80808080u);
}

// v_perm_b32: byte i of the result is byte sel[i] of the eight bytes {hi : lo} (0..3 = lo, 4..7 = hi)
DXTLT_PIXEL_FN uint32_t byte_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i)
        r |= (uint32_t)((both >> (8 * ((sel >> (8 * i)) & 7))) & 0xFF) << (8 * i);
    return r;
#endif
}

// Sixteen pixels of B bytes in 4 B dwords (memory order) <-> B planes of four dwords (byte i of a plane = byte c of pixel i).
template <int B>
struct Pixels16;

template <>
struct Pixels16<4> {
    // a 4 x 4 byte transpose per four pixels; it is its own inverse
    static DXTLT_PIXEL_FN void transpose(const uint32_t* in, uint32_t* o0, uint32_t* o1, uint32_t* o2, uint32_t* o3)
    {
        const uint32_t t0 = byte_perm(in[1], in[0], 0x05010400u), t1 = byte_perm(in[1], in[0], 0x07030602u);
        const uint32_t t2 = byte_perm(in[3], in[2], 0x05010400u), t3 = byte_perm(in[3], in[2], 0x07030602u);
        *o0 = byte_perm(t2, t0, 0x05040100u);
        *o1 = byte_perm(t2, t0, 0x07060302u);
        *o2 = byte_perm(t3, t1, 0x05040100u);
        *o3 = byte_perm(t3, t1, 0x07060302u);
    }
    static DXTLT_PIXEL_FN void deinterleave(const uint32_t (&w)[16], uint32_t (&pl)[4][4])
    {
        for (int k = 0; k < 4; ++k)
            transpose(&w[4 * k], &pl[0][k], &pl[1][k], &pl[2][k], &pl[3][k]);
    }
    static DXTLT_PIXEL_FN void interleave(const uint32_t (&pl)[4][4], uint32_t (&w)[16])
    {
        for (int k = 0; k < 4; ++k) {
            const uint32_t in[4] = {pl[0][k], pl[1][k], pl[2][k], pl[3][k]};
            transpose(in, &w[4 * k], &w[4 * k + 1], &w[4 * k + 2], &w[4 * k + 3]);
        }
    }
};

template <>
struct Pixels16<3> {
    // four pixels are three dwords: [c0 c1 c2 c0'] [c1' c2' c0" c1"] [c2" c0"' c1"' c2"']
    static DXTLT_PIXEL_FN void deinterleave(const uint32_t (&w)[12], uint32_t (&pl)[3][4])
    {
        for (int k = 0; k < 4; ++k) {
            const uint32_t d0 = w[3 * k], d1 = w[3 * k + 1], d2 = w[3 * k + 2];
            pl[0][k] = byte_perm(d2, byte_perm(d1, d0, 0x00060300u), 0x05020100u);
            pl[1][k] = byte_perm(d2, byte_perm(d1, d0, 0x00070401u), 0x06020100u);
            pl[2][k] = byte_perm(d2, byte_perm(d1, d0, 0x00000502u), 0x07040100u);
        }
    }
    static DXTLT_PIXEL_FN void interleave(const uint32_t (&pl)[3][4], uint32_t (&w)[12])
    {
        for (int k = 0; k < 4; ++k) {
            const uint32_t a = pl[0][k], b = pl[1][k], c = pl[2][k];
            w[3 * k] = byte_perm(c, byte_perm(b, a, 0x01000400u), 0x03040100u);
            w[3 * k + 1] = byte_perm(c, byte_perm(b, a, 0x06020005u), 0x03020500u);
            w[3 * k + 2] = byte_perm(c, byte_perm(b, a, 0x00070300u), 0x07020106u);
        }
    }
};

// subtract-green on planes: byte 0 and byte 2 of every pixel lose (forward) or regain (inverse) byte 1
template <int B, bool INVERSE>
DXTLT_PIXEL_FN void decorrelate_planes(uint32_t (&pl)[B][4])
{
    for (int k = 0; k < 4; ++k) {
        pl[0][k] = INVERSE ? byte_add(pl[0][k], pl[1][k]) : byte_sub(pl[0][k], pl[1][k]);
        pl[2][k] = INVERSE ? byte_add(pl[2][k], pl[1][k]) : byte_sub(pl[2][k], pl[1][k]);
    }
}

// p[i] - p[i - 1] over the 16 bytes of `p`, `prev` (0..255) in front of byte 0
DXTLT_PIXEL_FN void delta16(uint32_t (&p)[4], uint32_t prev)
{
    const uint32_t s0 = (p[0] << 8) | prev, s1 = (p[1] << 8) | (p[0] >> 24), s2 = (p[2] << 8) | (p[1] >> 24),
                   s3 = (p[3] << 8) | (p[2] >> 24);
    p[0] = byte_sub(p[0], s0);
    p[1] = byte_sub(p[1], s1);
    p[2] = byte_sub(p[2], s2);
    p[3] = byte_sub(p[3], s3);
}

// inclusive prefix sum modulo 256 over the 16 bytes of `p`, in place; returns the sum of all sixteen (the last byte)
DXTLT_PIXEL_FN uint32_t scan16(uint32_t (&p)[4])
{
    uint32_t carry = 0;
    for (int k = 0; k < 4; ++k) {
        uint32_t d = p[k];
        d = byte_add(d, d << 8);
        d = byte_add(d, d << 16);
        d = byte_add(d, carry * 0x01010101u);
        carry = d >> 24;
        p[k] = d;
    }
    return carry;
}

// adds the byte `x` (0..255) to all sixteen bytes
DXTLT_PIXEL_FN void add_to_all16(uint32_t (&p)[4], uint32_t x)
{
    for (int k = 0; k < 4; ++k)
        p[k] = byte_add(p[k], x * 0x01010101u);
}

}  // namespace pixels
}  // namespace dxtlt
