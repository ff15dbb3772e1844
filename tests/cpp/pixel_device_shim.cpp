// Host shim over csrc/pixel_device.h for tests/test_pixel_device.py: the register helpers of the pixel kernels, compiled by the
// host compiler (byte_perm takes its portable branch) and run over arrays of cases.  Bytes travel as they lie in memory: a
// vector of 16 bytes is four little-endian dwords, sixteen pixels are 4 B dwords.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../dxt-lossless-transform_amd/csrc/pixel_device.h"

namespace px = dxtlt::pixels;

namespace {

template <int B>
void deinterleave_n(const uint8_t* in, uint8_t* planes, size_t n)
{
    for (size_t k = 0; k < n; ++k) {
        uint32_t w[4 * B], pl[B][4];
        memcpy(w, in + 16 * B * k, sizeof w);
        px::Pixels16<B>::deinterleave(w, pl);
        memcpy(planes + 16 * B * k, pl, sizeof pl);
    }
}

template <int B>
void interleave_n(const uint8_t* planes, uint8_t* out, size_t n)
{
    for (size_t k = 0; k < n; ++k) {
        uint32_t w[4 * B], pl[B][4];
        memcpy(pl, planes + 16 * B * k, sizeof pl);
        px::Pixels16<B>::interleave(pl, w);
        memcpy(out + 16 * B * k, w, sizeof w);
    }
}

template <int B, bool INVERSE>
void decorrelate_n(uint8_t* planes, size_t n)
{
    for (size_t k = 0; k < n; ++k) {
        uint32_t pl[B][4];
        memcpy(pl, planes + 16 * B * k, sizeof pl);
        px::decorrelate_planes<B, INVERSE>(pl);
        memcpy(planes + 16 * B * k, pl, sizeof pl);
    }
}

}  // namespace

extern "C" {

void shim_pixel_byte_add(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n)
{
    for (size_t k = 0; k < n; ++k)
        out[k] = px::byte_add(a[k], b[k]);
}

void shim_pixel_byte_sub(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n)
{
    for (size_t k = 0; k < n; ++k)
        out[k] = px::byte_sub(a[k], b[k]);
}

// n groups of sixteen pixels (16 B bytes each) <-> n groups of B planes of 16 bytes; -1 for a pixel size the header does not have
int shim_pixel_deinterleave(int pixel_bytes, const uint8_t* in, uint8_t* planes, size_t n)
{
    if (pixel_bytes == 4)
        deinterleave_n<4>(in, planes, n);
    else if (pixel_bytes == 3)
        deinterleave_n<3>(in, planes, n);
    else
        return -1;
    return 0;
}

int shim_pixel_interleave(int pixel_bytes, const uint8_t* planes, uint8_t* out, size_t n)
{
    if (pixel_bytes == 4)
        interleave_n<4>(planes, out, n);
    else if (pixel_bytes == 3)
        interleave_n<3>(planes, out, n);
    else
        return -1;
    return 0;
}

// subtract-green (inverse: add it back) on n groups of B planes of 16 bytes, in place
int shim_pixel_decorrelate_planes(int pixel_bytes, int inverse, uint8_t* planes, size_t n)
{
    if (pixel_bytes == 4)
        inverse ? decorrelate_n<4, true>(planes, n) : decorrelate_n<4, false>(planes, n);
    else if (pixel_bytes == 3)
        inverse ? decorrelate_n<3, true>(planes, n) : decorrelate_n<3, false>(planes, n);
    else
        return -1;
    return 0;
}

// n vectors of 16 bytes, in place; prev[k] is the byte in front of vector k
void shim_pixel_delta16(uint8_t* p, const uint8_t* prev, size_t n)
{
    for (size_t k = 0; k < n; ++k) {
        uint32_t v[4];
        memcpy(v, p + 16 * k, sizeof v);
        px::delta16(v, prev[k]);
        memcpy(p + 16 * k, v, sizeof v);
    }
}

// n vectors of 16 bytes, in place; ret[k] is the function's return value, all 32 bits of it
void shim_pixel_scan16(uint8_t* p, uint32_t* ret, size_t n)
{
    for (size_t k = 0; k < n; ++k) {
        uint32_t v[4];
        memcpy(v, p + 16 * k, sizeof v);
        ret[k] = px::scan16(v);
        memcpy(p + 16 * k, v, sizeof v);
    }
}

void shim_pixel_add_to_all16(uint8_t* p, const uint8_t* x, size_t n)
{
    for (size_t k = 0; k < n; ++k) {
        uint32_t v[4];
        memcpy(v, p + 16 * k, sizeof v);
        px::add_to_all16(v, x[k]);
        memcpy(p + 16 * k, v, sizeof v);
    }
}

}  // extern "C"
