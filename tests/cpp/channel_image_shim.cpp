// Host build of csrc/image_sink.h with 1 and 2 bytes per pixel and of the BC4 / BC5 row decoders of csrc/bcn_decode.h, for
// tests/test_channel_image_layout.py.  Addresses are numbers: nothing is dereferenced.
#include <cstddef>
#include <cstdint>
#define __host__
#define __device__
#include "../../dxt-lossless-transform_amd/csrc/bcn_decode.h"
#include "../../dxt-lossless-transform_amd/csrc/image_sink.h"

extern "C" {

// one record per pixel the sink addresses, in block order: the address of the pixel's first byte, its block, its number in
// the block, and (cols, rows) of the block; returns the number of records (those beyond `cap` are counted only)
size_t shim_channel_sink_pixels(uint64_t base, uint64_t pitch, uint32_t width, uint32_t height, uint32_t bpp, uint64_t* address,
                                uint64_t* block, uint32_t* pixel, uint32_t* cols, uint32_t* rows, size_t cap)
{
    const dxtlt::ImageSink s = dxtlt::make_image_sink(reinterpret_cast<void*>(static_cast<uintptr_t>(base)), pitch, width, height, bpp);
    size_t n = 0;
    for (uint64_t b = 0; b < dxtlt::image_blocks(s); ++b) {
        const dxtlt::BlockPlace p = dxtlt::place_block(s, b);
        // the kernels know the bytes per pixel at compile time: that form must place the block where the member does
        const dxtlt::BlockPlace k = bpp == 1 ? dxtlt::place_block<1>(s, b) : bpp == 2 ? dxtlt::place_block<2>(s, b) : dxtlt::place_block<4>(s, b);
        if (k.bx != p.bx || k.by != p.by || k.offset != p.offset || k.cols != p.cols || k.rows != p.rows)
            return (size_t)-1;
        for (uint32_t r = 0; r < p.rows; ++r)
            for (uint32_t c = 0; c < p.cols; ++c) {
                if (n < cap) {
                    address[n] = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(dxtlt::block_row(s, p, (int)r))) + bpp * c;
                    block[n] = b;
                    pixel[n] = 4 * r + c;
                    cols[n] = p.cols;
                    rows[n] = p.rows;
                }
                ++n;
            }
    }
    return n;
}

// fmt = 4: 8-byte blocks -> 16 bytes of R8 pixels each; fmt = 5: 16-byte blocks -> 32 bytes of RG8 pixels each (row-major)
void shim_decode_channel_blocks(int fmt, const uint8_t* in, uint64_t num_blocks, uint8_t* out)
{
    for (uint64_t b = 0; b < num_blocks; ++b) {
        uint32_t q[4] = {0, 0, 0, 0};
        const int bs = fmt == 4 ? 8 : 16;
        for (int i = 0; i < bs; ++i)
            q[i >> 2] |= (uint32_t)in[bs * b + i] << (8 * (i & 3));
        if (fmt == 4) {
            uint32_t rows[4];
            dxtlt::decode_bc4_block_rows(q[0], q[1], rows);
            for (int i = 0; i < 16; ++i)
                out[16 * b + i] = (uint8_t)(rows[i >> 2] >> (8 * (i & 3)));
        } else {
            uint32_t rows[4][2];
            dxtlt::decode_bc5_block_rows(q, rows);
            for (int i = 0; i < 32; ++i)
                out[32 * b + i] = (uint8_t)(rows[i >> 3][(i >> 2) & 1] >> (8 * (i & 3)));
        }
    }
}

}  // extern "C"
