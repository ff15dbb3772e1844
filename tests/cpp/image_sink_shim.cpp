// Host build of csrc/image_sink.h for tests/test_image_layout.py: every (byte address, block, pixel of the block) the sink
// produces for an image.  Addresses are numbers: nothing is dereferenced.
#include <cstddef>
#include <cstdint>
#define __host__
#define __device__
#include "../../dxt-lossless-transform_amd/csrc/image_sink.h"

extern "C" {

// one record per pixel the sink writes, in block order; returns the number of records (those beyond `cap` are counted only)
size_t shim_image_sink_pixels(uint64_t base, uint64_t pitch, uint32_t width, uint32_t height, uint64_t* address, uint64_t* block,
                              uint32_t* pixel, size_t cap)
{
    const dxtlt::ImageSink s = dxtlt::make_image_sink(reinterpret_cast<void*>(static_cast<uintptr_t>(base)), pitch, width, height);
    size_t n = 0;
    for (uint64_t b = 0; b < dxtlt::image_blocks(s); ++b) {
        const dxtlt::BlockPlace p = dxtlt::place_block(s, b);
        for (uint32_t r = 0; r < p.rows; ++r)
            for (uint32_t c = 0; c < p.cols; ++c) {
                if (n < cap) {
                    address[n] = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(dxtlt::block_row(s, p, (int)r))) + 4 * c;
                    block[n] = b;
                    pixel[n] = 4 * r + c;
                }
                ++n;
            }
    }
    return n;
}

// (bx, by, cols, rows) of block b
void shim_image_sink_place(uint64_t pitch, uint32_t width, uint32_t height, uint64_t b, uint32_t out[4])
{
    const dxtlt::ImageSink s = dxtlt::make_image_sink(nullptr, pitch, width, height);
    const dxtlt::BlockPlace p = dxtlt::place_block(s, b);
    out[0] = p.bx, out[1] = p.by, out[2] = p.cols, out[3] = p.rows;
}

uint64_t shim_image_blocks(uint32_t width, uint32_t height)
{
    return dxtlt::image_blocks(dxtlt::make_image_sink(nullptr, 0, width, height));
}

}  // extern "C"
