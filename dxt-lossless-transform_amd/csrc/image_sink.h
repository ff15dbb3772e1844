// image_sink.h -- where the sixteen pixels of a decoded block go in a row-major image of bpp bytes per pixel: 4 (RGBA8888, the
// default), 1 (R8, BC4) or 2 (RG8, BC5).  Host and device code; the tests build it for the host.  The image is width x height
// pixels, pixel (x, y) at pixels + y * pitch + bpp * x; its blocks are numbered row-major over blocks_per_row = ceil(width / 4)
// columns and ceil(height / 4) rows.  A block of the last column or row may reach over the image's edge: the columns and rows
// that do not exist are never written.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace dxtlt {

struct ImageSink {
    uint8_t* pixels;
    uint64_t pitch;           // bytes from one pixel row to the next
    uint64_t blocks_per_row;  // ceil(width / 4)
    uint32_t width, height;   // pixels
    uint32_t bpp;             // bytes per pixel
};

inline ImageSink make_image_sink(void* pixels, uint64_t pitch, uint32_t width, uint32_t height, uint32_t bpp = 4)
{
    return ImageSink{static_cast<uint8_t*>(pixels), pitch, ((uint64_t)width + 3) / 4, width, height, bpp};
}

// blocks of the image
__host__ __device__ inline uint64_t image_blocks(const ImageSink& s) { return s.blocks_per_row * (((uint64_t)s.height + 3) / 4); }

struct BlockPlace {
    uint32_t bx, by;   // block column and row
    uint64_t offset;   // byte offset from `pixels` of the block's pixel (0, 0); its pixel row r starts `r * pitch` further
    uint32_t cols;     // 1..4: the block's pixel columns [0, cols) lie inside the image
    uint32_t rows;     // 1..4: the same for its pixel rows
};

// block `b` < image_blocks(s).  BPP: the bytes per pixel when the caller knows them at compile time (the kernels, whose format
// fixes them), 0 = s.bpp.
template <int BPP = 0>
__host__ __device__ inline BlockPlace place_block(const ImageSink& s, uint64_t b)
{
    const uint32_t block_row_bytes = 4u * (BPP != 0 ? (uint32_t)BPP : s.bpp);
    BlockPlace p;
    // (an image of 2^32 blocks or more is 64 Gpixel: the 64-bit division is for completeness)
    if ((b >> 32) == 0)
        p.by = (uint32_t)b / (uint32_t)s.blocks_per_row;   // blocks_per_row <= 2^30
    else
        p.by = (uint32_t)(b / s.blocks_per_row);
    p.bx = (uint32_t)(b - (uint64_t)p.by * s.blocks_per_row);
    p.offset = (uint64_t)p.by * 4u * s.pitch + (uint64_t)p.bx * block_row_bytes;
    const uint32_t left_x = s.width - 4u * p.bx, left_y = s.height - 4u * p.by;
    p.cols = left_x < 4u ? left_x : 4u;
    p.rows = left_y < 4u ? left_y : 4u;
    return p;
}

// address of pixel row r of the block
__host__ __device__ inline uint8_t* block_row(const ImageSink& s, const BlockPlace& p, int r)
{
    return s.pixels + p.offset + (uint64_t)r * s.pitch;
}

}  // namespace dxtlt
