// bc7_image_sinks.h -- what is BC7's own in its image kernels (granule_image.h writes the kernels once for BC7 and BC6H;
// bc7_image_batch_kernels.hip: the images of many buffers): the block decode of the plain decoders (their load is image_store.h's
// load_block), the stores of a part of a block, the staging sinks of the inverse granule sort -- Bc7PixelSink for one image,
// Bc7RegionPixelSinkOf for the images of a region table (image_regions.h) -- and Bc7Image, the family that names them all.
// docs/IMAGE_DECODE.md, "BC7" and "Several images of one BC7 buffer".
#pragma once
#include "bc7_decode.h"
#include "bc7_granule_codec.h"
#include "image_region_sinks.h"
#include "image_regions.h"
#include "image_store.h"

namespace dxtlt {
namespace bc7 {
namespace {

using granule::kT;

__device__ __forceinline__ void decode_px(u32x4 q, uint32_t (&px)[16])
{
    const B128 b = {{q.x, q.y, q.z, q.w}};
    decode_bc7_block(b, px);
}

// ---- the inverse granule sort with a pixel sink --------------------------------------------------------------------------
// A staging sink of inverse_granule (granule_sort.h, BlockSink).  The inverse has every block twice: in the sorted domain, where
// lane j holds sorted block j and a wave's 64 blocks are of one mode except where two classes meet, and -- behind its last
// barrier -- in block order, where a wave's 64 lanes hold 64 consecutive blocks of the image.  The decoder's mode switch wants the
// first, the stores want the second, so the pixels cross instead of the blocks: hold() decodes sorted block j into registers,
// stage() puts two of its four pixel rows into LDS (row k of the part at k * 16 KiB + 16 j: consecutive lanes, consecutive 16
// bytes), store_staged() fetches them for the lane's block-order block from its sorted position and stores them as the BC2 / BC3
// decoders do, 1 KiB of consecutive bytes of a pixel row per wave instruction; then the other two rows take the same way.  By then
// nothing else lives in LDS, so the 32 KiB of a part start at byte 0 and are the kernel's whole allocation.
// Block `b` of the buffer is block b - first_block of the image when it lies in [first_block, first_block + blocks); every block
// of a covered granule is decoded, the ones outside are dropped at the store.
// What else was built and measured (16384 x 16384; ms on a buffer of mode 6 only / the uniform / the skewed mode mix;
// profiles/bc7_image_bench.json, "ab"; docs/IMAGE_DECODE.md):
//   * decode in block order behind the un-sort, the mode switch per lane, 19 KiB of LDS: 0.238 / 1.431 / 1.058 -- a wave ran the
//     arm of every mode among its 64 blocks;
//   * this sink with all four rows in one part, 64 KiB of LDS, two workgroups per CU: 0.290 / 0.476 / 0.452;
//   * with one row per part, 19 KiB, six more barriers: 0.249 / 0.412 / 0.367;
//   * two rows per part (here), 32 KiB, five workgroups per CU by the 95 VGPRs: 0.231 / 0.401 / 0.355.
// rows [r0, r0 + ROWS) of block `b` of the image: store_block_pixels (image_store.h) for a part of a block
template <int ROWS>
__device__ __forceinline__ void store_block_rows(const ImageSink& img, uint64_t b, int r0, const u32x4 (&rows)[ROWS])
{
    const BlockPlace p = place_block<4>(img, b);
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(img.pixels) | img.pitch) & 15) == 0;   // uniform
    if (p.cols == 4 && p.rows == 4) {
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            uint8_t* row = block_row(img, p, r0 + k);
            if (aligned16)
                store_streaming16(row, rows[k]);
            else
                *reinterpret_cast<u32x4_align4*>(row) = rows[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            uint32_t* row = reinterpret_cast<uint32_t*>(block_row(img, p, r0 + k));
            const uint32_t px[4] = {rows[k].x, rows[k].y, rows[k].z, rows[k].w};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if ((uint32_t)(r0 + k) < p.rows && (uint32_t)c < p.cols)
                    row[c] = px[c];
        }
    }
}

struct Bc7PixelSink {
    static constexpr bool kStaged = true;
    static constexpr int kParts = 2, kRows = 4 / kParts;   // pixel rows per part
    static constexpr int kStageBytes = kRows * kT * 16;
    struct Held {
        uint32_t px[16];
    };
    ImageSink img;
    uint64_t first_block, blocks;

    __device__ __forceinline__ Held hold(const B128& b) const
    {
        Held h;
        decode_bc7_block(b, h.px);
        return h;
    }

    // row k of the part of sorted block j at k * 16 KiB + 16 j: consecutive lanes, consecutive 16 bytes
    __device__ __forceinline__ void stage(uint8_t* lds, int j, const Held& h, int part) const
    {
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const int r = part * kRows + k;
            granule::lds_at<u32x4>(lds, k * (kT * 16) + 16 * j) = u32x4{h.px[4 * r], h.px[4 * r + 1], h.px[4 * r + 2], h.px[4 * r + 3]};
        }
    }

    __device__ __forceinline__ void store_staged(uint8_t* lds, uint64_t b, int pos, int part) const
    {
        const uint64_t at = b - first_block;   // wraps for b < first_block
        if (at >= blocks)
            return;
        u32x4 rows[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k)
            rows[k] = granule::lds_at<u32x4>(lds, k * (kT * 16) + 16 * pos);
        store_block_rows<kRows>(img, at, part * kRows, rows);
    }
};

// ---- the same sink for the images of a region table ----------------------------------------------------------------------
// hold() and stage() are Bc7PixelSink's: the blocks are decoded in the sorted domain and their pixels cross through LDS exactly
// as for one image.  store_staged() differs in who owns the block: block `b` of the buffer belongs to whichever region of `tab`
// holds it, and to none in a gap.  Behind the barrier a wave's 64 lanes hold 64 consecutive blocks of the buffer, so the wave
// asks first, with its first block in scalar registers (wave_run, image_region_sinks.h): the image it finds is uniform and the
// stores are the single-image sink's, the streaming-or-plain choice uniform again.  Only a wave whose run straddles a boundary or
// touches a gap -- and the tail part's last, partly filled wave, whose run reaches past the buffer's end -- lets every lane
// search for itself; there the image, the store choice and the clipping are per lane.
// Three questions, the cheapest first.  prepare() asks once per granule, before the decode, whether ONE region holds the whole
// granule (or the whole tail part) -- all but a handful of the granules of a large image; its answer stays in scalar registers
// and serves every store of the granule.  Where it does not, the wave asks about its run of 64 and then the lanes about their
// blocks, inside store_staged and again for each of the two parts (and each of the lane's four blocks) instead of being held
// across the parts: what they find -- an ImageSink and a block number per held block, in vector registers on the per-lane path
// -- would otherwise live through the second part's stage() beside the decoded pixels (docs/IMAGE_DECODE.md, "Several images
// of one BC7 buffer", resources).
// No lane leaves here before inverse_granule's barriers: a block without an image only skips its stores.
// Written once for every kind of table the lookups of image_regions.h take, as the BC1 - BC5 region sinks are.
template <typename TABLE>
struct Bc7RegionPixelSinkOf {
    static constexpr bool kStaged = Bc7PixelSink::kStaged;
    static constexpr int kParts = Bc7PixelSink::kParts, kRows = Bc7PixelSink::kRows;
    static constexpr int kStageBytes = Bc7PixelSink::kStageBytes;
    using Held = Bc7PixelSink::Held;
    TABLE tab;

    // (the single-image sink's members do not read its fields)
    __device__ __forceinline__ Held hold(const B128& b) const { return Bc7PixelSink{}.hold(b); }
    __device__ __forceinline__ void stage(uint8_t* lds, int j, const Held& h, int part) const { Bc7PixelSink{}.stage(lds, j, h, part); }

    __device__ __forceinline__ void fetch_and_store(uint8_t* lds, const ImageSink& img, uint64_t local, int pos, int part) const
    {
        u32x4 rows[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k)
            rows[k] = granule::lds_at<u32x4>(lds, k * (kT * 16) + 16 * pos);
        store_block_rows<kRows>(img, local, part * kRows, rows);
    }

    // the region that holds the whole granule (tail part), if one does: most granules of a large image
    using Prepared = WaveRun;
    __device__ __forceinline__ Prepared prepare(uint64_t first, uint64_t n) const { return wave_run(tab, first, n); }

    __device__ __forceinline__ void store_staged(uint8_t* lds, uint64_t b, int pos, int part, const Prepared& whole) const
    {
        if (whole.region >= 0) {
            fetch_and_store(lds, whole.img, whole.local + (b - whole.first), pos, part);
            return;
        }
        // A granule -- and the tail part -- starts at a multiple of 1024 blocks and a wave holds places 64 w .. 64 w + 63 of it, so
        // the wave's first block is b with its low six bits cleared and the lane is those bits.  (Taking the lane from
        // threadIdx.x instead kept one more value alive through the decode -- 97 VGPRs, the fifth wave per SIMD gone -- in the form
        // that had no prepare().)
        static_assert(kT % 64 == 0, "a wave's 64 blocks start at a multiple of 64");
        const WaveRun run = wave_run(tab, b & ~(uint64_t)63, 64);
        if (run.region >= 0) {
            fetch_and_store(lds, run.img, run.local + (b & 63), pos, part);
        } else {
            ImageSink img{nullptr, 0, 1, 0, 0, 4};
            uint64_t local = 0;
            if (region_of_block(tab, b, img, local) >= 0)
                fetch_and_store(lds, img, local, pos, part);
        }
    }
};

}  // namespace

// BC7 as the kernels and launchers of granule_image.h see it: the family of RGBA8888 images.  Neither sink differs for the tail
// part.  The table of RegionSink is the one in the kernel arguments there; bc7_image_batch_kernels.hip has the one in device memory.
struct Bc7Image {
    using Codec = Bc7Codec;
    template <bool TAIL>
    using Sink = Bc7PixelSink;
    template <typename TABLE, bool TAIL>
    using RegionSink = Bc7RegionPixelSinkOf<TABLE>;
    static constexpr uint32_t kBpp = 4;
    // the plain decoders: a block's sixteen pixels, stored as the BC2 / BC3 plain decoder stores them (image_store.h)
    using Decoded = uint32_t[16];
    static __device__ __forceinline__ void decode(u32x4 q, Decoded& px) { decode_px(q, px); }
    static __device__ __forceinline__ void store(const ImageSink& img, uint64_t b, const Decoded& px) { store_block_pixels(img, b, px); }
};

}  // namespace bc7
}  // namespace dxtlt
