// bc6h_image_sinks.h -- what is BC6H's own in its image kernels (granule_image.h writes the kernels once for BC7 and BC6H): the
// block decode of the plain decoders (their load is image_store.h's load_block), the stores of a block's 32-byte pixel rows, the
// staging sinks of the inverse granule sort -- Bc6hPixelSink for one image, Bc6hRegionPixelSinkOf for the images of a region table
// (image_regions.h) -- and Bc6hImage, the family that names them all.
// docs/IMAGE_DECODE.md, "BC6H blocks to a row-major RGBA16F image" and "Several images of one BC6H buffer".
#pragma once
#include "bc6h_decode.h"
#include "bc6h_granule_codec.h"
#include "image_region_sinks.h"
#include "image_regions.h"
#include "image_store.h"

namespace dxtlt {
namespace bc6h {
namespace {

using granule::kT;

__device__ __forceinline__ Interp prepare_q(u32x4 q)
{
    const B128 b = {{q.x, q.y, q.z, q.w}};
    return prepare_bc6h_block(b);
}

// pixel row `r` of block `b` of the image, row[0] = pixels 0 and 1, row[1] = pixels 2 and 3: whole blocks in two 16-byte stores on
// 8-byte addresses, clipped blocks pixel by pixel.  The stores are PLAIN whatever the alignment: a lane owns 32 bytes of the row, so a
// wave instruction writes every other 16 bytes and the 128-byte lines are completed by the next one -- the shape streaming_store.h
// rules out for `sc1 nt`.  Measured (profiles/bc6h_image_bench.json, "ab"): with `sc1 nt` here, as the BC2 / BC3 plain decoder has
// it for its 16-byte rows, untransform + plain image decode of 16384 x 16384 took 1.97 ms (one class) / 2.06 (every class), with
// plain stores 0.55 / 0.90.
__device__ __forceinline__ void store_block_row(const ImageSink& img, const BlockPlace& p, int r, const u32x4 (&row)[2])
{
    uint8_t* at = block_row(img, p, r);
    if (p.cols == 4 && p.rows == 4) {
        *reinterpret_cast<u32x4_align8*>(at) = row[0];
        *reinterpret_cast<u32x4_align8*>(at + 16) = row[1];
    } else if ((uint32_t)r < p.rows) {
        u32x2* px = reinterpret_cast<u32x2*>(at);
        px[0] = u32x2{row[0].x, row[0].y};
        if (p.cols > 1)
            px[1] = u32x2{row[0].z, row[0].w};
        if (p.cols > 2)
            px[2] = u32x2{row[1].x, row[1].y};
        if (p.cols > 3)
            px[3] = u32x2{row[1].z, row[1].w};
    }
}

// the sixteen pixels of block `b` of the image from its prepared endpoints and indices, a row at a time
__device__ __forceinline__ void store_block_pixels(const ImageSink& img, uint64_t b, const Interp& s)
{
    const BlockPlace p = place_block<8>(img, b);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        uint32_t o[8];
        row_pixels(s, r, o);
        const u32x4 row[2] = {u32x4{o[0], o[1], o[2], o[3]}, u32x4{o[4], o[5], o[6], o[7]}};
        store_block_row(img, p, r, row);
    }
}

// ---- the inverse granule sort with a pixel sink --------------------------------------------------------------------------
// A staging sink of inverse_granule (granule_sort.h), shaped like Bc7PixelSink (bc7_image_sinks.h): decode in the sorted domain,
// where a wave's 64 blocks are of one class except where two classes meet, and cross to block order through LDS.  Two things
// differ.
// Registers.  A decoded block is 16 pixels x 3 halves = 24 registers, and a lane of the 256-lane workgroup holds four blocks.
// So Held is not the pixels but the Interp of bc6h_decode.h -- unquantised endpoints, normalised index bits, subset mask: nine
// registers a block -- made by hold(), the wave-uniform mode switch; the interpolation is deferred to stage(), which is the same
// code for every class, and makes only the pixel row of the part that is being staged.
// Stores.  A block's pixel row is 32 bytes, so the 64 consecutive blocks a wave holds behind the barrier own 2 KiB of a pixel row:
// 128 pieces of 16 bytes.  A part is ONE pixel row of the granule's 1024 blocks, 32 KiB, the row of sorted block j at 32 j.  The
// pixels come out by sorted position, so which lane fetches which piece is free: lane l takes pieces l and 64 + l of its wave's run
// -- the halves l & 1 of blocks l / 2 and 32 + l / 2, whose sorted positions it gets from their lanes by one cross-lane move each
// -- and every store instruction of a wave writes 1 KiB of consecutive bytes, `sc1 nt` where the image's pointer and pitch are
// multiples of 16.  That needs every lane of the wave at the store, which a full granule gives and a tail part does not (the
// lanes behind its last block never get there): TAIL, one workgroup per call, every lane fetches its own block's row and writes it
// with store_block_row.
// What else was built and measured (16384 x 16384; ms on a buffer of class 12 only / the every-class mix / the mix with an offset
// range; profiles/bc6h_image_bench.json, "ab"; docs/IMAGE_DECODE.md):
//   * every lane its own block's row in two `sc1 nt` stores, a wave instruction writing every other 16 bytes: 1.99 / 1.99 / 2.05;
//   * the same with two rows per part, 64 KiB of LDS: 2.03 / 2.02 / 2.06; the same with 512 lanes x 2 blocks: 1.96 / 1.96 / 2.03;
//   * this form with 512 lanes x 2 blocks (fewer registers, two more waves per SIMD): 0.516 / 0.513 / 0.514;
//   * this form, 256 lanes x 4 blocks (here): 0.494 / 0.542 / 0.543.
// Block `b` of the buffer is block b - first_block of the image when it lies in [first_block, first_block + blocks); every block
// of a covered granule is decoded, the ones outside are dropped at the store.

// 16 bytes -- pixels 2 half, 2 half + 1 -- of pixel row r of a block; whole blocks `sc1 nt` where the image allows it
__device__ __forceinline__ void store_half_row(const ImageSink& img, const BlockPlace& p, int r, int half, u32x4 v)
{
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(img.pixels) | img.pitch) & 15) == 0;   // uniform
    uint8_t* at = block_row(img, p, r) + 16 * half;
    if (p.cols == 4 && p.rows == 4) {
        if (aligned16)
            store_streaming16(at, v);
        else
            *reinterpret_cast<u32x4_align8*>(at) = v;
    } else if ((uint32_t)r < p.rows) {
        u32x2* px = reinterpret_cast<u32x2*>(at);
        if ((uint32_t)(2 * half) < p.cols)
            px[0] = u32x2{v.x, v.y};
        if ((uint32_t)(2 * half + 1) < p.cols)
            px[1] = u32x2{v.z, v.w};
    }
}

template <bool TAIL>
struct Bc6hPixelSink {
    static constexpr bool kStaged = true;
    static constexpr int kParts = 4;              // one pixel row per part
    static constexpr int kStageBytes = kT * 32;
    using Held = Interp;
    ImageSink img;
    uint64_t first_block, blocks;

    __device__ __forceinline__ Held hold(const B128& b) const { return prepare_bc6h_block(b); }

    __device__ __forceinline__ void stage(uint8_t* lds, int j, const Held& h, int part) const
    {
        uint32_t o[8];
        row_pixels(h, part, o);
        granule::lds_at<u32x4>(lds, 32 * j) = u32x4{o[0], o[1], o[2], o[3]};
        granule::lds_at<u32x4>(lds, 32 * j + 16) = u32x4{o[4], o[5], o[6], o[7]};
    }

    __device__ __forceinline__ void store_staged(uint8_t* lds, uint64_t b, int pos, int part) const
    {
        if constexpr (!TAIL) {
            // every lane of the wave is here; a granule starts at a multiple of 1024 blocks, so the lane is b's low six bits
            const int lane = (int)(b & 63u);
            const uint64_t run_first = b - (uint64_t)lane;
            const int pos_lo = __builtin_amdgcn_ds_bpermute((lane >> 1) * 4, pos);
            const int pos_hi = __builtin_amdgcn_ds_bpermute((32 + (lane >> 1)) * 4, pos);
            const int half = lane & 1;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const uint64_t at = run_first + (uint64_t)(32 * q + (lane >> 1)) - first_block;   // wraps below first_block
                if (at < blocks)
                    store_half_row(img, place_block<8>(img, at), part, half,
                                   granule::lds_at<u32x4>(lds, 32 * (q ? pos_hi : pos_lo) + 16 * half));
            }
        } else {
            const uint64_t at = b - first_block;   // wraps for b < first_block
            if (at >= blocks)
                return;
            const u32x4 row[2] = {granule::lds_at<u32x4>(lds, 32 * pos), granule::lds_at<u32x4>(lds, 32 * pos + 16)};
            store_block_row(img, place_block<8>(img, at), part, row);
        }
    }
};

// ---- the same sink for the images of a region table ----------------------------------------------------------------------
// hold() and stage() are Bc6hPixelSink's: the blocks are prepared in the sorted domain and one pixel row per part crosses through
// LDS exactly as for one image.  store_staged() differs in who owns a block: block `b` of the buffer belongs to whichever region
// of `tab` holds it, and to none in a gap.  Three questions, the cheapest first, as in Bc7RegionPixelSinkOf (bc7_image_sinks.h):
// prepare() asks once per granule (or tail part), before the decode, whether ONE region holds all of it -- its answer stays in
// scalar registers, serves every store of the granule, and the stores are then the single-image sink's, the uniform `sc1 nt`-or-
// plain choice included; otherwise the wave asks about its run of 64 (wave_run, image_region_sinks.h); otherwise the lanes ask
// region_of_block, and the image, the store choice and the clipping are per lane.  The wave's and the lanes' answers are looked up
// again for each of the four parts instead of being held across them: an ImageSink and a block number per stored block would
// otherwise live through the next part's stage() beside the 36 registers of the held blocks.
// What differs from BC7 is whose block a lane stores.  In a full granule lane l does not store the block it holds but halves
// l & 1 of blocks l / 2 and 32 + l / 2 of its wave's run, after two cross-lane moves.  So
//   * all 64 lanes take part in both moves before any lane finds that a block has no image: a block without one only skips its
//     stores, and no lane leaves before a barrier of inverse_granule;
//   * the ownership question is asked about the block a lane STORES, run_first + 32 q + l / 2, not about `b`, the block it holds.
// TAIL, one workgroup: every lane fetches its own block's row, so the wave and then the lane ask about `b` itself, as the BC7
// sink does; the tail part's last, partly filled wave reaches past the buffer's end and takes the per-lane path.
// Written once for every kind of table the lookups of image_regions.h take.
template <typename TABLE, bool TAIL>
struct Bc6hRegionPixelSinkOf {
    using One = Bc6hPixelSink<TAIL>;
    static constexpr bool kStaged = One::kStaged;
    static constexpr int kParts = One::kParts;
    static constexpr int kStageBytes = One::kStageBytes;
    using Held = typename One::Held;
    TABLE tab;

    // (the single-image sink's members do not read its fields)
    __device__ __forceinline__ Held hold(const B128& b) const { return One{}.hold(b); }
    __device__ __forceinline__ void stage(uint8_t* lds, int j, const Held& h, int part) const { One{}.stage(lds, j, h, part); }

    // the region that holds the whole granule (tail part), if one does: most granules of a large image
    using Prepared = WaveRun;
    __device__ __forceinline__ Prepared prepare(uint64_t first, uint64_t n) const { return wave_run(tab, first, n); }

    // full granules: half `half` of pixel row `part` of block `local` of `img`, staged at sorted position `pos`
    __device__ __forceinline__ void fetch_and_store_half(uint8_t* lds, const ImageSink& img, uint64_t local, int pos, int part, int half) const
    {
        store_half_row(img, place_block<8>(img, local), part, half, granule::lds_at<u32x4>(lds, 32 * pos + 16 * half));
    }

    // TAIL: pixel row `part` of block `local` of `img`
    __device__ __forceinline__ void fetch_and_store_row(uint8_t* lds, const ImageSink& img, uint64_t local, int pos, int part) const
    {
        const u32x4 row[2] = {granule::lds_at<u32x4>(lds, 32 * pos), granule::lds_at<u32x4>(lds, 32 * pos + 16)};
        store_block_row(img, place_block<8>(img, local), part, row);
    }

    __device__ __forceinline__ void store_staged(uint8_t* lds, uint64_t b, int pos, int part, const Prepared& whole) const
    {
        static_assert(kT % 64 == 0, "a wave's 64 blocks start at a multiple of 64");
        if constexpr (!TAIL) {
            // every lane of the wave is here; a granule starts at a multiple of 1024 blocks, so the lane is b's low six bits and the
            // wave's first block is b with them cleared
            const int lane = (int)(b & 63u);
            const uint64_t run_first = b & ~(uint64_t)63;
            const int mine = lane >> 1, half = lane & 1;   // the lane stores halves `half` of blocks mine and 32 + mine of the run
            const int pos_lo = __builtin_amdgcn_ds_bpermute(mine * 4, pos);
            const int pos_hi = __builtin_amdgcn_ds_bpermute((32 + mine) * 4, pos);
            if (whole.region >= 0) {
                const uint64_t local = whole.local + (run_first - whole.first) + (uint64_t)mine;
                fetch_and_store_half(lds, whole.img, local, pos_lo, part, half);
                fetch_and_store_half(lds, whole.img, local + 32, pos_hi, part, half);
                return;
            }
            const WaveRun run = wave_run(tab, run_first, 64);
            if (run.region >= 0) {
                fetch_and_store_half(lds, run.img, run.local + (uint64_t)mine, pos_lo, part, half);
                fetch_and_store_half(lds, run.img, run.local + (uint64_t)(32 + mine), pos_hi, part, half);
            } else {
                DXTLT_REGIONS_LOOP
                for (int q = 0; q < 2; ++q) {
                    ImageSink img{nullptr, 0, 1, 0, 0, 8};
                    uint64_t local = 0;
                    if (region_of_block(tab, run_first + (uint64_t)(32 * q + mine), img, local) >= 0)
                        fetch_and_store_half(lds, img, local, q ? pos_hi : pos_lo, part, half);
                }
            }
        } else {
            if (whole.region >= 0) {
                fetch_and_store_row(lds, whole.img, whole.local + (b - whole.first), pos, part);
                return;
            }
            const WaveRun run = wave_run(tab, b & ~(uint64_t)63, 64);
            if (run.region >= 0) {
                fetch_and_store_row(lds, run.img, run.local + (b & 63), pos, part);
            } else {
                ImageSink img{nullptr, 0, 1, 0, 0, 8};
                uint64_t local = 0;
                if (region_of_block(tab, b, img, local) >= 0)
                    fetch_and_store_row(lds, img, local, pos, part);
            }
        }
    }
};

}  // namespace

// BC6H as the kernels and launchers of granule_image.h see it: the family of RGBA16F images
struct Bc6hImage {
    using Codec = Bc6hCodec;
    template <bool TAIL>
    using Sink = Bc6hPixelSink<TAIL>;
    template <typename TABLE, bool TAIL>
    using RegionSink = Bc6hRegionPixelSinkOf<TABLE, TAIL>;
    static constexpr uint32_t kBpp = 8;
    // the plain decoders: a block's prepared endpoints and indices, interpolated and stored a pixel row at a time -- plain stores,
    // never `sc1 nt` (store_block_row says why)
    using Decoded = Interp;
    static __device__ __forceinline__ void decode(u32x4 q, Decoded& s) { s = prepare_q(q); }
    static __device__ __forceinline__ void store(const ImageSink& img, uint64_t b, const Decoded& s) { store_block_pixels(img, b, s); }
};

}  // namespace bc6h
}  // namespace dxtlt
