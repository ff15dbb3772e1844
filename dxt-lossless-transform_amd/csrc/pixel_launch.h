// pixel_launch.h -- internal launch interface between the C ABI layer (pixels_api.cpp) and the uncompressed-pixel kernels
// (pixel_kernels.hip): RGBA8888 / BGRA8888 (4 bytes per pixel) and BGR888 (3), docs/PIXEL_FORMAT.md layout version 1.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace dxtlt {
namespace pixels {

constexpr uint64_t kTile = 4096;   // pixels per workgroup = bytes per plane segment (DXTLT_PIXEL_SEGMENT)
enum Layout : int { kInterleaved = 0, kPlanar = 1, kPlanarDelta = 2 };

// Pixels [first, first + num) of a buffer of `total` pixels of `pixel_bytes` (3 or 4) bytes.  The interleaved-side pointer is
// the range's first pixel, the transformed-side pointer byte 0 of the whole transformed buffer; forward reads the former
// and writes the latter, inverse the other way round.  `first` is a multiple of kTile.  Enqueues on `stream`;
// hipErrorInvalidValue for arguments the kernels do not take (checked by the caller first), else the launch's error.
hipError_t launch_range(int pixel_bytes, bool inverse, bool decorrelate, int layout, const void* src, void* dst, uint64_t total,
                        uint64_t first, uint64_t num, hipStream_t stream);

// The fused candidate kernel of the pixel auto transform (pixel_auto_kernels.hip): from the `total` pixels at `src` (on a 16-byte
// boundary) the forward transform with (decorrelate, PLANAR_DELTA), (decorrelate, PLANAR), (decorrelate, INTERLEAVED),
// (plain, PLANAR_DELTA) and (plain, PLANAR), in this order, at arena + i * total * pixel_bytes.  Enqueues on `stream`.
hipError_t launch_auto_candidates(int pixel_bytes, const void* src, void* arena, uint64_t total, hipStream_t stream);

// The six candidates of the pixel auto transforms (include/dxtlt_pixels.h, "the auto transform") in the order they are compared:
// the five above, then the input itself.
struct AutoCandidate {
    bool decorrelate;
    uint8_t layout;
};
constexpr int kAutoCandidates = 6;
constexpr AutoCandidate kAutoOrder[kAutoCandidates] = {{true, 2}, {true, 1}, {true, 0}, {false, 2}, {false, 1}, {false, 0}};
// the first smallest total: from the first candidate with best = UINT64_MAX, replaced on strict `<`
inline int auto_pick_of(const uint64_t* totals)
{
    int pick = 0;
    uint64_t best = UINT64_MAX;
    for (int i = 0; i < kAutoCandidates; ++i)
        if (totals[i] < best) {
            best = totals[i];
            pick = i;
        }
    return pick;
}

}  // namespace pixels
}  // namespace dxtlt
