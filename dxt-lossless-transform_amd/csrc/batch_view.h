// batch_view.h -- a BatchEntry (bcn_launch.h) as a workgroup of a tile batch launch sees it: shared by batch_kernel
// (batch_kernels.hip) and batch_norm_kernel (batch_norm_kernels.hip).  Device code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bcn_device.h"

namespace dxtlt {

// A table entry as the workgroup sees it: everything arrives through scalar (dword) loads -- byte fields read one by
// one would go through the vector memory path and add a second round trip before the tile's own load can start --
// and the buffer pointers are tagged as global memory again (a pointer that was loaded from memory is a generic one
// to the compiler, which would turn every access of the tile into a flat_* instruction).
struct BatchView {
    const uint8_t* src;
    uint8_t* dst;
    uint64_t blocks;
    uint32_t first_wg, end_wg, full_tiles;
    uint32_t flags;       // form | halo_vecs << 8 | natural << 16 | reserved << 24 (batch_norm_kernel: the entry's normalisation modes)
    uint32_t shifts[2];   // shift[0..3], shift[4..5]
    uint64_t gbase[6];
};

__device__ __forceinline__ BatchView load_batch_entry(const BatchEntry* entry)
{
    const uint64_t* q = reinterpret_cast<const uint64_t*>(entry);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(entry);
    BatchView v;
    v.src = (const uint8_t*)(global_cptr)q[0];
    v.dst = (uint8_t*)(global_ptr)q[1];
    v.blocks = q[2];
    v.first_wg = w[6];
    v.end_wg = w[7];
    v.full_tiles = w[8];
    v.flags = w[9];
    v.shifts[0] = w[10];
    v.shifts[1] = w[11];
#pragma unroll
    for (int i = 0; i < 6; ++i)
        v.gbase[i] = q[6 + i];
    return v;
}
__device__ __forceinline__ void pin_batch_view(BatchView& v)
{
    uint64_t s = reinterpret_cast<uintptr_t>(v.src), d = reinterpret_cast<uintptr_t>(v.dst);
    asm("" : "+s"(s), "+s"(d), "+s"(v.blocks));
    v.src = (const uint8_t*)(global_cptr)s;
    v.dst = (uint8_t*)(global_ptr)d;
    asm("" : "+s"(v.first_wg), "+s"(v.end_wg), "+s"(v.full_tiles), "+s"(v.flags), "+s"(v.shifts[0]), "+s"(v.shifts[1]));
#pragma unroll
    for (int i = 0; i < 6; ++i)
        asm("" : "+s"(v.gbase[i]));
}
static_assert(offsetof(BatchEntry, first_wg) == 24 && offsetof(BatchEntry, end_wg) == 28 && offsetof(BatchEntry, full_tiles) == 32 && offsetof(BatchEntry, form) == 36 &&
                  offsetof(BatchEntry, reserved) == 39 && offsetof(BatchEntry, shift) == 40 && offsetof(BatchEntry, gbase) == 48,
              "load_batch_entry reads BatchEntry by dword offsets");

constexpr uint32_t kBatchAligned = 1;   // BatchEntry::form

}  // namespace dxtlt
