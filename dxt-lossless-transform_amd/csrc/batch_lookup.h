// batch_lookup.h -- from a workgroup of a batch launch to its table entry and to the tile of the entry it runs: the lookup of
// batch_kernel (batch_kernels.hip: blocks in, blocks out) and of the batch image kernels (image_batch_kernels.hip: transformed
// blocks in, pixels out), written once.  Device code.
//
// An ENTRY is a table record whose dword 7 is `end_wg` (BatchEntry, bcn_launch.h, and every record laid out like its first 48
// bytes); load_batch_entry(const ENTRY*) hands back the VIEW of it in scalar registers -- with first_wg and end_wg among its
// members -- and pin_batch_view(VIEW&) makes every field of the view needed at once.  The index is build_batch_index's.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dxtlt {

// The entry that owns workgroup `wg`, loaded into `en`; returns its index in the launch.  n_base: batch_index_base_count of
// the launch, bit 31 = the wide form of the index; n_entries: the bound of the bisection.
template <typename ENTRY, typename VIEW>
__device__ __forceinline__ uint32_t batch_entry_of_workgroup(const ENTRY* entries, const uint8_t* index, uint32_t n_base,
                                                             uint32_t n_entries, uint32_t wg, VIEW& en)
{
    // base[wg / 4096] + delta[wg / 64] = the entry that owns workgroup 64 * (wg / 64) (bcn_launch.h); an entry carries its own
    // end, so a workgroup of a buffer of 64 workgroups or more is two dependent table loads away from its tile (three scalar
    // round trips with the kernel arguments).  What was measured on the way here (profiles/r04_batch_edge_tiles.txt; one
    // 2 GiB odd-count buffer or the corpus, forward): no table load 0.80, ONE load of an entry that thousands of workgroups
    // share 0.80 -- a scalar-cache hit costs next to nothing -- but an index record that every workgroup of a CU sees for the
    // first time 0.72-0.76 whatever it saves in round trips (a 144-byte record per 256 workgroups with the entry inline:
    // 0.72; a 16-byte bit mask per 64: 0.76; 4 bytes per 64: 0.77).  So the index is as small as it can be -- one byte per 64
    // workgroups, a cache line per 4096 -- and the entry, shared by all workgroups of its buffer, is what is fetched behind it.
    // Wide form (bit 31 of n_base; build_batch_index): 16-bit deltas, for launches in which more than 255 entries begin inside
    // one 4096-workgroup span -- thousands of buffers of one to three tiles -- where a byte would saturate and leave a walk of
    // up to ~3800 entries.  Branch-free on purpose: both forms issue the same two index loads.
    static_assert(offsetof(ENTRY, end_wg) == 28, "the bisection reads end_wg as dword 7 of an entry");
    const uint32_t* base = reinterpret_cast<const uint32_t*>(index);
    const uint32_t wide = n_base >> 31;
    const uint8_t* delta = index + (n_base & 0x7FFFFFFFu) * 4;
    uint32_t e = base[wg >> 12];
    const uint32_t dword = reinterpret_cast<const uint32_t*>(delta)[wg >> (8u - wide)];   // (a scalar load is a dword load)
    e += (dword >> (((wg >> 6) & (3u >> wide)) << (3u + wide))) & (0xFFu | (wide * 0xFF00u));
    en = load_batch_entry(entries + e);
    // every field is needed HERE (empty non-volatile asm: the value becomes opaque, memory is untouched, the loads stay
    // scalar): left alone the compiler fetches end_wg, runs the search and only then asks for the rest of the entry
    pin_batch_view(en);
    if (en.end_wg <= wg) {
        // Only buffers of fewer than 64 workgroups take this: `e` owns workgroup 64 * (wg / 64), so the owner of `wg` is one of
        // the next (wg & 63) entries.  Bisection over their end_wg fields -- at most six dependent dword loads, where walking
        // on entry by entry took up to 63 loads of a whole entry.
        uint32_t lo = e + 1, hi = e + (wg & 63u);
        hi = hi < n_entries - 1u ? hi : n_entries - 1u;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            const uint32_t end = reinterpret_cast<const uint32_t*>(entries + mid)[7];   // end_wg
            // (two selects, spelled as such: batch_kernels.hip then compiles to the instruction streams it had with the search in place)
            lo = end <= wg ? mid + 1 : lo;
            hi = end <= wg ? hi : mid;
        }
        e = lo;
        en = load_batch_entry(entries + e);
    }
    return e;
}

// Which of its entry's tiles workgroup `wg` takes: the entry's tiles rotated over the eight XCDs so that entry e's last tile -- the
// edge tile, 1.2-1.9 x a whole tile's time -- runs on XCD e % 8 and not on the same XCD for every entry.  batch_kernel
// (batch_kernels.hip) has the measurements and spells the same six lines out in place: as a call the compiler orders two of its
// scalar instructions the other way round, and that file's instruction streams are kept as they were.
__device__ __forceinline__ uint32_t batch_rotated_tile(uint32_t first_wg, uint32_t end_wg, uint32_t e, uint32_t wg)
{
    const uint32_t n_wgs = end_wg - first_wg;
    uint32_t local = wg - first_wg;
    if (n_wgs >= 8) {
        local += (first_wg + n_wgs - 1u - e) & 7u;
        local = local >= n_wgs ? local - n_wgs : local;
    }
    return local;
}

}  // namespace dxtlt
