// estimate_sections.h -- the section table of the estimator launches, written once: how up to 16 sections travel in the kernel
// arguments of one launch, how a workgroup finds the 32 KiB window it owns, and how the host cuts a list of sections into such
// launches.  Shared by the gram estimator (estimate_kernels.hip) and the entropy estimator (entropy_kernels.hip): both run one
// workgroup per window and add into one 64-bit counter per section.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "estimate_launch.h"

namespace dxtlt {

constexpr int kSectionsPerLaunch = 16;

struct EstimateTable {
    const uint8_t* base[kSectionsPerLaunch];
    uint64_t len[kSectionsPerLaunch];
    uint32_t end_wg[kSectionsPerLaunch];   // section s owns workgroups [end_wg[s - 1], end_wg[s]); unused entries: 0xFFFFFFFF
    unsigned long long* out;               // the counter of section 0 of this launch
};

// The window of workgroup `wg`, declared into the kernel's scope: section `s` of the launch, `w` bytes (the last window of a section
// may be shorter than W) at byte `off` of the section at `base`, which has `len` bytes.  The section is the first whose end_wg is
// above wg (uniform: scalar compares and selects).  A macro, not a function: the gram kernel's code is pinned, and through an
// inlined function -- returning a struct, or writing through references -- hipcc loads the whole table first and the kernel comes
// out as other instructions; expanded in place the statements compile to the code they always did.
#define DXTLT_ESTIMATE_WINDOW_OF(W, tab, wg)                          \
    uint32_t s = 0, begin = 0;                                        \
    const uint8_t* base = (tab).base[0];                              \
    uint64_t len = (tab).len[0];                                      \
    _Pragma("unroll") for (int k = 0; k < kSectionsPerLaunch - 1; ++k) \
        if ((wg) >= (tab).end_wg[k]) {                                \
            s = k + 1;                                                \
            begin = (tab).end_wg[k];                                  \
            base = (tab).base[k + 1];                                 \
            len = (tab).len[k + 1];                                   \
        }                                                             \
    const uint64_t off = uint64_t((wg) - begin) * (W);                \
    const uint32_t w = len - off < (W) ? uint32_t(len - off) : (W)

// The same for a section table in DEVICE memory (EstimateTableEntry, estimate_launch.h: any number of entries in workgroup order):
// the entry is the first whose end_wg is above `wg`, found by bisection -- uniform: scalar loads and compares; the grid ends at the
// last end_wg.  Declares `base`, `len`, `off` and `w` as above and `out`, the entry's counter in `counters`.
#define DXTLT_ESTIMATE_TABLE_WINDOW_OF(W, tab, entries, counters, wg)            \
    uint32_t lo = 0, hi = (entries) - 1;                                          \
    while (lo < hi) {                                                             \
        const uint32_t mid = (lo + hi) >> 1;                                      \
        if ((tab)[mid].end_wg > (wg))                                             \
            hi = mid;                                                             \
        else                                                                      \
            lo = mid + 1;                                                         \
    }                                                                             \
    const uint32_t begin = lo == 0 ? 0u : (tab)[lo - 1].end_wg;                   \
    const uint8_t* base = (tab)[lo].base;                                         \
    const uint64_t len = (tab)[lo].len;                                           \
    unsigned long long* out = (counters) + (tab)[lo].counter;                     \
    const uint64_t off = uint64_t((wg) - begin) * (W);                            \
    const uint32_t w = len - off < (W) ? uint32_t(len - off) : (W)

// d_out[i] receives the sum section i's windows add, i < count: zeroes the counters on `stream`, then calls
// launch(grid, table) once per 16 sections (fewer where a launch would pass 2^31 - 1 workgroups; a launch of no windows is
// skipped).  hipErrorInvalidValue, before anything is enqueued: a section of more than 2^31 - 1 windows.
template <uint32_t W, class Launch>
hipError_t launch_per_section_table(const EstimateSection* sections, size_t count, uint64_t* d_out, hipStream_t stream, Launch launch)
{
    if (count == 0)
        return hipSuccess;
    for (size_t i = 0; i < count; ++i)
        if ((sections[i].len + W - 1) / W > 0x7FFFFFFFu)   // more windows than one launch has workgroups
            return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_out, 0, count * sizeof(uint64_t), stream);
    for (size_t at = 0; at < count && e == hipSuccess;) {
        EstimateTable tab;
        for (int k = 0; k < kSectionsPerLaunch; ++k) {
            tab.base[k] = nullptr;
            tab.len[k] = 0;
            tab.end_wg[k] = 0xFFFFFFFFu;
        }
        uint64_t wgs = 0;
        int n = 0;
        while (at + n < count && n < kSectionsPerLaunch) {
            const uint64_t windows = (sections[at + n].len + W - 1) / W;
            if (n > 0 && wgs + windows > 0x7FFFFFFFu)
                break;   // the next launch takes it (the first section of a launch fits: checked above)
            wgs += windows;
            tab.base[n] = static_cast<const uint8_t*>(sections[at + n].d_ptr);
            tab.len[n] = sections[at + n].len;
            tab.end_wg[n] = uint32_t(wgs);
            ++n;
        }
        tab.out = reinterpret_cast<unsigned long long*>(d_out + at);
        if (wgs != 0) {
            launch(dim3{uint32_t(wgs)}, tab);
            e = hipGetLastError();
        }
        at += n;
    }
    return e;
}

}  // namespace dxtlt
