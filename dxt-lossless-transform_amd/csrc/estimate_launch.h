// estimate_launch.h -- internal interface of the device-resident size estimator (estimate_kernels.hip), version 1 of
// docs/ESTIMATOR.md: estimate = L - (positions whose 4-byte gram repeats the first gram of its hash slot, per 32 KiB window).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace dxtlt {

constexpr uint32_t kEstimatorVersion = 1;
constexpr uint32_t kEstimatorWindow = 32768;   // W
constexpr uint32_t kEstimatorBits = 14;        // BITS

struct EstimateSection {
    const void* d_ptr;   // any alignment; NULL estimates as `len`
    uint64_t len;
};

// d_out[i] = estimate of sections[i], i < count.  Zeroes the counters on `stream`, then one launch per 16 sections (the
// table travels in the kernel arguments: nothing of the caller's has to outlive the call).  Enqueues only.
// hipErrorInvalidValue: a section of more than 2^31 - 1 windows.
hipError_t launch_estimate(const EstimateSection* sections, size_t count, uint64_t* d_out, hipStream_t stream);

// One section of a table in device memory (launch_estimate_table): entries in workgroup order, entry e owning workgroups
// [end_wg of entry e - 1, end_wg) -- one per 32 KiB window, so an entry has len > 0 -- and adding into counters[counter].
struct EstimateTableEntry {
    const uint8_t* base;   // any alignment
    uint64_t len;
    uint32_t end_wg;
    uint32_t counter;
};
static_assert(sizeof(EstimateTableEntry) == 24, "EstimateTableEntry layout is shared between host and device");

// The estimates of any number of sections in ONE launch: `d_table` (device memory, `entries` entries) as above, `workgroups` =
// the last entry's end_wg (at most 2^31 - 1: hipErrorInvalidValue beyond).  Adds into d_counters, which the caller has zeroed on
// `stream`; several entries may share a counter.  Enqueues only.
hipError_t launch_estimate_table(const EstimateTableEntry* d_table, uint32_t entries, uint32_t workgroups, uint64_t* d_counters,
                                 hipStream_t stream);

// The same launch with `lanes` per workgroup (256, 512, 1024) and another (window, bits) pair -- (32768, 14), (32768, 13),
// (16384, 13), (8192, 12) are compiled; anything else: hipErrorInvalidValue.  For the shape sweep of tools/estimator_bench.py
// and the tests; only (32768, 14) is the product's estimator, and its result does not depend on `lanes`.
hipError_t launch_estimate_shape(const EstimateSection* sections, size_t count, uint64_t* d_out, hipStream_t stream, int lanes,
                                 uint32_t window, uint32_t bits);

}  // namespace dxtlt
