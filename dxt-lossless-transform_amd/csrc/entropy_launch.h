// entropy_launch.h -- internal interface of the entropy estimator (entropy_kernels.hip), "The entropy estimator, version 1" of
// docs/ESTIMATOR.md: per 32 KiB window of n bytes with byte counts c[v], q = max(0, n T[n] - sum c[v] T[c[v]]) in 1/65536 bit,
// T[k] = floor(2^16 log2 k); estimate = (sum of q over the section's windows + 2^19 - 1) >> 19 bytes.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "estimate_launch.h"

namespace dxtlt {

constexpr uint32_t kEntropyEstimatorVersion = 1;
constexpr uint32_t kEntropyWindow = kEstimatorWindow;   // the windows the gram estimator cuts
constexpr uint32_t kEntropyShift = 19;                  // 1/65536 bit -> bytes

// d_out[i] = entropy estimate of sections[i], i < count (NULL or empty: 0).  Zeroes the counters on `stream`, one launch per 16
// sections that adds every window's q into its section's counter, then one finishing launch that rounds the sums up to bytes
// in place.  Enqueues only.  hipErrorInvalidValue: a section of more than 2^31 - 1 windows.
hipError_t launch_entropy(const EstimateSection* sections, size_t count, uint64_t* d_out, hipStream_t stream);

// The q sums of any number of sections in ONE launch, the twin of launch_estimate_table (estimate_launch.h): `d_table` (device
// memory, `entries` entries in workgroup order, each with len > 0 and one workgroup per 32 KiB window) and `workgroups` = the last
// entry's end_wg (at most 2^31 - 1: hipErrorInvalidValue beyond).  ADDS every window's q into d_counters[entry.counter], which
// the caller has zeroed on `stream`; several entries may share a counter.  The counters then hold sums of q, not bytes:
// launch_entropy_finish rounds `count` of them up to bytes in place, (sum + 2^19 - 1) >> 19.  Both enqueue only.
hipError_t launch_entropy_table(const EstimateTableEntry* d_table, uint32_t entries, uint32_t workgroups, uint64_t* d_counters,
                                hipStream_t stream);
hipError_t launch_entropy_finish(uint64_t* d_counters, size_t count, hipStream_t stream);

// T[k] on the host, k <= 32768 (0 beyond): the table the kernels read, for the tests.
uint32_t entropy_table_host(uint32_t k);

}  // namespace dxtlt
