// pixel_batch_api.h -- what pixel_batch_api.cpp offers the batched pixel auto call (pixel_batch_auto_api.cpp): a planned pixel
// batch on its way to the device.  Host only.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "pixel_batch_plan.h"

namespace dxtlt_host {

// Stages the plan's tables in one slot of the calling thread's table ring, uploads them on `stream` and launches every class of
// the plan behind them; enqueues only.  A status of host_common.h, the error text recorded.  The stream is not capturing.
int32_t pixel_batch_enqueue(const pixel_batch::Plan& plan, hipStream_t stream);

}  // namespace dxtlt_host
