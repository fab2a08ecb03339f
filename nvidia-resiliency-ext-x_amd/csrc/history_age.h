// history_age.h -- the host entries of history_age.hip, called from abi.cpp after its checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nvrx {

// every count of chist[R][stride] (elements of NVRX_CHIST_BYTES) shifted right, the emptied
// entries evicted; evicted / full: u64 [R] or NULL
hipError_t compact_history_age(void* chist, int64_t R, int64_t stride, int shift, uint64_t* evicted,
                               uint64_t* full, hipStream_t st);
// every word of hist[R][stride][NVRX_HIST_BINS] shifted right
hipError_t histogram_history_age(uint32_t* hist, int64_t R, int64_t stride, int shift, hipStream_t st);

}  // namespace nvrx
