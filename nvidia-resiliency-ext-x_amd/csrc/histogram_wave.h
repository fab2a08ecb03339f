// histogram_wave.h -- what the histogram score kernels share (histogram_scores.hip: a rank against
// the fleet; histogram_history.hip: a rank against its own history): the bucket weight, the u64
// DPP reduction and inclusive prefix over a wave.
#pragma once
#include "nvrx_common.h"
#include "nvrx_internal.h"

namespace nvrx {
namespace {

constexpr int HB = NVRX_HIST_BINS;
constexpr int HV = HB / 4;  // 16-byte vectors per histogram
static_assert(HB % 4 == 0 && HV <= NVRX_WAVE, "a histogram is at most one vector per lane");

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// w(b): the lower edge of bucket min(b, 238) as a duration key (both wide buckets weigh
// NVRX_KEY_WIDE)
__device__ __forceinline__ unsigned weight_of(int b) {
    b = min(b, HB - 2);
    return b < 8 ? (unsigned)b : (8u + ((unsigned)b & 7u)) << ((b >> 3) - 1);
}

template <int CTRL>
__device__ __forceinline__ u64 dpp_u64(u64 x) {
    const unsigned lo = dpp<CTRL>((unsigned)x), hi = dpp<CTRL>((unsigned)(x >> 32));
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 rl_u64(u64 x, int l) {
    return ((u64)rl((unsigned)(x >> 32), l) << 32) | rl((unsigned)x, l);
}
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
    v += dpp_u64<0xB1>(v);
    v += dpp_u64<0x4E>(v);
    v += dpp_u64<0x141>(v);
    v += dpp_u64<0x140>(v);
    return (rl_u64(v, 0) + rl_u64(v, 16)) + (rl_u64(v, 32) + rl_u64(v, 48));
}
// inclusive prefix over the 64 lanes, as wave_incl_scan_u32
__device__ __forceinline__ u64 wave_incl_scan_u64(u64 v) {
    v += dpp_u64<0x111>(v);
    v += dpp_u64<0x112>(v);
    v += dpp_u64<0x114>(v);
    v += dpp_u64<0x118>(v);
    const int l = lane_id();
    const u64 r0 = rl_u64(v, 15), r1 = rl_u64(v, 31), r2 = rl_u64(v, 47);
    v += (l >= 16 ? r0 : 0ull) + (l >= 32 ? r1 : 0ull) + (l >= 48 ? r2 : 0ull);
    return v;
}

}  // namespace
}  // namespace nvrx
