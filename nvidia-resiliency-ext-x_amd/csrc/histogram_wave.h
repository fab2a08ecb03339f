// histogram_wave.h -- what the histogram and tail-score kernels share: the bucket of a duration key
// and its weight, the u64 DPP reduction and inclusive prefix over a wave, and the one copy of what
// the tail-score family repeats -- a lane's four bins, the saturating add, the wave's LDS count,
// the slot of a column, the loss (`excess`), and the clear and finalize kernels of a score.
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

// bucket(x) of a duration key, as segment_histogram.hip's header derives it: sh = e - 3 for
// x >= 8, 0 below
__device__ __forceinline__ unsigned bucket_of(unsigned x) {
    const unsigned sh = 28u - (unsigned)__builtin_clz(x | 8u);
    return (sh << 3) + (x >> sh);
}

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

// a lane's four bins and their weights: constants of the launch
struct LaneBins {
    int b0;
    unsigned w0, w1, w2, w3;
};
__device__ __forceinline__ LaneBins lane_bins(int lane) {
    const int b0 = 4 * lane;
    return {b0, weight_of(b0), weight_of(b0 + 1), weight_of(b0 + 2), weight_of(b0 + 3)};
}

__device__ __forceinline__ unsigned sat_add(unsigned h, unsigned c) {
    const unsigned s = h + c;
    return s < h ? 0xFFFFFFFFu : s;  // min(h + c, 2^32 - 1) of the 64-bit sum
}

// 64 buckets, one per lane (NONE: no sample), into the bins h in LDS: the bucket of the first live
// lane is counted with one ballot + population count and one LDS add, twice; only the lanes left
// add on their own
template <unsigned NONE>
__device__ __forceinline__ void count_wave(unsigned b, unsigned* h) {
    uint64_t live = __ballot(b != NONE);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (!live) return;  // wave-uniform
        const int l = __builtin_ctzll(live);
        const unsigned lead = rl(b, l);
        const uint64_t same = __ballot(b == lead);
        if (lane_id() == l) atomicAdd(&h[lead], (unsigned)__popcll(same));
        live &= ~same;
    }
    if ((live >> lane_id()) & 1) atomicAdd(&h[b], 1u);
}

// a lane's integer sums over samples against the threshold bucket t; CALLS adds the count above it
template <bool CALLS>
struct TailAcc {
    u64 total = 0, tail = 0;
    unsigned calls = 0;
    __device__ __forceinline__ void add(unsigned x, int t) {
        const int b = (int)bucket_of(x);
        const u64 w = weight_of(b);
        const bool hit = b > t;
        total += w;
        tail += hit ? w : 0ull;
        if (CALLS) calls += hit;
    }
};

// history slot of column k (wave-uniform), -1 where the column is not eligible
template <typename Args>
__device__ __forceinline__ int64_t slot_of(const Args& a, int64_t k) {
    int64_t s = a.hist_index ? (int64_t)a.hist_index[k] : k;
    if (a.col_valid && !a.col_valid[k]) s = -1;
    return s;
}

// the three f64 operations of a loss, each rounded separately (-ffp-contract=off): the loss and
// the select kernel of an attribution both call it, so a winner's stored loss is the loss that
// ranked it
__device__ __forceinline__ double excess(u64 tail, u64 total, u64 btail, u64 btotal, double& share) {
    share = (double)btail / (double)btotal;
    return (double)tail - (double)total * share;
}

// the four u64 row sums of an individual score, cleared on the stream before the pass adds to
// them (templates, so that only the files that launch them carry them)
template <typename T>
__global__ __launch_bounds__(256) void clear4_kernel(T* a, T* b, T* c, T* d, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        a[i] = 0;
        b[i] = 0;
        c[i] = 0;
        d[i] = 0;
    }
}
// the same with the compact history's folded count: a null (SCORE) / folded null (UPDATE) is skipped
template <typename T>
__global__ __launch_bounds__(256)
void clear4_folded_kernel(T* a, T* b, T* c, T* d, T* folded, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (a) {  // SCORE
        a[i] = 0;
        b[i] = 0;
        c[i] = 0;
        d[i] = 0;
    }
    if (folded) folded[i] = 0;  // UPDATE
}

// per row the three separately rounded f64 operations of an individual score, and strag
template <typename Args>
__global__ __launch_bounds__(256) void tail_score_finalize_kernel(Args a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.R) return;
    const u64 tl = a.tail_ns[r], tt = a.total_ns[r], bl = a.base_tail_ns[r], bt = a.base_total_ns[r];
    double score = __builtin_nan("");
    if (tt != 0 && bt != 0) {
        const double share = (double)tl / (double)tt;
        const double bs = (double)bl / (double)bt;
        const double den = 1.0 - bs;
        if (den != 0.0) score = (1.0 - share) / den;
    }
    a.score[r] = score;
    if (a.strag) a.strag[r] = score < a.score_thr;  // NaN compares false
}

}  // namespace
}  // namespace nvrx
