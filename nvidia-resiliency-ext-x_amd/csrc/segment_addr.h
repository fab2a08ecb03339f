// segment_addr.h -- where a segment lies in memory (strided, ragged), what a launch over such
// segments has to be sized for, the fused column reference and the empty result: what every
// segment kernel takes as arguments.
#pragma once
#include "nvrx_common.h"
#include "nvrx_internal.h"

namespace nvrx {

struct StridedSegs {  // segment s = base[s*stride + begin : + len], last `cap` kept
    const uint32_t* base;
    int64_t stride, begin, len, cap;
    __device__ __forceinline__ void get(int64_t s, const uint32_t*& p, int& n) const {
        int64_t keep = (cap > 0 && len > cap) ? cap : len;
        p = base + s * stride + begin + (len - keep);
        n = (int)keep;
    }
};
struct RaggedSegs {  // segment s = base[off[s] : off[s] + len[s]] (len NULL: off[s+1]), last `cap` kept;
                     // len[s] < 0: skipped (already reduced, e.g. by records_stats)
    const uint32_t* base;
    const int64_t* off;
    const int32_t* lens;
    int64_t cap;
    __device__ __forceinline__ void get(int64_t s, const uint32_t*& p, int& n) const {
        const int64_t b = off[s];
        const int64_t e = lens ? b + lens[s] : off[s + 1];
        const int64_t len = e - b;
        int64_t keep = (cap > 0 && len > cap) ? cap : len;
        p = base + (e - keep);
        n = (int)keep;
    }
    // the retained length alone (no offset load when `lens` is given)
    __device__ __forceinline__ int kept_len(int64_t s) const {
        const int64_t len = lens ? (int64_t)lens[s] : off[s + 1] - off[s];
        return (int)((cap > 0 && len > cap) ? cap : len);
    }
};

// The sample loads of the tail kernels that sort a wave's 64 ragged segments into two treatments
// (segment_tail.hip, segment_tail_attribution.hip): a retained run <= ST_LANE_MAX is walked by the
// lane that holds it, a longer one by the whole wave.
constexpr int ST_LANE_MAX = 16;  // the longest retained run a lane walks alone
constexpr int ST_UNROLL = 4;     // loads in flight per lane

__device__ __forceinline__ const uint32_t* rl_ptr(const uint32_t* p, int l) {
    const uint64_t b = (uint64_t)(uintptr_t)p;
    return (const uint32_t*)(uintptr_t)(((uint64_t)rl((unsigned)(b >> 32), l) << 32) | rl((unsigned)b, l));
}
// samples [base, base + 64 ST_UNROLL) of a segment of m, 64 consecutive ones per load; a lane past
// the end re-reads the last sample (its slot is then masked by the caller)
__device__ __forceinline__ void wave_load(const uint32_t* q, int m, int base, unsigned (&x)[ST_UNROLL]) {
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u)
        x[u] = __builtin_nontemporal_load(q + min(base + u * 64 + lane_id(), m - 1));
}
// samples [i, i + ST_UNROLL) of a lane's own segment of n
__device__ __forceinline__ void lane_load(const uint32_t* p, int n, int i, unsigned (&x)[ST_UNROLL]) {
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) x[u] = p[min(i + u, n - 1)];
}

// need = retained length + offset in the first 16-byte vector: what a wave has to hold
__device__ __forceinline__ int seg_need(const uint32_t* p, int n) {
    return n + (int)(((uintptr_t)p & 15) >> 2);
}

// Host side, before a launch: keep = the longest retained length, [need_lo, need_hi] = the range
// every segment's need lies in, aligned = every retained run starts on a 16-byte boundary.
struct SegRange {
    int64_t keep, need_lo, need_hi;
    bool aligned;
};
inline int64_t seg_keep(int64_t len, int64_t cap) { return (cap > 0 && len > cap) ? cap : len; }
// every strided segment has the same length and phase
inline SegRange seg_range(const StridedSegs& g) {
    const int64_t keep = seg_keep(g.len, g.cap);
    const bool aligned = ((g.stride % 4) == 0) &&
                         ((((uintptr_t)(g.base + g.begin + (g.len - keep))) & 15) == 0);
    return {keep, keep, aligned ? keep : keep + 3, aligned};
}
// ragged segments of at most max_len samples; aligned16: the caller's word for every run
inline SegRange seg_range(const RaggedSegs& g, int64_t max_len, bool aligned16) {
    const int64_t keep = seg_keep(max_len, g.cap);
    return {keep, 0, aligned16 ? keep : keep + 3, aligned16};
}

// Optional fused per-column reference (segment s = row s / ncols, column s % ncols):
// minbits[c] = atomicMin of the float bits of MED (non-negative floats order like their
// bit patterns), missing[c] |= 1 for an empty segment -- _all_reduce_times'
// MIN-over-ranks with the -1 => NaN rule (reporting.py:255-296), done in the epilogue.
struct ColRef {
    uint32_t* minbits;
    uint32_t* missing;
    int64_t ncols;
    double inv;  // 1.0 / ncols
    // no column reference: add / miss do nothing
    static constexpr __host__ __device__ ColRef none() { return ColRef{nullptr, nullptr, 1, 1.0}; }
    // s % ncols without a 64-bit integer divide: the f64 quotient is off by at most one
    // for s < 2^52
    __device__ __forceinline__ int64_t col(int64_t s) const {
        int64_t q = (int64_t)((double)s * inv);
        int64_t r = s - q * ncols;
        if (r < 0) r += ncols;
        if (r >= ncols) r -= ncols;
        return r;
    }
    __device__ __forceinline__ void add(int64_t s, float med) const {
        if (minbits) atomicMin(&minbits[col(s)], __float_as_uint(med));
    }
    __device__ __forceinline__ void miss(int64_t s) const {
        if (minbits) atomicOr(&missing[col(s)], 1u);
    }
};

__device__ __forceinline__ void write_empty(const nvrx_stats_soa& o, int64_t s) {
    // KernelStats() default: num_calls 0, every float NaN (CuptiProfiler.h:39-45)
    const float q = __builtin_nanf("");
    o.num[s] = 0;
    o.min[s] = q;
    o.max[s] = q;
    o.med[s] = q;
    o.avg[s] = q;
    o.std[s] = q;
}

}  // namespace nvrx
