// nvrx_common.h -- shared device helpers for the gfx950 straggler-scoring kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NVRX_WAVE 64

namespace nvrx {

__device__ __forceinline__ int lane_id() { return __lane_id(); }

// Number of lanes below this one whose bit is set in mask.
__device__ __forceinline__ unsigned mbcnt(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// ---- cross-lane reductions on DPP (pure VALU, no LDS crossbar, no index VGPRs) ----
// Within each 16-lane row: quad_perm xor1 (0xB1), quad_perm xor2 (0x4E),
// row_half_mirror (0x141), row_mirror (0x140) pair every lane with a distinct partner,
// so after 4 steps every lane holds its row's result; the 4 row results are then
// combined from lanes 0/16/32/48 in a fixed order (uniform, deterministic).
template <int CTRL>
__device__ __forceinline__ unsigned dpp(unsigned x) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    const unsigned lo = dpp<CTRL>((unsigned)b), hi = dpp<CTRL>((unsigned)(b >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ unsigned rl(unsigned x, int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ double rl(double x, int l) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)b, l);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
    v = min(v, dpp<0xB1>(v));
    v = min(v, dpp<0x4E>(v));
    v = min(v, dpp<0x141>(v));
    v = min(v, dpp<0x140>(v));
    return min(min(rl(v, 0), rl(v, 16)), min(rl(v, 32), rl(v, 48)));
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    v = max(v, dpp<0xB1>(v));
    v = max(v, dpp<0x4E>(v));
    v = max(v, dpp<0x141>(v));
    v = max(v, dpp<0x140>(v));
    return max(max(rl(v, 0), rl(v, 16)), max(rl(v, 32), rl(v, 48)));
}
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
    v += dpp<0xB1>(v);
    v += dpp<0x4E>(v);
    v += dpp<0x141>(v);
    v += dpp<0x140>(v);
    return (rl(v, 0) + rl(v, 16)) + (rl(v, 32) + rl(v, 48));
}
// Fixed pairing order: every lane ends with the same, run-to-run identical sum
// (a + b == b + a exactly, so both partners of a pair agree).
__device__ __forceinline__ double wave_sum_f64(double v) {
    v = v + dpp_f64<0xB1>(v);
    v = v + dpp_f64<0x4E>(v);
    v = v + dpp_f64<0x141>(v);
    v = v + dpp_f64<0x140>(v);
    return (rl(v, 0) + rl(v, 16)) + (rl(v, 32) + rl(v, 48));
}
// Whole-wave reductions finished with row_bcast:15 / row_bcast:31 (rows 1,3 then rows 2,3
// take the previous rows' partials) -- two DPP ops instead of four readlanes and the scalar
// combine; the result is read from lane 63.  wave_sum_f64_b pairs (r3 + r2) + (r1 + r0),
// which by commutativity is bitwise wave_sum_f64's (r0 + r1) + (r2 + r3).
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned dpp_rows(unsigned old, unsigned x) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)x, CTRL, ROWS, 0xF, false);
}
__device__ __forceinline__ unsigned wave_min_b(unsigned v) {
    v = min(v, dpp<0xB1>(v));
    v = min(v, dpp<0x4E>(v));
    v = min(v, dpp<0x141>(v));
    v = min(v, dpp<0x140>(v));
    v = min(v, dpp_rows<0x142, 0xA>(v, v));
    v = min(v, dpp_rows<0x143, 0xC>(v, v));
    return rl(v, 63);
}
__device__ __forceinline__ unsigned wave_max_b(unsigned v) {
    v = max(v, dpp<0xB1>(v));
    v = max(v, dpp<0x4E>(v));
    v = max(v, dpp<0x141>(v));
    v = max(v, dpp<0x140>(v));
    v = max(v, dpp_rows<0x142, 0xA>(v, v));
    v = max(v, dpp_rows<0x143, 0xC>(v, v));
    return rl(v, 63);
}
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_rows_f64(double x) {  // 0.0 in the rows not selected
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    const unsigned lo = dpp_rows<CTRL, ROWS>(0u, (unsigned)b);
    const unsigned hi = dpp_rows<CTRL, ROWS>(0u, (unsigned)(b >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ double wave_sum_f64_b(double v) {
    v = v + dpp_f64<0xB1>(v);
    v = v + dpp_f64<0x4E>(v);
    v = v + dpp_f64<0x141>(v);
    v = v + dpp_f64<0x140>(v);
    v = v + dpp_rows_f64<0x142, 0xA>(v);
    v = v + dpp_rows_f64<0x143, 0xC>(v);
    return rl(v, 63);
}

// Inclusive prefix sum over the 64 lanes: row_shr 1/2/4/8 (bound_ctrl zero-fills
// lanes whose source is outside the row), then add the preceding rows' totals.
__device__ __forceinline__ unsigned wave_incl_scan_u32(unsigned v) {
    v += dpp<0x111>(v);
    v += dpp<0x112>(v);
    v += dpp<0x114>(v);
    v += dpp<0x118>(v);
    const int l = lane_id();
    const unsigned r0 = rl(v, 15), r1 = rl(v, 31), r2 = rl(v, 47);
    v += (l >= 16 ? r0 : 0u) + (l >= 32 ? r1 : 0u) + (l >= 48 ? r2 : 0u);
    return v;
}

// Per-lane sums of the samples d[0..PL) held in registers.
//   sd = sum d, exact: 64-bit add-with-carry on 32-bit halves (keeps v[] 32-bit; a zext
//        to i64 lets the scheduler widen every sample to a register pair and spill).
//   sq = sum (d - c)^2 about a pivot c that is one of the segment's own samples, so the
//        variance sq/n - ((sd - n c)/n)^2 does not cancel against the mean even for
//        tightly clustered durations with far outliers.  Squares accumulate in f32 over
//        two chains of <= 8 terms and are folded into f64: relative error ~1e-7
//        (tests/test_gpu_segment_stats.py bounds it against an f64 reference).
template <int PL>
__device__ __forceinline__ void lane_sums(const unsigned (&v)[PL], unsigned c, uint64_t& sd,
                                          double& sq) {
    unsigned lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
    double acc = 0.0;
    constexpr int G = PL < 16 ? PL : 16;
#pragma unroll
    for (int g = 0; g < PL; g += G) {
        float q0 = 0.0f, q1 = 0.0f;
#pragma unroll
        for (int i = 0; i < G; i += 2) {
            unsigned c0, c1;
            lo0 = __builtin_addc(lo0, v[g + i], 0u, &c0);
            hi0 += c0;
            lo1 = __builtin_addc(lo1, v[g + i + 1], 0u, &c1);
            hi1 += c1;
            const float fa = (float)(int)(v[g + i] - c), fb = (float)(int)(v[g + i + 1] - c);
            q0 = __builtin_fmaf(fa, fa, q0);
            q1 = __builtin_fmaf(fb, fb, q1);
        }
        acc += (double)q0 + (double)q1;
    }
    sd = ((uint64_t)hi0 << 32 | lo0) + ((uint64_t)hi1 << 32 | lo1);
    sq = acc;
}

// Same sums with f64 squares about c = 0, for masked segments whose padding holds d = 0
// (contributes nothing to either sum).
template <int PL>
__device__ __forceinline__ void lane_sums_f64(const unsigned (&v)[PL], uint64_t& sd, double& sq) {
    unsigned lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
    double q0 = 0.0, q1 = 0.0;
#pragma unroll
    for (int i = 0; i < PL; i += 2) {
        unsigned c0, c1;
        lo0 = __builtin_addc(lo0, v[i], 0u, &c0);
        hi0 += c0;
        lo1 = __builtin_addc(lo1, v[i + 1], 0u, &c1);
        hi1 += c1;
        const double fa = (double)v[i], fb = (double)v[i + 1];
        q0 = __builtin_fma(fa, fa, q0);
        q1 = __builtin_fma(fb, fb, q1);
    }
    sd = ((uint64_t)hi0 << 32 | lo0) + ((uint64_t)hi1 << 32 | lo1);
    sq = q0 + q1;
}

// Duration keys.  The reference keeps (end - start) / 1000.0f (CuptiProfiler.cpp:187): the u64
// ns difference converted to f32, then divided.  Every statistic it reports is therefore a
// function of f32(ns) alone, so a 32-bit key that is exactly ns below NVRX_KEY_WIDE (3.76 s) and
// the f32 bits of f32(ns) above it (offset to follow on) loses nothing and keeps the order:
//   key(ns) = ns                                              ns <  0xE0000000
//           = 0xE0000000 + bits(f32(ns)) - bits(f32(0xE0000000))   otherwise (<= 0xF0200000 for
//                                                              ns < 2^64)
// MIN / MAX / MED select on keys exactly as on ns; the FAST sums use d = key - MIN and are
// exact below NVRX_KEY_WIDE (segments reaching it take a decoded f64 pass instead).
#ifndef NVRX_KEY_WIDE  // also in include/nvrx_straggler.h
#define NVRX_KEY_WIDE 0xE0000000u
#define NVRX_KEY_WIDE_F32BITS 0x4F600000u  // bits of f32(0xE0000000) = 1.75 * 2^31
#endif

// f32(ns) of a key: the value the reference divides by 1000.  u32 values above NVRX_KEY_MAX
// (0xF0200000, the key of f32(2^64 - 1)) come from no u64 duration; they continue the same
// monotone f32 bit pattern (durations beyond 2^64 ns), so selection on keys stays exact for
// every u32.
__host__ __device__ __forceinline__ float key_to_f32(unsigned k) {
    return k < NVRX_KEY_WIDE ? (float)k : __builtin_bit_cast(float, k - NVRX_KEY_WIDE + NVRX_KEY_WIDE_F32BITS);
}

// CuptiProfiler.cpp:187 -- (end - start) / 1000.0f: integer ns -> f32 (round to nearest),
// then the correctly rounded f32 quotient by 1000.  Computed as one f64 multiply by
// RN(1/1000) rounded to f32 (4 VALU instead of the 11-instruction f32 divide sequence):
// x = f32(ns) is exact in f64 and the product is within 2^-52 relative of x/1000, while
// x/1000 is never an f32 rounding midpoint (its odd part would need > 24 bits) and lies at
// least 2^-24 relative away from every other one, so both round to the same f32.  Checked
// exhaustively for all 2^32 inputs (tests/test_oracle_golden.py re-checks a sample); the
// argument depends on the 24-bit significand only, so it holds for the f32 values of wide keys.
__device__ __forceinline__ float ns_to_us(unsigned key) {
    return (float)((double)key_to_f32(key) * (1.0 / 1000.0));
}
// the same for a key known to lie below NVRX_KEY_WIDE (the key is the ns), in f32 only: the
// product by 0.001f corrected by its residual (two FMAs) is the correctly rounded quotient
// (float)ns / 1000.0f for every such key -- checked exhaustively on gfx950 against the IEEE f32
// division and against the f64 form above (tools/probe_us_conversion.hip: 0 mismatches in
// 3,758,096,384 keys); f64 runs at half the f32 rate, and the lane classes convert every sample
__device__ __forceinline__ float ns_to_us_narrow(unsigned ns) {
    const float f = (float)ns;
    const float q = f * 0.001f;
    return __builtin_fmaf(__builtin_fmaf(-q, 1000.0f, f), 0.001f, q);
}

// Host side: the split rule of every kernel whose grid is (rows, splits of K).  About target_wgs
// workgroups over rows x splits, a split (kper columns) no shorter than one workgroup trip and a
// whole number of trips.  The result is <= target_wgs: it fits grid.y.  Needs R, K > 0.
inline int64_t row_splits(int64_t R, int64_t K, int64_t trip, int64_t target_wgs, int64_t* kper) {
    int64_t splits = (target_wgs + R - 1) / R;
    splits = splits < (K + trip - 1) / trip ? splits : (K + trip - 1) / trip;
    *kper = ((K + splits - 1) / splits + trip - 1) / trip * trip;
    return (K + *kper - 1) / *kper;
}

}  // namespace nvrx

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
