// segment_emit.h -- the FAST epilogues: what lean_core returns to the six statistics, per
// segment (emit_stats) or for the segments whose results wait one per lane (LaneResults).
#pragma once
#include "segment_wave.h"

namespace nvrx {

// Epilogue of the FAST kernels, lane-parallel: lanes 0-3 convert MIN, MAX, s[t0], s[t1]
// in one ns_to_us, lanes 0/1 form avg and std from one f64 divide; lane 0 stores.
//   sd = sum(d), sq = sum((d - c)^2) over the n samples, d = x - MIN.
//   avg = (n MIN + sd) / (1000 n)               (numerator exact in f64)
//   std = sqrtf(f32((n sq - (sd - n c)^2) / (1000 n)^2))  (population std, CuptiProfiler.cpp:66-70)
// num / dd from the hardware reciprocal refined by two Newton steps and one residual
// correction (~1e-16 relative; emit_stats and the group epilogue share it, so both round alike)
__device__ __forceinline__ double quot_f64(double num, double dd) {
    double rc = __builtin_amdgcn_rcp(dd);
    rc = __builtin_fma(rc, __builtin_fma(-dd, rc, 1.0), rc);
    rc = __builtin_fma(rc, __builtin_fma(-dd, rc, 1.0), rc);
    double q = num * rc;
    return __builtin_fma(__builtin_fma(-dd, q, num), rc, q);
}

__device__ __forceinline__ void emit_stats(const nvrx_stats_soa& o, int64_t s, int n,
                                           unsigned mn, unsigned mx, unsigned d0, unsigned d1,
                                           double sd, double sq, unsigned c, const ColRef& cr) {
    const int lane = lane_id();
    const unsigned x = lane == 0 ? mn : lane == 1 ? mx : lane == 2 ? mn + d0 : mn + d1;
    const float f = mx < NVRX_KEY_WIDE ? ns_to_us_narrow(x) : ns_to_us(x);  // wave-uniform
    const float fmn = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f), 0));
    const float fmx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f), 1));
    const float f0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f), 2));
    const float f1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, f), 3));
    // CuptiProfiler.cpp:58: f32 add, exact halving
    const float med = (n & 1) ? f0 : (f0 + f1) / 2;
    const double dn = (double)n;
    const double se = sd - dn * (double)c;  // exact: integers < 2^53
    // lane 0: avg = (n MIN + sd) / (1000 n), rounded once to f32;
    // lane 1: std = sqrt(n sq - se^2) / (1000 n) as the f32 root of the f32-rounded variance
    //         in us^2.
    // The quotient is num times the hardware reciprocal refined by Newton steps (~1e-16
    // relative, so at most a rounding-boundary case off the correctly rounded f32) and the root
    // is the hardware v_sqrt_f32 (~1 ulp): both inside the FAST bound,
    // without the f64 divide and correctly rounded sqrt sequences (~20 of ~400 VALU
    // per segment at 1024 samples).
    const double den = 1000.0 * dn;
    const double vq = __builtin_fma(sq, dn, -(se * se));
    const double num = lane == 0 ? __builtin_fma((double)mn, dn, sd) : (vq > 0.0 ? vq : 0.0);
    const double dd = lane == 0 ? den : den * den;
    const double q = quot_f64(num, dd);
    const float r = lane == 0 ? (float)q : __builtin_amdgcn_sqrtf((float)q);
    const float avg = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), 0));
    const float sdv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), 1));
    if (lane == 0) {
        o.num[s] = n;
        o.min[s] = fmn;
        o.max[s] = fmx;
        o.med[s] = med;
        o.avg[s] = avg;
        o.std[s] = sdv;
        cr.add(s, med);
    }
}

// emit_stats for one segment per lane (the group epilogues: lane j holds segment s0 + j's
// results); the same arithmetic, so the same bits.  k0 / k1: the middle-rank keys (mn + d0,
// mn + d1).
__device__ __forceinline__ void emit_lane(const nvrx_stats_soa& o, int64_t s, int n, unsigned mn,
                                          unsigned mx, unsigned k0, unsigned k1, double sd,
                                          double sq, unsigned c, const ColRef& cr) {
    const float f0 = ns_to_us(k0), f1 = ns_to_us(k1);
    const float med = (n & 1) ? f0 : (f0 + f1) / 2;  // CuptiProfiler.cpp:58
    const double dn = (double)n;
    const double se = sd - dn * (double)c;
    const double den = 1000.0 * dn;
    const double vq = __builtin_fma(sq, dn, -(se * se));
    o.num[s] = n;
    o.min[s] = ns_to_us(mn);
    o.max[s] = ns_to_us(mx);
    o.med[s] = med;
    o.avg[s] = (float)quot_f64(__builtin_fma((double)mn, dn, sd), den);
    o.std[s] = __builtin_amdgcn_sqrtf((float)quot_f64(vq > 0.0 ? vq : 0.0, den * den));
    cr.add(s, med);
}

// FAST AVG / STD of a segment whose keys reach NVRX_KEY_WIDE (a kernel of 3.76 s or more): the
// integer sums of the bodies do not apply to f32-valued keys, so lane 0 overwrites what
// emit_stats stored with the mean and population std of the decoded f32(ns) values in f64, each
// rounded once to f32 us -- two strided passes over the segment p[0:n) in memory (no register
// arrays: this rare branch must not raise the bodies' register pressure).
__device__ __forceinline__ void wide_moments(const uint32_t* p, int n, int64_t s, const nvrx_stats_soa& o) {
    const int lane = lane_id();
    double a = 0.0;
    for (int i = lane; i < n; i += 64) a += (double)key_to_f32(p[i]);
    const double mean = wave_sum_f64(a) / (double)n;
    double q = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double e = (double)key_to_f32(p[i]) - mean;
        q = __builtin_fma(e, e, q);
    }
    const double var = wave_sum_f64(q) / (double)n;
    if (lane == 0) {
        o.avg[s] = (float)(mean / 1000.0);
        o.std[s] = (float)(__builtin_sqrt(var) / 1000.0);
    }
}

// The results of up to 64 segments a wave reduced one after another, segment j's in lane j, so
// the epilogue (emit_lane) runs once for all of them, lane-parallel with coalesced stores.
// Mask: one bit per entry with a key of NVRX_KEY_WIDE or more (uint32_t for up to 32 entries).
template <int PL, class Mask>
struct LaneResults {
    // nine 32-bit registers; the halves of sd and sq apart, so that the compiler does not read a
    // pair back as one 64-bit value and carry it as such (another register allocation)
    unsigned mn, mx, k0, k1, c, sdlo, sqlo, sdhi, sqhi;
    Mask wide;
    // entry j = r: one compare, nine selects
    __device__ __forceinline__ void keep(int j, const LeanOut<PL>& r) {
        const uint64_t sqb = (uint64_t)__double_as_longlong(r.sq);
        const bool mine = lane_id() == j;
        mn = mine ? r.mn : mn;
        mx = mine ? r.mx : mx;
        k0 = mine ? r.mn + r.d0 : k0;
        k1 = mine ? r.mn + r.d1 : k1;
        c = mine ? r.c : c;
        const uint64_t sdb = sd_bits(r.sd);
        sdlo = mine ? (uint32_t)sdb : sdlo;
        sdhi = mine ? (uint32_t)(sdb >> 32) : sdhi;
        sqlo = mine ? (uint32_t)sqb : sqlo;
        sqhi = mine ? (uint32_t)(sqb >> 32) : sqhi;
        if (r.mx >= NVRX_KEY_WIDE) wide |= (Mask)1 << j;
    }
    // this lane's entry: segment s of n samples.  For the lanes below the number of entries kept;
    // the caller tests that, so that what it computes s from stays under the branch.
    __device__ __forceinline__ void emit(const nvrx_stats_soa& o, int64_t s, int n, const ColRef& cr) const {
        emit_lane(o, s, n, mn, mx, k0, k1, sd_value<PL>(((uint64_t)sdhi << 32) | sdlo),
                  __longlong_as_double((long long)(((uint64_t)sqhi << 32) | sqlo)), c, cr);
    }
    // f(j) for every entry with wide keys, ascending (they take wide_moments: rare)
    template <class F>
    __device__ __forceinline__ void each_wide(F&& f) {
        while (wide) {
            const int j = (sizeof(Mask) > 4 ? __builtin_ffsll((long long)wide) : __builtin_ffs((int)wide)) - 1;
            wide &= wide - 1;
            f(j);
        }
    }
};

}  // namespace nvrx
