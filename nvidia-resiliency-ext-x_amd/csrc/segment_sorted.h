// segment_sorted.h -- statistics over sorted samples, the reference statement by statement:
// one segment per lane in a register sorting network (lane_stats), one per workgroup bitonic-
// sorted in LDS (exact_body) or in device scratch (exact_global_body).
#pragma once
#include <algorithm>

#include "segment_addr.h"

namespace nvrx {

// Batcher's odd-even merge sort over N registers (N a power of two) as a compile-time list of
// compare-exchanges -- v_min/v_max pairs, no LDS, no branches: 19 / 63 / 191 / 543 / 1471 of them
// for N = 8 / 16 / 32 / 64 / 128, against the bitonic network's 24 / 80 / 240 / 672 / 1792.
template <int N>
struct OemNet {
    template <class F>
    static constexpr void walk(F&& f) {
        for (int p = 1; p < N; p += p)
            for (int k = p; k > 0; k /= 2)
                for (int j = k % p; j + k < N; j += k + k)
                    for (int i = 0; i < k && i + j + k < N; ++i)
                        if ((i + j) / (p + p) == (i + j + k) / (p + p)) f(i + j, i + j + k);
    }
    static constexpr int count() {
        int c = 0;
        walk([&](int, int) { ++c; });
        return c;
    }
    static constexpr int NC = count();
    short a[NC], b[NC];
    constexpr OemNet() : a(), b() {
        int c = 0;
        walk([&](int x, int y) {
            a[c] = (short)x;
            b[c] = (short)y;
            ++c;
        });
    }
};
// compare-exchanges [LO, HI) of the network, split in halves down to single ones, so every
// register index is a constant expression (a loop over the table left 128-register networks
// with runtime indices: the array went to scratch)
template <int N, int LO, int HI>
__device__ __forceinline__ void net_range(unsigned (&v)[N]) {
    if constexpr (HI - LO == 1) {
        constexpr OemNet<N> net{};
        constexpr int a = net.a[LO], b = net.b[LO];
        const unsigned x = v[a], y = v[b];
        v[a] = min(x, y);
        v[b] = max(x, y);
    } else if constexpr (HI - LO > 1) {
        net_range<N, LO, (LO + HI) / 2>(v);
        net_range<N, (LO + HI) / 2, HI>(v);
    }
}
template <int N>
__device__ __forceinline__ void sort_net(unsigned (&v)[N]) {
    net_range<N, 0, OemNet<N>::NC>(v);
}

constexpr int pow2_ceil(int m) {
    int p = 1;
    while (p < m) p += p;
    return p;
}
// v[idx] for a runtime idx known to lie in the compile-time range [LO, HI] (any register of the
// range otherwise): a multiplexer tree on the bits of idx - LO, one v_cndmask per candidate,
// instead of a compare and a select per register.
template <int LO, int HI, int N>
__device__ __forceinline__ unsigned pick(const unsigned (&v)[N], int idx) {
    constexpr int P = pow2_ceil(HI - LO + 1);
    unsigned t[P];
#pragma unroll
    for (int j = 0; j < P; ++j) t[j] = v[LO + j <= HI ? LO + j : HI];
    const unsigned k = (unsigned)(idx - LO);
#pragma unroll
    for (int w = P, bit = 1; w > 1; w >>= 1, bit += bit) {
        const bool hi = (k & (unsigned)bit) != 0u;
#pragma unroll
        for (int j = 0; j < w / 2; ++j) t[j] = hi ? t[2 * j + 1] : t[2 * j];
    }
    return t[0];
}

// One segment of n samples per LANE, NMIN <= n <= N (v: the n samples in slots [0, n) in any
// order, slots >= n ignored; a length class guarantees NMIN, so slots below it need no masks).
// u32 -> f32 us is monotone, so sorting the integer ns sorts the floats computeStats sorts; then
// CuptiProfiler.cpp:53-71 statement by statement (sequential f32 sums over the sorted samples)
// -- every field bit-exact.
template <int N, int NMIN = 1>
__device__ __forceinline__ void lane_stats(unsigned (&v)[N], int n, int64_t s,
                                           const nvrx_stats_soa& out, const ColRef& cr) {
    static_assert(NMIN >= 1 && NMIN <= N, "NMIN in [1, N]");
#pragma unroll
    for (int j = NMIN; j < N; ++j) v[j] = j < n ? v[j] : 0xFFFFFFFFu;  // sentinels sort last
    sort_net<N>(v);
    float acc = 0.0f;
    // keys of 3.76 s and more (rare) are decoded; the wave takes the plain conversion unless
    // one of its lanes holds such a key
    const bool wide = __ballot(pick<NMIN - 1, N - 1>(v, n - 1) >= NVRX_KEY_WIDE) != 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float f = wide ? ns_to_us(v[j]) : ns_to_us_narrow(v[j]);
        v[j] = __float_as_uint(f);
        acc = (j < NMIN || j < n) ? acc + f : acc;  // accumulate(sorted, 0.0f): sequential f32
    }
    // s[n-1], s[n/2] and s[n/2 - 1] (the latter read only for even n >= 2)
    const float fmin = __uint_as_float(v[0]);
    const float fmax = __uint_as_float(pick<NMIN - 1, N - 1>(v, n - 1));
    const float f1 = __uint_as_float(pick<NMIN / 2, N / 2>(v, n / 2));
    const float f0 = __uint_as_float(pick<(NMIN / 2 > 0 ? NMIN / 2 - 1 : 0), N / 2 - 1>(v, n / 2 - 1));
    const float med = (n & 1) ? f1 : (f0 + f1) / 2;
    const float avg = acc / (float)n;
    float sq = 0.0f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float t = __uint_as_float(v[j]) - avg;
        sq = (j < NMIN || j < n) ? sq + t * t : sq;
    }
    out.num[s] = n;
    out.min[s] = fmin;
    out.max[s] = fmax;
    out.med[s] = med;
    out.avg[s] = avg;
    out.std[s] = (float)__builtin_sqrt((double)(sq / (float)n));  // sqrtf, correctly rounded
    cr.add(s, med);
}

// ---------------------------------------------------------------------------
// EXACT mode: one 256-thread workgroup per segment, bitonic sort in LDS.
// ---------------------------------------------------------------------------
// Block-wide body: the segment p[0:n), n >= 1, into sbuf[NMAX] (LDS), sorted, then the
// reference's statistics statement by statement.  Every thread of the block calls it.
template <int NMAX>
__device__ __forceinline__ void exact_body(const uint32_t* p, int n, int64_t s, float* sbuf,
                                           const nvrx_stats_soa& out, const ColRef& cr) {
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    for (int i = threadIdx.x; i < np2; i += blockDim.x)
        sbuf[i] = (i < n) ? ns_to_us(p[i]) : __builtin_inff();
    __syncthreads();
    // bitonic sort, ascending (+inf padding sorts last)
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < np2; i += blockDim.x) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const float a = sbuf[i], b = sbuf[ixj];
                    const bool up = (i & k) == 0;
                    if (up ? (a > b) : (a < b)) {
                        sbuf[i] = b;
                        sbuf[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        // CuptiProfiler.cpp:53-71, statement by statement
        const float mnv = sbuf[0], mxv = sbuf[n - 1];
        float med;
        if (n % 2 == 0)
            med = (sbuf[n / 2 - 1] + sbuf[n / 2]) / 2;
        else
            med = sbuf[n / 2];
        float acc = 0.0f;
        for (int i = 0; i < n; ++i) acc = acc + sbuf[i];
        const float avg = acc / (float)n;
        float sqs = 0.0f;
        for (int i = 0; i < n; ++i) {
            const float t = sbuf[i] - avg;
            sqs = sqs + t * t;
        }
        // sqrtf, correctly rounded: f64 sqrt then one rounding to f32 is exact for sqrt
        const float sd = (float)__builtin_sqrt((double)(sqs / (float)n));
        out.num[s] = n;
        out.min[s] = mnv;
        out.max[s] = mxv;
        out.med[s] = med;
        cr.add(s, med);
        out.avg[s] = avg;
        out.std[s] = sd;
    }
    __syncthreads();  // sbuf is reused by the block's next segment
}

// ---------------------------------------------------------------------------
// Rings longer than the LDS holds (statsMaxLenPerKernel > NVRX_LDS_SEGMENT; the reference's
// CircularBuffer takes any capacity, CuptiProfiler.h:49-51).  One 1024-thread workgroup per
// segment sorts its samples in a slice `g` of a device scratch buffer (np2 floats): the bitonic
// stages whose partner distance j reaches XG_CHUNK run in global memory; for every k the stages
// below it stay inside aligned XG_CHUNK blocks, which are sorted in LDS.  The sequential f32 sums
// of computeStats then run on one lane over the sorted samples staged through LDS chunk by
// chunk -- the same statements, so every field is bit-exact.  Global stores are visible to the
// block after __syncthreads (one workgroup, one CU).
// ---------------------------------------------------------------------------
#define XG_CHUNK 8192
#define XG_THREADS 1024
__device__ __forceinline__ void bitonic_step(float* b, int i, int j, int k) {
    const int ixj = i ^ j;
    if (ixj > i) {
        const float a = b[i], c = b[ixj];
        if (((i & k) == 0) ? (a > c) : (a < c)) {
            b[i] = c;
            b[ixj] = a;
        }
    }
}

__device__ __forceinline__ void exact_global_body(const uint32_t* p, int n, int64_t s, float* g,
                                                  float* lds, const nvrx_stats_soa& out,
                                                  const ColRef& cr) {
    int np2 = XG_CHUNK;
    while (np2 < n) np2 <<= 1;
    for (int i = threadIdx.x; i < np2; i += XG_THREADS) g[i] = (i < n) ? ns_to_us(p[i]) : __builtin_inff();
    __syncthreads();
    // the stages of k <= XG_CHUNK, one aligned chunk at a time in LDS; then, for every larger k,
    // the global stages (j >= XG_CHUNK) and the remaining ones per chunk in LDS.  The direction
    // bit (i & k) is taken on the global index.
    for (int k = 2; k <= np2; k <<= 1) {
        if (k <= XG_CHUNK && k != 2) continue;  // k = 2 .. XG_CHUNK all run on the first visit
        const int kmax = k == 2 ? XG_CHUNK : k;
        int j = k >> 1;
        if (k > XG_CHUNK) {
            for (; j >= XG_CHUNK; j >>= 1) {  // partners XG_CHUNK or more apart: global memory
                for (int i = threadIdx.x; i < np2; i += XG_THREADS) bitonic_step(g, i, j, k);
                __syncthreads();
            }
        }
        for (int c0 = 0; c0 < np2; c0 += XG_CHUNK) {
            for (int i = threadIdx.x; i < XG_CHUNK; i += XG_THREADS) lds[i] = g[c0 + i];
            __syncthreads();
            for (int kk = k; kk <= kmax; kk <<= 1) {
                for (int jj = (kk == k ? j : kk >> 1); jj > 0; jj >>= 1) {
                    for (int i = threadIdx.x; i < XG_CHUNK; i += XG_THREADS) {
                        const int ixj = i ^ jj;
                        if (ixj > i) {
                            const float a = lds[i], c = lds[ixj];
                            if ((((c0 + i) & kk) == 0) ? (a > c) : (a < c)) {
                                lds[i] = c;
                                lds[ixj] = a;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            for (int i = threadIdx.x; i < XG_CHUNK; i += XG_THREADS) g[c0 + i] = lds[i];
            __syncthreads();
        }
    }
    // CuptiProfiler.cpp:53-71, statement by statement; the sums stage the sorted samples in LDS
    float acc = 0.0f;
    for (int c0 = 0; c0 < n; c0 += XG_CHUNK) {
        const int m = min(XG_CHUNK, n - c0);
        for (int i = threadIdx.x; i < m; i += XG_THREADS) lds[i] = g[c0 + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) acc = acc + lds[i];
        __syncthreads();
    }
    const float avg = acc / (float)n;  // meaningful on thread 0 only (the others never summed)
    float sqs = 0.0f;
    for (int c0 = 0; c0 < n; c0 += XG_CHUNK) {
        const int m = min(XG_CHUNK, n - c0);
        for (int i = threadIdx.x; i < m; i += XG_THREADS) lds[i] = g[c0 + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) {
                const float t = lds[i] - avg;
                sqs = sqs + t * t;
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float med = (n % 2 == 0) ? (g[n / 2 - 1] + g[n / 2]) / 2 : g[n / 2];
        out.num[s] = n;
        out.min[s] = g[0];
        out.max[s] = g[n - 1];
        out.med[s] = med;
        cr.add(s, med);
        out.avg[s] = avg;
        out.std[s] = (float)__builtin_sqrt((double)(sqs / (float)n));
    }
    __syncthreads();  // g and lds are reused by the block's next segment
}

// scratch for the global path: np2 floats per block, bounded to ~256 MiB (at least one block)
static inline int64_t exact_global_np2(int64_t max_len) {
    int64_t np2 = XG_CHUNK;
    while (np2 < max_len) np2 <<= 1;
    return np2;
}
static inline int64_t exact_global_blocks(int64_t np2, int64_t want) {
    const int64_t per = std::max<int64_t>(1, ((int64_t)256 << 20) / (np2 * (int64_t)sizeof(float)));
    return std::max<int64_t>(1, std::min(want, per));
}

}  // namespace nvrx
