// histogram_scores.hip -- tail scores from the fixed-bucket histograms, on gfx950.
//
// No reference counterpart.  The scores of a report rest on medians (s = ref / MED): a rank that
// is slow on every n-th call keeps a healthy median.  The histograms of segment_histogram.hip have
// the same 240 buckets for every rank and kernel, so they add over ranks; these kernels turn
// counts[R][K][240] into one number per rank on the scale of the GPU scores, in exact integers:
//     F[k][b]      = sum_r C[r][k][b]                                          (u64)
//     T_k          = the bucket of the fleet's sample of rank (pm (N_k - 1)) / 1000
//     w(b)         = edge(min(b, 238))        the bucket's lower edge, a lower bound of its ns
//     total_ns[r]  = sum_k sum_b       C[r][k][b] w(b)
//     tail_ns[r]   = sum_k sum_{b>T_k} C[r][k][b] w(b)
//     score[r]     = (1 - tail_ns[r] / total_ns[r]) / (1 - fleet_tail / fleet_total)      (f64)
// (include/nvrx_straggler.h has the full definition).  Three stream-ordered entries:
//
//   histogram_sum        column sum over the rows of the [R][K * 60] matrix of 16-byte vectors.
//                        A thread owns one vector column and a range of rows, HS_UNROLL loads in
//                        flight, four u64 sums in registers.  grid.x covers the columns, grid.y
//                        splits the rows so that about 2,048 workgroups exist at any R: 64 rows
//                        and 16,384 rows both fill the device.  Combine: with one split the owner
//                        stores its sums (or adds them to `fleet`, accumulate); with more, `fleet`
//                        is cleared by a kernel on the stream first (unless accumulating) and every
//                        split adds its non-zero sums with 64-bit device atomics.  Partials plus a
//                        second pass would need splits * K * 1,920 B of scratch the entry may not
//                        allocate; a kernel's durations sit in a few buckets, so most sums are
//                        zero and are never sent; integer adds are exact in any order.
//   tail_threshold       one wave per kernel, 4 bins per lane on 60 lanes: a DPP inclusive prefix of
//                        the lanes' u64 sums locates the lane of the rank (ballot), the walk over
//                        that lane's four bins the bucket.  The weighted fleet sums of the kernel
//                        are reduced in the wave and added to fleet_sums (cleared on the stream by
//                        a kernel first) with one pair of 64-bit atomics per kernel.
//   tail_scores          one 1024-thread workgroup per row.  A wave takes a kernel per trip: 60
//                        lanes load its 960 B as one 16-byte vector each, so a lane's four weights
//                        are constants of the whole kernel and T_k is wave-uniform (scalar loads);
//                        TS_UNROLL kernels per wave are in flight.  Per lane two u64 accumulators
//                        fed by 32x32->64 multiply-adds, one DPP + LDS reduction at the end, then
//                        the three f64 operations of the score by one thread.  Only the CALLS
//                        instantiation reduces a 32-bit tail count per kernel (tail_calls).
// Every loop is bounded by R or K.  No kernel uses scratch memory (make asm).

#include "histogram_wave.h"

namespace nvrx {
namespace {

__global__ __launch_bounds__(256) void clear_u64_kernel(u64* p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0ull;
}

// ------------------------------------------------------------------ entry 1: the fleet histogram
constexpr int HS_THREADS = 256;
constexpr int HS_UNROLL = 8;        // rows in flight per thread
constexpr int HS_MIN_ROWS = 16;     // fewest rows worth a split of their own
constexpr int HS_TARGET_WGS = 2048; // 256 CUs x 8 workgroups

// V: vectors per row (K * 60); rows [blockIdx.y * rows_per, + rows_per) of column v
template <bool ATOMIC>
__global__ __launch_bounds__(HS_THREADS)
void histogram_sum_kernel(const u32x4* __restrict__ counts, int64_t R, int64_t V, int64_t rows_per,
                          int accumulate, u64* fleet) {
    const int64_t v = (int64_t)blockIdx.x * HS_THREADS + threadIdx.x;
    if (v >= V) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per;
    const int64_t r1 = min(R, r0 + rows_per);
    const u32x4* p = counts + r0 * V + v;
    u64 s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    int64_t r = r0;
    for (; r + HS_UNROLL <= r1; r += HS_UNROLL, p += HS_UNROLL * V) {
        u32x4 q[HS_UNROLL];
#pragma unroll
        for (int u = 0; u < HS_UNROLL; ++u) q[u] = __builtin_nontemporal_load(p + u * V);
#pragma unroll
        for (int u = 0; u < HS_UNROLL; ++u) {
            s0 += q[u].x;
            s1 += q[u].y;
            s2 += q[u].z;
            s3 += q[u].w;
        }
    }
    for (; r < r1; ++r, p += V) {
        const u32x4 q = __builtin_nontemporal_load(p);
        s0 += q.x;
        s1 += q.y;
        s2 += q.z;
        s3 += q.w;
    }
    u64* o = fleet + 4 * v;
    if (ATOMIC) {
        if (s0) atomicAdd(o + 0, s0);
        if (s1) atomicAdd(o + 1, s1);
        if (s2) atomicAdd(o + 2, s2);
        if (s3) atomicAdd(o + 3, s3);
    } else {
        u64x2 a = {s0, s1}, b = {s2, s3};
        if (accumulate) {
            a += *(const u64x2*)o;
            b += *(const u64x2*)(o + 2);
        }
        *(u64x2*)o = a;
        *(u64x2*)(o + 2) = b;
    }
}

// ------------------------------------------------------------------ entry 2: threshold buckets
__global__ __launch_bounds__(256)
void tail_threshold_kernel(const u64* __restrict__ fleet, int64_t K, int pm,
                           const uint8_t* __restrict__ col_valid, int32_t* thr, u64* fleet_sums) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t k = (int64_t)blockIdx.x * 4 + wave;
    if (k >= K) return;  // wave-uniform; the kernel has no workgroup barrier
    u64 h[4] = {0ull, 0ull, 0ull, 0ull};
    if (lane < HV) {
        const u64x2* p = (const u64x2*)(fleet + k * HB + 4 * lane);
        const u64x2 a = p[0], b = p[1];
        h[0] = a.x;
        h[1] = a.y;
        h[2] = b.x;
        h[3] = b.y;
    }
    const u64 local = (h[0] + h[1]) + (h[2] + h[3]);
    const u64 incl = wave_incl_scan_u64(local);
    const u64 n = rl_u64(incl, 63);
    int T = -1;
    if (n != 0 && (!col_valid || col_valid[k])) {  // wave-uniform
        // (pm (n - 1)) / 1000 without the product leaving 64 bits
        const u64 q = (n - 1) / 1000ull, m = (n - 1) % 1000ull;
        const u64 rank = (u64)pm * q + ((u64)pm * m) / 1000ull;
        // incl is non-decreasing and incl[59] = n > rank: the lanes at or below rank are a prefix
        const int L = (int)__popcll(__ballot(incl <= rank));
        u64 c = incl - local;
        int j = 0;
        c += h[0];
        j += c <= rank;
        c += h[1];
        j += c <= rank;
        c += h[2];
        j += c <= rank;
        T = (int)rl((unsigned)(4 * lane + j), L);
        u64 total = 0, tail = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = 4 * lane + i;
            const u64 t = h[i] * (u64)weight_of(b);
            total += t;
            tail += b > T ? t : 0ull;
        }
        total = wave_sum_u64(total);
        tail = wave_sum_u64(tail);
        if (lane == 0) {
            if (tail) atomicAdd(fleet_sums + 0, tail);
            if (total) atomicAdd(fleet_sums + 1, total);
        }
    }
    if (lane == 0) thr[k] = T;
}

// ------------------------------------------------------------------ entry 3: per-row scores
constexpr int TS_THREADS = 1024;
constexpr int TS_WAVES = TS_THREADS / 64;
constexpr int TS_UNROLL = 4;  // kernels in flight per wave

template <bool CALLS>
__global__ __launch_bounds__(TS_THREADS) void tail_scores_kernel(nvrx_tail_args a) {
    __shared__ u64 red[TS_WAVES][2];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const int b0 = 4 * lane;
    const unsigned w0 = weight_of(b0), w1 = weight_of(b0 + 1), w2 = weight_of(b0 + 2),
                   w3 = weight_of(b0 + 3);
    const u32x4* row = (const u32x4*)(a.counts + r * K * HB) + lane;
    u64 total = 0, tail = 0;
    for (int64_t k0 = wave; k0 < K; k0 += TS_WAVES * TS_UNROLL) {
        u32x4 q[TS_UNROLL];
        int T[TS_UNROLL];
#pragma unroll
        for (int u = 0; u < TS_UNROLL; ++u) {
            const int64_t k = k0 + u * TS_WAVES;  // wave-uniform
            q[u] = (u32x4){0u, 0u, 0u, 0u};
            T[u] = -1;
            if (k < K) {
                if (lane < HV) q[u] = __builtin_nontemporal_load(row + k * HV);
                const int64_t ti = a.thr_index ? (int64_t)a.thr_index[k] : k;
                if (ti >= 0) T[u] = a.thr[ti];
            }
        }
#pragma unroll
        for (int u = 0; u < TS_UNROLL; ++u) {
            const int64_t k = k0 + u * TS_WAVES;
            const int t = T[u];
            if (t >= 0) {  // wave-uniform; lanes 60..63 hold zeros
                const u64 p0 = (u64)q[u].x * w0, p1 = (u64)q[u].y * w1, p2 = (u64)q[u].z * w2,
                          p3 = (u64)q[u].w * w3;
                total += (p0 + p1) + (p2 + p3);
                tail += ((b0 > t ? p0 : 0ull) + (b0 + 1 > t ? p1 : 0ull)) +
                        ((b0 + 2 > t ? p2 : 0ull) + (b0 + 3 > t ? p3 : 0ull));
            }
            if (CALLS && k < K) {
                unsigned c = 0;
                if (t >= 0) {
                    c = ((b0 > t ? q[u].x : 0u) + (b0 + 1 > t ? q[u].y : 0u)) +
                        ((b0 + 2 > t ? q[u].z : 0u) + (b0 + 3 > t ? q[u].w : 0u));
                    c = wave_sum_u32(c);
                }
                if (lane == 0) a.tail_calls[r * K + k] = c;
            }
        }
    }
    total = wave_sum_u64(total);
    tail = wave_sum_u64(tail);
    if (lane == 0) {
        red[wave][0] = tail;
        red[wave][1] = total;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    u64 tl = 0, tt = 0;
#pragma unroll
    for (int w = 0; w < TS_WAVES; ++w) {
        tl += red[w][0];
        tt += red[w][1];
    }
    a.tail_ns[r] = tl;
    a.total_ns[r] = tt;
    const u64 ftail = a.fleet_sums[0], ftotal = a.fleet_sums[1];
    double score = __builtin_nan("");
    if (tt != 0 && ftotal != 0) {
        const double share = (double)tl / (double)tt;
        const double fs = (double)ftail / (double)ftotal;
        const double den = 1.0 - fs;
        if (den != 0.0) score = (1.0 - share) / den;
    }
    a.score[r] = score;
    if (a.strag) a.strag[r] = score < a.score_thr;  // NaN compares false
}

}  // namespace

// Argument checks happen in abi.cpp before these run.
hipError_t histogram_sum(const uint32_t* counts, int64_t R, int64_t K, int accumulate, uint64_t* fleet,
                         hipStream_t st) {
    if (R <= 0 || K <= 0) return hipSuccess;
    const int64_t n = K * HB;
    const int64_t V = K * HV;
    const int64_t nbx = (V + HS_THREADS - 1) / HS_THREADS;
    int64_t splits = (HS_TARGET_WGS + nbx - 1) / nbx;
    splits = min(splits, (R + HS_MIN_ROWS - 1) / HS_MIN_ROWS);
    const int64_t rows_per = (R + splits - 1) / splits;
    splits = (R + rows_per - 1) / rows_per;  // <= HS_TARGET_WGS: fits grid.y
    const dim3 grid((unsigned)nbx, (unsigned)splits);
    if (splits == 1) {
        hipLaunchKernelGGL(histogram_sum_kernel<false>, grid, dim3(HS_THREADS), 0, st,
                           (const u32x4*)counts, R, V, rows_per, accumulate, (u64*)fleet);
    } else {
        if (!accumulate)
            hipLaunchKernelGGL(clear_u64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                               (u64*)fleet, n);
        hipLaunchKernelGGL(histogram_sum_kernel<true>, grid, dim3(HS_THREADS), 0, st,
                           (const u32x4*)counts, R, V, rows_per, accumulate, (u64*)fleet);
    }
    return hipGetLastError();
}

hipError_t histogram_tail_threshold(const uint64_t* fleet, int64_t K, int permille,
                                    const uint8_t* col_valid, int32_t* thr, uint64_t* fleet_sums,
                                    hipStream_t st) {
    if (K <= 0) return hipSuccess;
    hipLaunchKernelGGL(clear_u64_kernel, dim3(1), dim3(256), 0, st, (u64*)fleet_sums, (int64_t)2);
    hipLaunchKernelGGL(tail_threshold_kernel, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, st,
                       (const u64*)fleet, K, permille, col_valid, thr, (u64*)fleet_sums);
    return hipGetLastError();
}

hipError_t histogram_tail_scores(const nvrx_tail_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    if (a.tail_calls)
        hipLaunchKernelGGL(tail_scores_kernel<true>, dim3((unsigned)a.R), dim3(TS_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(tail_scores_kernel<false>, dim3((unsigned)a.R), dim3(TS_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace nvrx
