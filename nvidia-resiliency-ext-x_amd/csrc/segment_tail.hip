// segment_tail.hip -- tail scores straight from ragged segments, on gfx950.
//
// No reference counterpart.  The tail-score chain of histogram_scores.hip starts from a dense
// counts[R][K][240] matrix: 960 B per (rank, kernel).  Record streams (records.hip) leave a few
// samples in most buckets, and at 16,384 ranks x 2,048 kernels the matrix would be 32 GB for 6 GB
// of records.  The scores never need it: by the ABI's definition they are integer sums over the
// samples, so two passes over the bucketed samples give the same bits,
//     F[k][b]     = sum_r #{x in window(r, k) : bucket(x) = b}                       (u64)
//     total_ns[r] = sum_k sum_x w(bucket(x)),   tail_ns[r] the same over bucket(x) > T_k
// with nvrx_histogram_tail_threshold (unchanged) between them for T_k and the fleet's sums.
// Segments are addressed as nvrx_segment_histogram_ragged addresses them (segment_addr.h):
// segment r K + k, the last `cap` samples retained, seg_len <= 0 contributes nothing.
//
// Both kernels sort a wave's 64 segments into two treatments:
//   lane   retained length <= ST_LANE_MAX (16): the lane that loaded the segment's offset and
//          length walks it alone, four loads in flight;
//   wave   longer: the wave takes such segments one after the other (ballot over the lanes that
//          hold one), 64 consecutive samples per load, four loads in flight.
//
//   segment_fleet_kernel   a 256-thread workgroup owns SF_COLS = 32 columns x a block of rows and
//          their 32 x 240 u32 bins in LDS (30 KB: five workgroups per CU).  A wave takes two
//          rows x 32 columns per trip, the next trip's offsets and lengths loaded before the
//          current one is counted.  The lanes of the lane class sit on 32 different columns (two
//          rows each), so their LDS adds do not meet on one address unless two rows hit the same
//          bucket of the same kernel.  The wave class counts 64 samples at a time: the bucket of
//          the first live lane is counted with one ballot + population count and one LDS add,
//          twice, and only the lanes left add on their own -- clustered input (a real kernel's
//          durations sit in one to three buckets) costs one or two LDS adds per 64 samples.  At
//          the end the non-zero bins are added to `fleet` with 64-bit device atomics (integer adds
//          are exact in any order; `fleet` is cleared by a kernel on the stream first unless
//          accumulating): a hot column costs one atomic per non-zero bin and row block, not one
//          per sample.  The row blocks are sized so that about 2,048 workgroups exist (64 rows
//          and 16,384 rows both fill the device) and no LDS bin can pass 2^32.
//   segment_tail_kernel    grid (rows, splits of K), the split rule of histogram_history.hip.  A
//          lane takes a column per trip, so seg_off / seg_len / thr_index of a row are coalesced
//          reads; per-lane u64 accumulators, one DPP + LDS reduction per workgroup, non-zero sums
//          added to the row's tail_ns / total_ns (cleared on the stream first).  Only the CALLS
//          instantiation counts and stores tail_calls.
//   segment_tail_finalize_kernel   the three separately rounded f64 operations of the score and
//          the straggler flag, per row: the operations of tail_scores_kernel's last thread.
// Every loop is bounded by a segment length, R or K.  No kernel uses scratch memory (make asm;
// DESIGN 3.14).

#include "histogram_wave.h"
#include "segment_addr.h"

namespace nvrx {
namespace {

constexpr unsigned ST_NONE = HB; // the bucket of a slot past the segment's end

__global__ __launch_bounds__(256) void clear2_u64_kernel(u64* a, u64* b, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        a[i] = 0ull;
        if (b) b[i] = 0ull;
    }
}

// ------------------------------------------------------------------ the fleet histogram
constexpr int SF_THREADS = 256;
constexpr int SF_WAVES = SF_THREADS / 64;
constexpr int SF_COLS = 32;                        // columns per workgroup
constexpr int SF_ROWS = 64 / SF_COLS;              // rows per wave trip
constexpr int SF_TRIP = SF_WAVES * SF_ROWS;        // rows per workgroup trip
constexpr int SF_STRIDE = HB + 1;                  // LDS words per column: odd, the columns of a
                                                   // wave start on different banks
constexpr int SF_TARGET_WGS = 2048;                // 256 CUs x 8 workgroups
static_assert((SF_COLS & (SF_COLS - 1)) == 0 && 64 % SF_COLS == 0, "columns per wave");

__global__ __launch_bounds__(SF_THREADS)
void segment_fleet_kernel(RaggedSegs segs, int64_t R, int64_t K, int64_t nbx, int64_t rows_per, u64* fleet) {
    __shared__ unsigned h[SF_COLS * SF_STRIDE];
    const int tid = threadIdx.x;
    for (int i = tid; i < SF_COLS * SF_STRIDE; i += SF_THREADS) h[i] = 0u;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = lane_id();
    const int64_t by = (int64_t)blockIdx.x / nbx;
    const int64_t c0 = ((int64_t)blockIdx.x - by * nbx) * SF_COLS;
    const int64_t r0 = by * rows_per;
    const int64_t r1 = min(R, r0 + rows_per);
    const int col = lane & (SF_COLS - 1);
    const int64_t k = c0 + col;
    unsigned* const hc = h + col * SF_STRIDE;
    // the lane's segment of the trip that starts at row rb: (nullptr, 0) outside the block
    const auto fetch = [&](int64_t rb, const uint32_t*& p, int& n) {
        const int64_t r = rb + (lane / SF_COLS);
        p = nullptr;
        n = 0;
        if (rb < r1 && r < r1 && k < K) segs.get(r * K + k, p, n);
    };
    const uint32_t *p, *pn;
    int n, nn;
    fetch(r0 + wave * SF_ROWS, p, n);
    for (int64_t rb = r0 + wave * SF_ROWS; rb < r1; rb += SF_TRIP) {  // wave-uniform
        fetch(rb + SF_TRIP, pn, nn);
        if (n > 0 && n <= ST_LANE_MAX) {
            for (int i = 0; i < n; i += ST_UNROLL) {
                unsigned x[ST_UNROLL];
                lane_load(p, n, i, x);
#pragma unroll
                for (int u = 0; u < ST_UNROLL; ++u)
                    if (i + u < n) atomicAdd(&hc[bucket_of(x[u])], 1u);
            }
        }
        uint64_t longs = __ballot(n > ST_LANE_MAX);
        while (longs) {  // wave-uniform
            const int l = __builtin_ctzll(longs);
            longs &= longs - 1;
            const uint32_t* q = rl_ptr(p, l);
            const int m = (int)rl((unsigned)n, l);
            unsigned* const hl = h + (l & (SF_COLS - 1)) * SF_STRIDE;
            for (int base = 0; base < m; base += 64 * ST_UNROLL) {
                unsigned x[ST_UNROLL];
                wave_load(q, m, base, x);
#pragma unroll
                for (int u = 0; u < ST_UNROLL; ++u) {
                    if (base + u * 64 >= m) break;  // wave-uniform
                    count_wave<ST_NONE>(base + u * 64 + lane < m ? bucket_of(x[u]) : ST_NONE, hl);
                }
            }
        }
        p = pn;
        n = nn;
    }
    __syncthreads();
    for (int i = tid; i < SF_COLS * HB; i += SF_THREADS) {
        const int c = i / HB, b = i - c * HB;
        const unsigned v = h[c * SF_STRIDE + b];
        if (v && c0 + c < K) atomicAdd(fleet + (c0 + c) * HB + b, (u64)v);
    }
}

// ------------------------------------------------------------------ per-row sums and scores
constexpr int TT_THREADS = 256;
constexpr int TT_WAVES = TT_THREADS / 64;
constexpr int TT_TRIP = TT_THREADS;  // columns per workgroup trip: a split's granule
constexpr int TT_TARGET_WGS = 2048;

// columns [blockIdx.y * kper, + kper) of row blockIdx.x
template <bool CALLS>
__global__ __launch_bounds__(TT_THREADS)
void segment_tail_kernel(RaggedSegs segs, nvrx_segtail_args a, int64_t kper) {
    __shared__ u64 red[TT_WAVES][2];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const int64_t ks = (int64_t)blockIdx.y * kper;
    const int64_t ke = min(K, ks + kper);
    TailAcc<true> acc;  // the calls are dead code without CALLS
    for (int64_t kb = ks + wave * 64; kb < ke; kb += TT_TRIP) {  // wave-uniform
        const int64_t k = kb + lane;
        int T = -1, n = 0;
        const uint32_t* p = nullptr;
        if (k < ke) {
            const int64_t ti = a.thr_index ? (int64_t)a.thr_index[k] : k;
            if (ti >= 0) T = a.thr[ti];
            if (T >= 0) segs.get(r * K + k, p, n);
        }
        acc.calls = 0;
        if (n > 0 && n <= ST_LANE_MAX) {
            for (int i = 0; i < n; i += ST_UNROLL) {
                unsigned x[ST_UNROLL];
                lane_load(p, n, i, x);
#pragma unroll
                for (int u = 0; u < ST_UNROLL; ++u)
                    if (i + u < n) acc.add(x[u], T);
            }
        }
        // a skipped or empty (r, k) gets 0; a wave-class one is written below
        if (CALLS && k < ke && n <= ST_LANE_MAX) a.tail_calls[r * K + k] = acc.calls;
        uint64_t longs = __ballot(n > ST_LANE_MAX);
        while (longs) {  // wave-uniform
            const int l = __builtin_ctzll(longs);
            longs &= longs - 1;
            const uint32_t* q = rl_ptr(p, l);
            const int m = (int)rl((unsigned)n, l);
            const int t = (int)rl((unsigned)T, l);
            acc.calls = 0;
            for (int base = 0; base < m; base += 64 * ST_UNROLL) {
                unsigned x[ST_UNROLL];
                wave_load(q, m, base, x);
#pragma unroll
                for (int u = 0; u < ST_UNROLL; ++u)
                    if (base + u * 64 + lane < m) acc.add(x[u], t);
            }
            if (CALLS) {
                const unsigned c = wave_sum_u32(acc.calls);
                if (lane == 0) a.tail_calls[r * K + kb + l] = c;
            }
        }
    }
    const u64 total = wave_sum_u64(acc.total);
    const u64 tail = wave_sum_u64(acc.tail);
    if (lane == 0) {
        red[wave][0] = tail;
        red[wave][1] = total;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    u64 tl = 0, tt = 0;
#pragma unroll
    for (int w = 0; w < TT_WAVES; ++w) {
        tl += red[w][0];
        tt += red[w][1];
    }
    if (tl) atomicAdd((u64*)a.tail_ns + r, tl);
    if (tt) atomicAdd((u64*)a.total_ns + r, tt);
}

__global__ __launch_bounds__(256) void segment_tail_finalize_kernel(nvrx_segtail_args a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.R) return;
    const u64 tl = a.tail_ns[r], tt = a.total_ns[r];
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
hipError_t segment_fleet_histogram_ragged(const uint32_t* ns, const int64_t* seg_off,
                                          const int32_t* seg_len, int64_t R, int64_t K, int64_t max_len,
                                          int64_t cap, int accumulate, uint64_t* fleet, hipStream_t st) {
    if (R <= 0 || K <= 0) return hipSuccess;
    const int64_t n = K * HB;
    if (!accumulate)
        hipLaunchKernelGGL(clear2_u64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                           (u64*)fleet, (u64*)nullptr, n);
    const int64_t nbx = (K + SF_COLS - 1) / SF_COLS;
    int64_t splits = (SF_TARGET_WGS + nbx - 1) / nbx;
    splits = min(splits, (R + SF_TRIP - 1) / SF_TRIP);
    int64_t rows_per = (R + splits - 1) / splits;
    // a block's rows add into u32 LDS bins: rows_per * the longest retained run stays below 2^32
    const int64_t keep = seg_keep(max_len, cap);
    rows_per = min(rows_per, max((int64_t)1, (int64_t)0xFFFFFFFFll / max(keep, (int64_t)1)));
    splits = (R + rows_per - 1) / rows_per;  // nbx * splits <= R * K / 32 + R < 2^31: fits grid.x
    hipLaunchKernelGGL(segment_fleet_kernel, dim3((unsigned)(nbx * splits)), dim3(SF_THREADS), 0, st,
                       RaggedSegs{ns, seg_off, seg_len, cap}, R, K, nbx, rows_per, (u64*)fleet);
    return hipGetLastError();
}

hipError_t segment_tail_scores_ragged(const nvrx_segtail_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    int64_t kper;
    const int64_t splits = row_splits(a.R, a.K, TT_TRIP, TT_TARGET_WGS, &kper);
    const dim3 grid((unsigned)a.R, (unsigned)splits);
    const dim3 rows((unsigned)((a.R + 255) / 256));
    const RaggedSegs segs{a.ns, a.seg_off, a.seg_len, a.cap};
    hipLaunchKernelGGL(clear2_u64_kernel, rows, dim3(256), 0, st, (u64*)a.tail_ns, (u64*)a.total_ns, a.R);
    if (a.tail_calls)
        hipLaunchKernelGGL(segment_tail_kernel<true>, grid, dim3(TT_THREADS), 0, st, segs, a, kper);
    else
        hipLaunchKernelGGL(segment_tail_kernel<false>, grid, dim3(TT_THREADS), 0, st, segs, a, kper);
    hipLaunchKernelGGL(segment_tail_finalize_kernel, rows, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace nvrx
