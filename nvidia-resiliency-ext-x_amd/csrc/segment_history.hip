// segment_history.hip -- individual tail scores straight from ragged segments, on gfx950.
//
// No reference counterpart.  histogram_history.hip scores a rank against its own histogram history
// from a dense counts[R][K][240] matrix: 960 B per (rank, kernel), written by
// segment_histogram.hip and read back, next to a history of the same size.  For a fleet that
// arrives as record streams (records.hip) the matrix is 32 GB for 6 GB of records at 16,384 ranks x
// 2,048 kernels.  The scores never need it.  By the ABI's definition, per (rank r, kernel k) with
// history slot s and the retained samples x of segment r K + k,
//     T[r][k]      = the bucket of the history's sample of rank (pm (N - 1)) / 1000   (H alone)
//     total_ns[r]  = sum_k sum_x w(bucket(x)),   tail_ns[r] the same over bucket(x) > T
//     base_total / base_tail: the history's, as histogram_history.hip
//     H[r][s][b]   = min(H + #{x : bucket(x) = b}, 2^32 - 1)                            (UPDATE)
// are integer sums over the samples plus the history's bins, and the update touches only the bins
// the samples fall in.  Segments are addressed as nvrx_segment_histogram_ragged addresses them
// (segment_addr.h): the last `cap` samples retained, seg_len <= 0 an empty element -- not
// eligible, its history slot neither read nor written.
//
//   seghist_kernel     grid (rows, splits of K), 256 threads, the split rule of
//                      histogram_history.hip.  A wave takes one (row, kernel) per trip, SH_UNROLL
//                      in flight: offset, length and slot are wave-uniform; for a non-empty
//                      element 60 lanes load one 16-byte vector of H (the score instantiations;
//                      the update-only one loads only the vectors it changes), the u64 DPP prefix,
//                      a ballot and the walk over one lane's four bins give T.  The retained run is
//                      read 64 consecutive samples per load, SH_LOADS loads in flight, a lane past
//                      the end masked (it loads nothing).  Each lane forms its sample's bucket and
//                      weight: total and tail go into per-lane u64 accumulators that live across
//                      the workgroup's whole trip list, the calls come from a ballot and a
//                      population count.  With UPDATE the element's bins are counted in a
//                      wave-private LDS histogram (cleared per element; the two most frequent
//                      buckets of each 64 samples cost one LDS add each, as count_wave of
//                      segment_tail.hip); each of the 60 lanes then adds its four bins to its H
//                      vector, saturating, and stores it only if one of the four is non-zero.
//                      Row sums: one DPP + LDS reduction per workgroup, the non-zero sums added
//                      to the row's four u64 outputs with 64-bit device atomics (cleared by a
//                      kernel on the stream first).  Integer adds are exact in any order: the
//                      result is the same on every run.
//   tail_score_finalize_kernel<nvrx_seghist_args>   per row the three separately rounded f64
//                      operations of the score and strag (histogram_wave.h, as the clear,
//                      clear4_kernel).
// bucket_of, sat_add, count_wave and slot_of are histogram_wave.h's too, the split rule is
// nvrx_common.h's row_splits.  Every loop is bounded by K or by the retained length.  No kernel
// uses scratch memory (make asm).

#include "histogram_wave.h"
#include "segment_addr.h"

namespace nvrx {
namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_WAVES = SH_THREADS / 64;
constexpr int SH_UNROLL = 4;                     // elements in flight per wave
constexpr int SH_TRIP = SH_WAVES * SH_UNROLL;    // elements per workgroup trip: a split's granule
constexpr int SH_TARGET_WGS = 2048;              // 256 CUs x 8 workgroups
constexpr int SH_LOADS = 4;                      // sample loads in flight per lane
constexpr int SH_HW = 256;                       // LDS words per histogram: 64 lanes x one vector
constexpr unsigned SH_NONE = HB;                 // the bucket of a lane past the run's end
static_assert(SH_HW >= HB + 1 && SH_HW == 4 * NVRX_WAVE, "one 16-byte vector per lane clears it");

// kernels [blockIdx.y * kper, + kper) of row blockIdx.x
template <bool SCORE, bool UPDATE, bool CALLS>
__global__ __launch_bounds__(SH_THREADS)
void seghist_kernel(RaggedSegs segs, nvrx_seghist_args a, int64_t kper) {
    static_assert(SCORE || UPDATE, "nothing to do");
    static_assert(SCORE || !CALLS, "tail_calls belong to the score");
    __shared__ u64 red[SH_WAVES][4];
    __shared__ __attribute__((aligned(16))) unsigned bins[UPDATE ? SH_WAVES * SH_UNROLL * SH_HW : 4];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const int64_t kb = (int64_t)blockIdx.y * kper;
    const int64_t ke = min(K, kb + kper);
    const int64_t stride = a.hist_stride ? a.hist_stride : K;
    const int b0 = 4 * lane;
    const unsigned w0 = weight_of(b0), w1 = weight_of(b0 + 1), w2 = weight_of(b0 + 2),
                   w3 = weight_of(b0 + 3);
    u32x4* hrow = (u32x4*)(a.hist + r * stride * HB) + lane;
    const bool absorb = UPDATE && !(a.skip_rows && a.skip_rows[r]);  // workgroup-uniform
    const int pm = a.permille;
    u64 total = 0, tail = 0, btotal = 0, btail = 0;
    for (int64_t k0 = kb + wave; k0 < ke; k0 += SH_TRIP) {
        u32x4 h[SH_UNROLL];
        int64_t slot[SH_UNROLL];
        const uint32_t* run[SH_UNROLL];
        int len[SH_UNROLL];
#pragma unroll
        for (int u = 0; u < SH_UNROLL; ++u) {
            const int64_t k = k0 + u * SH_WAVES;  // wave-uniform, and so is all that follows from it
            h[u] = (u32x4){0u, 0u, 0u, 0u};
            slot[u] = -1;
            run[u] = nullptr;
            len[u] = 0;
            if (k < ke) {
                int64_t s = slot_of(a, k);
                if (s >= 0) segs.get(r * K + k, run[u], len[u]);
                if (len[u] <= 0) s = -1;  // an empty element: no score, no update, no read of H
                slot[u] = s;
                if (SCORE && s >= 0 && lane < HV) h[u] = hrow[s * HV];
            }
        }
#pragma unroll
        for (int u = 0; u < SH_UNROLL; ++u) {
            const int64_t k = k0 + u * SH_WAVES;
            const int64_t s = slot[u];
            if (s < 0) {  // wave-uniform
                if (CALLS && k < ke && lane == 0) a.tail_calls[r * K + k] = 0u;
                continue;
            }
            const uint32_t* const q = run[u];
            const int m = len[u];
            const u32x4 g = h[u];
            unsigned* const hb = bins + (UPDATE ? (wave * SH_UNROLL + u) * SH_HW : 0);
            const bool count = UPDATE && absorb;
            bool elig = false;
            int t = HB;  // no bucket lies above it
            if (SCORE) {
                // lanes 60..63 hold zeros; N is wave-uniform
                const u64 local = ((u64)g.x + g.y) + ((u64)g.z + g.w);
                const u64 incl = wave_incl_scan_u64(local);
                const u64 N = rl_u64(incl, 63);
                if (N != 0) {
                    elig = true;
                    // (pm (N - 1)) / 1000 without the product leaving 64 bits
                    const u64 d = (N - 1) / 1000ull, mm = (N - 1) % 1000ull;
                    const u64 rank = (u64)pm * d + ((u64)pm * mm) / 1000ull;
                    // incl is non-decreasing and incl[59] = N > rank: the lanes at or below rank
                    // are a prefix
                    const int L = (int)__popcll(__ballot(incl <= rank));
                    u64 e = incl - local;
                    int j = 0;
                    e += g.x;
                    j += e <= rank;
                    e += g.y;
                    j += e <= rank;
                    e += g.z;
                    j += e <= rank;
                    t = (int)rl((unsigned)(b0 + j), L);
                    const bool t0 = b0 > t, t1 = b0 + 1 > t, t2 = b0 + 2 > t, t3 = b0 + 3 > t;
                    const u64 o0 = (u64)g.x * w0, o1 = (u64)g.y * w1, o2 = (u64)g.z * w2,
                              o3 = (u64)g.w * w3;
                    btotal += (o0 + o1) + (o2 + o3);
                    btail += ((t0 ? o0 : 0ull) + (t1 ? o1 : 0ull)) + ((t2 ? o2 : 0ull) + (t3 ? o3 : 0ull));
                }
            }
            if (count) {
                *(u32x4*)(hb + 4 * lane) = (u32x4){0u, 0u, 0u, 0u};
                __builtin_amdgcn_wave_barrier();
            }
            unsigned calls = 0;
            if (elig || count) {  // wave-uniform
                for (int base = 0; base < m; base += 64 * SH_LOADS) {
                    unsigned x[SH_LOADS];
#pragma unroll
                    for (int v = 0; v < SH_LOADS; ++v) {
                        const int i = base + v * 64 + lane;
                        x[v] = i < m ? __builtin_nontemporal_load(q + i) : 0u;
                    }
#pragma unroll
                    for (int v = 0; v < SH_LOADS; ++v) {
                        if (base + v * 64 >= m) break;  // wave-uniform
                        const bool live = base + v * 64 + lane < m;
                        const unsigned b = bucket_of(x[v]);
                        if (SCORE && elig) {
                            const u64 w = live ? (u64)weight_of((int)b) : 0ull;
                            const bool hit = live && (int)b > t;
                            total += w;
                            tail += hit ? w : 0ull;
                            if (CALLS) calls += (unsigned)__popcll(__ballot(hit));
                        }
                        if (count) count_wave<SH_NONE>(live ? b : SH_NONE, hb);
                    }
                }
            }
            if (CALLS && lane == 0) a.tail_calls[r * K + k] = calls;
            if (count) {
                __builtin_amdgcn_wave_barrier();
                const u32x4 c = *(const u32x4*)(hb + 4 * lane);
                if (lane < HV && (c.x | c.y | c.z | c.w) != 0u) {
                    const u32x4 o = SCORE ? g : hrow[s * HV];
                    hrow[s * HV] = (u32x4){sat_add(o.x, c.x), sat_add(o.y, c.y), sat_add(o.z, c.z),
                                           sat_add(o.w, c.w)};
                }
            }
        }
    }
    if (!SCORE) return;  // the update-only instantiation has no barrier
    total = wave_sum_u64(total);
    tail = wave_sum_u64(tail);
    btotal = wave_sum_u64(btotal);
    btail = wave_sum_u64(btail);
    if (lane == 0) {
        red[wave][0] = tail;
        red[wave][1] = total;
        red[wave][2] = btail;
        red[wave][3] = btotal;
    }
    __syncthreads();
    if (threadIdx.x >= 4) return;
    u64 v = 0;
#pragma unroll
    for (int w = 0; w < SH_WAVES; ++w) v += red[w][threadIdx.x];
    uint64_t* const dst = threadIdx.x == 0 ? a.tail_ns : threadIdx.x == 1 ? a.total_ns
                        : threadIdx.x == 2 ? a.base_tail_ns : a.base_total_ns;
    if (v) atomicAdd((u64*)dst + r, v);
}

template <bool SCORE, bool UPDATE, bool CALLS>
void launch_seghist(const nvrx_seghist_args& a, dim3 grid, int64_t kper, hipStream_t st) {
    hipLaunchKernelGGL((seghist_kernel<SCORE, UPDATE, CALLS>), grid, dim3(SH_THREADS), 0, st,
                       RaggedSegs{a.ns, a.seg_off, a.seg_len, a.cap}, a, kper);
}

}  // namespace

// Argument checks happen in abi.cpp before this runs.
hipError_t segment_history_scores_ragged(const nvrx_seghist_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    const bool score = a.mode & NVRX_HTAIL_SCORE, update = a.mode & NVRX_HTAIL_UPDATE;
    int64_t kper;
    const int64_t splits = row_splits(a.R, a.K, SH_TRIP, SH_TARGET_WGS, &kper);
    const dim3 grid((unsigned)a.R, (unsigned)splits);
    const dim3 rows((unsigned)((a.R + 255) / 256));
    if (score)
        hipLaunchKernelGGL(clear4_kernel<u64>, rows, dim3(256), 0, st, (u64*)a.tail_ns,
                           (u64*)a.total_ns, (u64*)a.base_tail_ns, (u64*)a.base_total_ns, a.R);
    if (!score)
        launch_seghist<false, true, false>(a, grid, kper, st);
    else if (update)
        a.tail_calls ? launch_seghist<true, true, true>(a, grid, kper, st)
                     : launch_seghist<true, true, false>(a, grid, kper, st);
    else
        a.tail_calls ? launch_seghist<true, false, true>(a, grid, kper, st)
                     : launch_seghist<true, false, false>(a, grid, kper, st);
    if (score)
        hipLaunchKernelGGL(tail_score_finalize_kernel<nvrx_seghist_args>, rows, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace nvrx
