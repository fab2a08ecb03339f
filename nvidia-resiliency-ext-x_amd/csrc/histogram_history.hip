// histogram_history.hip -- individual tail scores: a rank against its own histogram history, gfx950.
//
// No reference counterpart.  histogram_scores.hip compares a rank's tail with the fleet's in the
// same report; a world of one, a degradation that hits every rank together, or a large share of
// slow ranks is invisible there.  Here the yardstick is the rank's own past: hist[R][stride][240]
// holds, per (rank, slot), the u32 counts of the intervals absorbed so far, over the same 240
// buckets as counts[R][K][240].  Per (rank r, kernel k) with slot s, in exact integers:
//     N            = sum_b H[r][s][b]      (before this call)       n = sum_b C[r][k][b]
//     T[r][k]      = the bucket of the history's sample of rank (pm (N - 1)) / 1000
//     total_ns[r]  = sum_k sum_b       C w(b)        base_total[r] = sum_k sum_b       H w(b)
//     tail_ns[r]   = sum_k sum_{b>T}   C w(b)        base_tail[r]  = sum_k sum_{b>T}   H w(b)
//     score[r]     = (1 - tail_ns / total_ns) / (1 - base_tail / base_total)               (f64)
//     H[r][s][b]   = min(H + C, 2^32 - 1)                                               (UPDATE)
// over the kernels with a slot, col_valid, N > 0 and n > 0 (include/nvrx_straggler.h has the full
// definition).  One fused pass:
//
//   history_kernel       grid (rows, splits of K), 256 threads.  A wave takes one (row, kernel) per
//                        trip: 60 lanes load one 16-byte vector of C and one of H, so a lane's four
//                        weights are constants of the whole kernel; the u64 DPP inclusive prefix of
//                        the lanes' H sums locates the lane of the rank (ballot), the walk over that
//                        lane's four bins the bucket; four u64 accumulators per lane are fed by
//                        32x32->64 multiplies; with UPDATE the saturated sum goes back as one
//                        16-byte store.  The prefix is a dependent chain per kernel: HH_UNROLL
//                        kernels per wave are in flight.  SCORE, UPDATE and CALLS are template
//                        flags: the update-only instantiation carries no scan, the score-only one
//                        no store.  One DPP + LDS reduction per workgroup, then its non-zero sums
//                        are added to the row's four u64 outputs with 64-bit device atomics -- the
//                        outputs are the accumulators, cleared by a kernel on the stream first.
//                        Integer adds are exact in any order: the result is the same on every run.
//   tail_score_finalize_kernel<nvrx_histtail_args>   per row the three f64 operations of the
//                        score and strag (histogram_wave.h, as the clear, clear4_kernel).
// The split of K exists because rows alone do not fill the device: Detector calls this with R = 1.
// Every loop is bounded by K.  No kernel uses scratch memory (make asm).

#include "histogram_wave.h"

namespace nvrx {
namespace {

constexpr int HH_THREADS = 256;
constexpr int HH_WAVES = HH_THREADS / 64;
constexpr int HH_UNROLL = 4;                     // kernels in flight per wave
constexpr int HH_TRIP = HH_WAVES * HH_UNROLL;    // kernels per workgroup trip: a split's granule
constexpr int HH_TARGET_WGS = 2048;              // 256 CUs x 8 workgroups

// kernels [blockIdx.y * kper, + kper) of row blockIdx.x
template <bool SCORE, bool UPDATE, bool CALLS>
__global__ __launch_bounds__(HH_THREADS) void history_kernel(nvrx_histtail_args a, int64_t kper) {
    static_assert(SCORE || UPDATE, "nothing to do");
    static_assert(SCORE || !CALLS, "tail_calls belong to the score");
    __shared__ u64 red[HH_WAVES][4];
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
    const u32x4* crow = (const u32x4*)(a.counts + r * K * HB) + lane;
    u32x4* hrow = (u32x4*)(a.hist + r * stride * HB) + lane;
    const bool absorb = UPDATE && !(a.skip_rows && a.skip_rows[r]);  // workgroup-uniform
    const int pm = a.permille;
    u64 total = 0, tail = 0, btotal = 0, btail = 0;
    for (int64_t k0 = kb + wave; k0 < ke; k0 += HH_TRIP) {
        u32x4 c[HH_UNROLL], h[HH_UNROLL];
        int64_t slot[HH_UNROLL];
#pragma unroll
        for (int u = 0; u < HH_UNROLL; ++u) {
            const int64_t k = k0 + u * HH_WAVES;  // wave-uniform
            c[u] = (u32x4){0u, 0u, 0u, 0u};
            h[u] = (u32x4){0u, 0u, 0u, 0u};
            slot[u] = -1;
            if (k < ke) {
                int64_t s = a.hist_index ? (int64_t)a.hist_index[k] : k;
                if (a.col_valid && !a.col_valid[k]) s = -1;
                slot[u] = s;
                if (s >= 0 && lane < HV) {
                    c[u] = __builtin_nontemporal_load(crow + k * HV);
                    h[u] = hrow[s * HV];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < HH_UNROLL; ++u) {
            const int64_t k = k0 + u * HH_WAVES;
            const int64_t s = slot[u];
            const u32x4 q = c[u], g = h[u];
            if (SCORE) {
                unsigned calls = 0;
                // lanes 60..63 hold zeros; N and n > 0 are wave-uniform
                const u64 local = ((u64)g.x + g.y) + ((u64)g.z + g.w);
                const u64 incl = wave_incl_scan_u64(local);
                const u64 N = rl_u64(incl, 63);
                const bool any = __ballot((q.x | q.y | q.z | q.w) != 0u) != 0ull;
                if (s >= 0 && N != 0 && any) {
                    // (pm (N - 1)) / 1000 without the product leaving 64 bits
                    const u64 d = (N - 1) / 1000ull, m = (N - 1) % 1000ull;
                    const u64 rank = (u64)pm * d + ((u64)pm * m) / 1000ull;
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
                    const int t = (int)rl((unsigned)(b0 + j), L);
                    const bool t0 = b0 > t, t1 = b0 + 1 > t, t2 = b0 + 2 > t, t3 = b0 + 3 > t;
                    const u64 p0 = (u64)q.x * w0, p1 = (u64)q.y * w1, p2 = (u64)q.z * w2,
                              p3 = (u64)q.w * w3;
                    const u64 o0 = (u64)g.x * w0, o1 = (u64)g.y * w1, o2 = (u64)g.z * w2,
                              o3 = (u64)g.w * w3;
                    total += (p0 + p1) + (p2 + p3);
                    tail += ((t0 ? p0 : 0ull) + (t1 ? p1 : 0ull)) + ((t2 ? p2 : 0ull) + (t3 ? p3 : 0ull));
                    btotal += (o0 + o1) + (o2 + o3);
                    btail += ((t0 ? o0 : 0ull) + (t1 ? o1 : 0ull)) + ((t2 ? o2 : 0ull) + (t3 ? o3 : 0ull));
                    if (CALLS)
                        calls = wave_sum_u32(((t0 ? q.x : 0u) + (t1 ? q.y : 0u)) +
                                             ((t2 ? q.z : 0u) + (t3 ? q.w : 0u)));
                }
                if (CALLS && k < ke && lane == 0) a.tail_calls[r * K + k] = calls;
            }
            if (UPDATE) {
                if (absorb && s >= 0 && lane < HV)
                    hrow[s * HV] = (u32x4){sat_add(g.x, q.x), sat_add(g.y, q.y), sat_add(g.z, q.z),
                                           sat_add(g.w, q.w)};
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
    for (int w = 0; w < HH_WAVES; ++w) v += red[w][threadIdx.x];
    uint64_t* const dst = threadIdx.x == 0 ? a.tail_ns : threadIdx.x == 1 ? a.total_ns
                        : threadIdx.x == 2 ? a.base_tail_ns : a.base_total_ns;
    if (v) atomicAdd((u64*)dst + r, v);
}

template <bool SCORE, bool UPDATE, bool CALLS>
void launch_history(const nvrx_histtail_args& a, dim3 grid, int64_t kper, hipStream_t st) {
    hipLaunchKernelGGL((history_kernel<SCORE, UPDATE, CALLS>), grid, dim3(HH_THREADS), 0, st, a, kper);
}

}  // namespace

// Argument checks happen in abi.cpp before this runs.
hipError_t histogram_history_scores(const nvrx_histtail_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    const bool score = a.mode & NVRX_HTAIL_SCORE, update = a.mode & NVRX_HTAIL_UPDATE;
    int64_t kper;
    const int64_t splits = row_splits(a.R, a.K, HH_TRIP, HH_TARGET_WGS, &kper);
    const dim3 grid((unsigned)a.R, (unsigned)splits);
    if (score)
        hipLaunchKernelGGL(clear4_kernel<u64>, dim3((unsigned)((a.R + 255) / 256)), dim3(256), 0, st,
                           (u64*)a.tail_ns, (u64*)a.total_ns, (u64*)a.base_tail_ns,
                           (u64*)a.base_total_ns, a.R);
    if (!score)
        launch_history<false, true, false>(a, grid, kper, st);
    else if (update)
        a.tail_calls ? launch_history<true, true, true>(a, grid, kper, st)
                     : launch_history<true, true, false>(a, grid, kper, st);
    else
        a.tail_calls ? launch_history<true, false, true>(a, grid, kper, st)
                     : launch_history<true, false, false>(a, grid, kper, st);
    if (score)
        hipLaunchKernelGGL(tail_score_finalize_kernel<nvrx_histtail_args>, dim3((unsigned)((a.R + 255) / 256)), dim3(256),
                           0, st, a);
    return hipGetLastError();
}

}  // namespace nvrx
