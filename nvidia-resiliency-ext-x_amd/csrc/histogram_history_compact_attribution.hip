// histogram_history_compact_attribution.hip -- individual tail score attribution of [R][K][240]
// counts against a compact history, on gfx950.
//
// No reference counterpart.  histogram_attribution.hip names the kernels behind an individual tail
// score from the counts and the dense history of 960 B per (rank, kernel);
// segment_history_compact_attribution.hip does so from record streams against the compact history
// of 64 B per element (include/nvrx_straggler.h, "compact history": u32 count[12], u8 bucket[12],
// u32 n).  Here the interval arrives as counts and the history is compact: the fourth corner.  It
// adds no definition: every output is what nvrx_histogram_tail_attribution writes with kind =
// NVRX_ATTR_INDIVIDUAL and hist the dense expansion of chist (H[bucket[i]] = count[i] for i < n,
// zero elsewhere): per (rank r, kernel k) with slot s,
//     T      = the bucket of the entry that holds the history's sample of rank (pm (N - 1)) / 1000
//     btail  = sum_{i : bucket[i] > T} count[i] w(bucket[i])    btotal = sum_i count[i] w(bucket[i])
//     tail   = sum_{b > T} C[r][k][b] w(b)                      total  = sum_b C[r][k][b] w(b)
//     loss   = tail - total * (btail / btotal)                                      (f64, ns)
// integer sums plus three f64 operations.  chist is read only.  Two kernels:
//
//   histchist_loss_kernel    grid (rows, splits of K), 256 threads, the split rule and the
//          16-element workgroup trip of histchist_kernel.  A wave takes the HCA_UNROLL = 4
//          consecutive kernels from k0 + 4 wave, as segchist_loss_kernel does, so that their losses
//          are neighbours in loss_all, and loads their elements with ONE instruction: DPP row u
//          (lanes 16u..16u+15) holds element u, one dword per lane (chist_wave.h).  A row whose
//          kernel is >= K, not valid or without a slot is not loaded (its word is 0: the empty
//          history), and neither is its C.  60 lanes load each element's 16-byte vector of C,
//          nontemporal, the four loads in flight together: lane l owns bins 4l..4l+3 with weights
//          that are constants of the launch.  Inside the rows, side by side for the four elements
//          (rows_base): the bpermute for the bucket byte, the u64 row_shr prefix, one ballot and a
//          readlane for T, the row sums for btotal and btail.  tail and total are per-lane u64
//          values against the wave-uniform T: two wave reductions per element (the dense
//          individual kernel pays four, and a prefix), the four elements' reductions next to each
//          other as independent DPP chains.  The three f64 operations (`excess`) finish each loss,
//          lane u keeps the loss of element u and lanes 0..3 store the trip's losses with one
//          32-byte store.  NaN where the element is not taken: loss_all is written in full, no
//          clear.
//   histchist_select_kernel  one 256-thread workgroup per row over loss_all[r][:]: the select of
//          topk_select.h.  Then wave v recomputes winners v, v + 4, ... from the winner's 64-byte
//          element (row 0 of rows_base, the other rows empty) and its vector of C with the same
//          arithmetic and `excess`, the calls from a wave_sum_u32, and lane 0 stores every
//          per-winner output.  What is stored comes from the inputs, the key only orders.
// Every (r, k) has one owner: no atomics, no scratch, no clear, no LDS in the loss kernel.
// slot_of, lane_bins and `excess` are histogram_wave.h's, rows_base chist_wave.h's; the select's
// first half (NVRX_TOPK_WINNERS), the winner's stores and the choice of TOP are topk_select.h's.
// Every loop is bounded by K, 4 or top.  No kernel uses scratch memory (make asm).

#include "chist_wave.h"
#include "topk_select.h"

namespace nvrx {
namespace {

constexpr int HCA_THREADS = 256;
constexpr int HCA_WAVES = HCA_THREADS / 64;
constexpr int HCA_UNROLL = CH_ROWS;                  // elements per wave trip: one per DPP row
constexpr int HCA_TRIP = HCA_WAVES * HCA_UNROLL;     // elements per workgroup trip: a split's granule
constexpr int HCA_TARGET_WGS = 2048;                 // 256 CUs x 8 workgroups

// A lane's part of one element's sums: its four bins of C against the threshold bucket t.
struct BinSums {
    u64 tail, total;
};
__device__ __forceinline__ BinSums bin_sums(const u32x4 q, int t, const LaneBins& w) {
    const bool t0 = w.b0 > t, t1 = w.b0 + 1 > t, t2 = w.b0 + 2 > t, t3 = w.b0 + 3 > t;
    const u64 p0 = (u64)q.x * w.w0, p1 = (u64)q.y * w.w1, p2 = (u64)q.z * w.w2, p3 = (u64)q.w * w.w3;
    BinSums s;
    s.total = (p0 + p1) + (p2 + p3);
    s.tail = ((t0 ? p0 : 0ull) + (t1 ? p1 : 0ull)) + ((t2 ? p2 : 0ull) + (t3 ? p3 : 0ull));
    return s;
}

// kernels [blockIdx.y * kper, + kper) of row blockIdx.x
__global__ __launch_bounds__(HCA_THREADS)
void histchist_loss_kernel(nvrx_histchistattr_args a, int64_t kper) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int row = lane >> 4, j = lane & 15;  // the element of the trip this lane holds a word of
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const int64_t kb = (int64_t)blockIdx.y * kper;
    const int64_t ke = min(K, kb + kper);
    const int64_t stride = a.hist_stride ? a.hist_stride : K;
    const LaneBins w = lane_bins(lane);
    const u32x4* const crow = (const u32x4*)(a.counts + r * K * HB) + lane;
    const unsigned* const hrow = (const unsigned*)a.chist + r * stride * CH_WORDS;
    double* const out = a.loss_all + r * K;
    const int pm = a.permille;
    const double qnan = __builtin_nan("");
    for (int64_t k0 = kb + wave * HCA_UNROLL; k0 < ke; k0 += HCA_TRIP) {  // wave-uniform
        u32x4 c[HCA_UNROLL];
        int64_t slot[HCA_UNROLL];
        // the four slots first (a kernel past the split reads the split's last column and is
        // dropped), so that no load of C waits for the slot of the element before it
#pragma unroll
        for (int u = 0; u < HCA_UNROLL; ++u) {
            const int64_t k = k0 + u;  // wave-uniform, and so is all that follows from it
            const int64_t s = slot_of(a, min(k, ke - 1));
            slot[u] = k < ke ? s : -1;
        }
#pragma unroll
        for (int u = 0; u < HCA_UNROLL; ++u) {
            c[u] = (u32x4){0u, 0u, 0u, 0u};
            if (slot[u] >= 0 && lane < HV) c[u] = __builtin_nontemporal_load(crow + (k0 + u) * HV);
        }
        // the trip's four elements in one load: row u, word j
        const int64_t sl = by_row(row, slot[0], slot[1], slot[2], slot[3]);
        const unsigned word = sl >= 0 ? hrow[sl * CH_WORDS + j] : 0u;
        const RowBase base = rows_base(word, pm, lane);
        BinSums p[HCA_UNROLL];
        bool take[HCA_UNROLL];
#pragma unroll
        for (int u = 0; u < HCA_UNROLL; ++u) {
            const u32x4 q = c[u];
            // lanes 60..63 hold zeros; an interval without samples is not taken
            take[u] = base.elig[u] && __ballot((q.x | q.y | q.z | q.w) != 0u) != 0ull;  // wave-uniform
            p[u] = bin_sums(q, base.T[u], w);
        }
        double loss = qnan;
        // the reductions are independent of each other
#pragma unroll
        for (int u = 0; u < HCA_UNROLL; ++u) {
            const u64 tail = wave_sum_u64(p[u].tail), total = wave_sum_u64(p[u].total);
            const u64 bl = rl_u64(base.btail, 16 * u), bt = rl_u64(base.btotal, 16 * u);
            double share;
            const double v = excess(tail, total, bl, bt, share);
            if (lane == u) loss = take[u] && v == v ? v : qnan;
        }
        if (lane < HCA_UNROLL && k0 + lane < ke) out[k0 + lane] = loss;
    }
}

template <int TOP>
__global__ __launch_bounds__(256)
void histchist_select_kernel(nvrx_histchistattr_args a) {
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const double* __restrict__ row = a.loss_all + r * K;
    const int top = a.top < TOP ? a.top : TOP;
    NVRX_TOPK_WINNERS(TOP, row, K, top, win);

    // wave v recomputes winners v, v + 4, ... from the element and the counts and stores their
    // outputs
    const int64_t stride = a.hist_stride ? a.hist_stride : K;
    const LaneBins w = lane_bins(lane);
    const u32x4* const crow = (const u32x4*)(a.counts + r * K * HB) + lane;
    const unsigned* const hrow = (const unsigned*)a.chist + r * stride * CH_WORDS;
    for (int j = wave; j < top; j += 4) {
        const int col = __builtin_amdgcn_readfirstlane(win[j]);
        u64 tail = 0, total = 0;
        unsigned calls = 0;
        int T = -1;
        double share = __builtin_nan(""), loss = share;
        if (col >= 0) {  // wave-uniform, as everything up to the stores
            const int64_t s = slot_of(a, (int64_t)col);
            if (s >= 0) {
                u32x4 q = (u32x4){0u, 0u, 0u, 0u};
                if (lane < HV) q = __builtin_nontemporal_load(crow + (int64_t)col * HV);
                // the winner's element in row 0, the empty history in the other rows
                const unsigned word = lane < CH_WORDS ? hrow[s * CH_WORDS + lane] : 0u;
                const RowBase base = rows_base(word, a.permille, lane);
                if (base.elig[0] && __ballot((q.x | q.y | q.z | q.w) != 0u) != 0ull) {
                    T = base.T[0];
                    const BinSums p = bin_sums(q, T, w);
                    tail = wave_sum_u64(p.tail);
                    total = wave_sum_u64(p.total);
                    const bool t0 = w.b0 > T, t1 = w.b0 + 1 > T, t2 = w.b0 + 2 > T, t3 = w.b0 + 3 > T;
                    calls = wave_sum_u32(((t0 ? q.x : 0u) + (t1 ? q.y : 0u)) +
                                         ((t2 ? q.z : 0u) + (t3 ? q.w : 0u)));
                    const u64 bl = rl_u64(base.btail, 0), bt = rl_u64(base.btotal, 0);
                    loss = excess(tail, total, bl, bt, share);
                }
            }
        }
        if (lane != 0) continue;
        store_winner(a, r * a.top + j, loss == loss, col, loss, tail, total, calls, T, share);
    }
}

}  // namespace

// Argument checks happen in abi.cpp before this runs.
hipError_t histogram_history_attribution_compact(const nvrx_histchistattr_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    if (a.top < 1 || a.top > NVRX_MAX_ATTRIBUTION) return hipErrorInvalidValue;
    int64_t kper;
    const int64_t splits = row_splits(a.R, a.K, HCA_TRIP, HCA_TARGET_WGS, &kper);
    const dim3 grid((unsigned)a.R, (unsigned)splits);
    const dim3 rows((unsigned)a.R), b(256);
    hipLaunchKernelGGL(histchist_loss_kernel, grid, dim3(HCA_THREADS), 0, st, a, kper);
    dispatch_top(a.top, [&](auto t) {
        hipLaunchKernelGGL(histchist_select_kernel<decltype(t)::value>, rows, b, 0, st, a);
    });
    return hipGetLastError();
}

}  // namespace nvrx
