// segment_history_compact_attribution.hip -- individual tail score attribution straight from
// ragged segments against a compact history, on gfx950.
//
// No reference counterpart.  segment_history_attribution.hip names the kernels behind an
// individual tail score from the bucketed samples and the dense history of 960 B per (rank,
// kernel); segment_history_compact.hip scores against a compact history of 64 B per element
// (include/nvrx_straggler.h, "compact history": u32 count[12], u8 bucket[12], u32 n).  This file
// attributes against that compact history.  By definition every output is what
// nvrx_segment_history_attribution_ragged writes with hist the dense expansion of chist
// (H[bucket[i]] = count[i] for i < n, zero elsewhere): per (rank r, kernel k) with slot s,
//     T      = the bucket of the entry that holds the history's sample of rank (pm (N - 1)) / 1000
//     btail  = sum_{i : bucket[i] > T} count[i] w(bucket[i])    btotal = sum_i count[i] w(bucket[i])
//     tail   = sum_{x : bucket(x) > T} w(bucket(x))             total  = sum_x w(bucket(x))
//     loss   = tail - total * (btail / btotal)                                      (f64, ns)
// integer sums plus three f64 operations.  chist is read only.  Two kernels:
//
//   segchist_loss_kernel    grid (rows, splits of K), 256 threads, the split rule and the
//          16-element workgroup trip of segchist_kernel / seghist_loss_kernel.  A wave takes the
//          SCA_UNROLL = 4 consecutive kernels from k0 + 4 wave, so that their losses are
//          neighbours in loss_all, and loads their elements with ONE instruction: DPP row u
//          (lanes 16u..16u+15) holds element u, one dword per lane -- lanes 0..11 a count, 12..14
//          the bucket bytes, 15 n; the row's address comes from its own slot.  A row whose kernel
//          is >= K, not valid, without a slot or whose segment is empty is not loaded (its word is
//          0: the empty history).  Inside the rows, side by side for the four elements
//          (rows_base): a bpermute hands each count lane its bucket byte; the u64 row_shr prefix
//          gives N in the row's last lane and the rank by the 64-bit split; a ballot gives the
//          entry that holds the rank and a readlane its bucket T; count * weight_of(bucket) per
//          lane, reduced in the row by four DPP steps, gives btotal and btail.  The retained run
//          is walked as in segment_history_attribution.hip (walk): 64 samples per load, SCA_LOADS
//          loads in flight, a lane past the end masked, per-lane u64 tail / total.  The partial
//          sums of the four elements are kept until all their samples are read; then their u64
//          wave reductions stand next to each other as independent DPP chains, the three f64
//          operations finish each loss, lane u keeps the loss of element u and lanes 0..3 store
//          the trip's losses with one 32-byte store.  NaN where the element is not taken:
//          loss_all is written in full, no clear.
//   segchist_select_kernel  one 256-thread workgroup per row over loss_all[r][:]: the scheme of
//          seghist_select_kernel (topk_select.h).  Then wave v recomputes winners v, v + 4, ...
//          from the winner's 64-byte element (row 0 of rows_base, the other rows empty) and its
//          samples with the same two functions and `excess`, the calls from a ballot and a
//          population count, and lane 0 stores every per-winner output.  What is stored comes
//          from the inputs, the key only orders.
// Every (r, k) has one owner: no atomics, no scratch, no clear, no LDS in the loss kernel.
// bucket_of, slot_of and `excess` are histogram_wave.h's, rows_base (with RowBase, row_sum_u64 and
// by_row, shared with histogram_history_compact_attribution.hip) chist_wave.h's; the
// select's first half (NVRX_TOPK_WINNERS), the winner's stores and the choice of TOP are
// topk_select.h's.  Every loop is bounded by K or a retained length (an element's 12 entries are
// lanes, not iterations).  No kernel uses scratch memory (make asm).

#include "chist_wave.h"
#include "segment_addr.h"
#include "topk_select.h"

namespace nvrx {
namespace {

constexpr int SCA_THREADS = 256;
constexpr int SCA_WAVES = SCA_THREADS / 64;
constexpr int SCA_UNROLL = 4;                      // elements per wave trip: one per DPP row
constexpr int SCA_TRIP = SCA_WAVES * SCA_UNROLL;   // elements per workgroup trip: a split's granule
constexpr int SCA_TARGET_WGS = 2048;               // 256 CUs x 8 workgroups
constexpr int SCA_LOADS = 4;                       // sample loads in flight per lane
constexpr int SCA_E = NVRX_CHIST_ENTRIES;
constexpr int SCA_WORDS = NVRX_CHIST_BYTES / 4;    // 16: one DPP row
static_assert(SCA_WORDS == 16 && SCA_UNROLL * SCA_WORDS == NVRX_WAVE, "an element is one DPP row");
static_assert(4 * SCA_E + SCA_E + 4 == NVRX_CHIST_BYTES, "count[12], bucket[12], n");

// One element's samples before the wave reductions: the lane's part of tail / total over the
// retained run q of m > 0 samples against the threshold bucket t.  CALLS adds the count above t.
struct Walk {
    u64 tail, total;
    unsigned calls;
};
template <bool CALLS>
__device__ __forceinline__ Walk walk(const uint32_t* q, int m, int t, int lane) {
    Walk p = {0ull, 0ull, 0u};
    for (int base = 0; base < m; base += 64 * SCA_LOADS) {
        unsigned x[SCA_LOADS];
#pragma unroll
        for (int v = 0; v < SCA_LOADS; ++v) {
            const int i = base + v * 64 + lane;
            x[v] = i < m ? __builtin_nontemporal_load(q + i) : 0u;
        }
#pragma unroll
        for (int v = 0; v < SCA_LOADS; ++v) {
            if (base + v * 64 >= m) break;  // wave-uniform
            const bool live = base + v * 64 + lane < m;
            const unsigned b = bucket_of(x[v]);
            const u64 wt = live ? (u64)weight_of((int)b) : 0ull;
            const bool hit = live && (int)b > t;
            p.total += wt;
            p.tail += hit ? wt : 0ull;
            if (CALLS) p.calls += (unsigned)__popcll(__ballot(hit));
        }
    }
    return p;
}

// kernels [blockIdx.y * kper, + kper) of row blockIdx.x
__global__ __launch_bounds__(SCA_THREADS)
void segchist_loss_kernel(RaggedSegs segs, nvrx_segchistattr_args a, int64_t kper) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int row = lane >> 4, j = lane & 15;  // the element of the trip this lane holds a word of
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const int64_t kb = (int64_t)blockIdx.y * kper;
    const int64_t ke = min(K, kb + kper);
    const int64_t stride = a.hist_stride ? a.hist_stride : K;
    const unsigned* const crow = (const unsigned*)a.chist + r * stride * SCA_WORDS;
    double* const out = a.loss_all + r * K;
    const int pm = a.permille;
    const double qnan = __builtin_nan("");
    for (int64_t k0 = kb + wave * SCA_UNROLL; k0 < ke; k0 += SCA_TRIP) {  // wave-uniform
        int64_t slot[SCA_UNROLL];
        const uint32_t* run[SCA_UNROLL];
        int len[SCA_UNROLL];
#pragma unroll
        for (int u = 0; u < SCA_UNROLL; ++u) {
            const int64_t k = k0 + u;  // wave-uniform, and so is all that follows from it
            slot[u] = -1;
            run[u] = nullptr;
            len[u] = 0;
            if (k < ke) {
                int64_t s = slot_of(a, k);
                if (s >= 0) segs.get(r * K + k, run[u], len[u]);
                if (len[u] <= 0) {  // an empty element: no loss, no read of the history
                    len[u] = 0;
                    s = -1;
                }
                slot[u] = s;
            }
        }
        // the trip's four elements in one load: row u, word j
        const int64_t sl = by_row(row, slot[0], slot[1], slot[2], slot[3]);
        const unsigned word = sl >= 0 ? crow[sl * SCA_WORDS + j] : 0u;
        const RowBase base = rows_base(word, pm, lane);
        Walk p[SCA_UNROLL];
        bool any = false;
#pragma unroll
        for (int u = 0; u < SCA_UNROLL; ++u) {
            p[u] = Walk{0ull, 0ull, 0u};
            if (base.elig[u]) p[u] = walk<false>(run[u], len[u], base.T[u], lane);  // len > 0
            any |= base.elig[u];
        }
        double loss = qnan;
        if (any) {  // wave-uniform; the reductions are independent of each other
#pragma unroll
            for (int u = 0; u < SCA_UNROLL; ++u) {
                const u64 tail = wave_sum_u64(p[u].tail), total = wave_sum_u64(p[u].total);
                const u64 bl = rl_u64(base.btail, 16 * u), bt = rl_u64(base.btotal, 16 * u);
                double share;
                const double v = excess(tail, total, bl, bt, share);
                if (lane == u) loss = base.elig[u] && v == v ? v : qnan;
            }
        }
        if (lane < SCA_UNROLL && k0 + lane < ke) out[k0 + lane] = loss;
    }
}

template <int TOP>
__global__ __launch_bounds__(256)
void segchist_select_kernel(RaggedSegs segs, nvrx_segchistattr_args a) {
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const double* __restrict__ row = a.loss_all + r * K;
    const int top = a.top < TOP ? a.top : TOP;
    NVRX_TOPK_WINNERS(TOP, row, K, top, win);

    // wave v recomputes winners v, v + 4, ... from the element and the samples and stores their
    // outputs
    const int64_t stride = a.hist_stride ? a.hist_stride : K;
    const unsigned* const crow = (const unsigned*)a.chist + r * stride * SCA_WORDS;
    for (int j = wave; j < top; j += 4) {
        const int col = __builtin_amdgcn_readfirstlane(win[j]);
        u64 tail = 0, total = 0;
        unsigned calls = 0;
        int T = -1;
        double share = __builtin_nan(""), loss = share;
        if (col >= 0) {  // wave-uniform, as everything up to the stores
            const int64_t s = slot_of(a, (int64_t)col);
            const uint32_t* q = nullptr;
            int m = 0;
            if (s >= 0) segs.get(r * K + col, q, m);
            if (m > 0) {
                // the winner's element in row 0, the empty history in the other rows
                const unsigned word = lane < SCA_WORDS ? crow[s * SCA_WORDS + lane] : 0u;
                const RowBase base = rows_base(word, a.permille, lane);
                if (base.elig[0]) {
                    const Walk p = walk<true>(q, m, base.T[0], lane);
                    tail = wave_sum_u64(p.tail);
                    total = wave_sum_u64(p.total);
                    const u64 bl = rl_u64(base.btail, 0), bt = rl_u64(base.btotal, 0);
                    calls = p.calls;
                    T = base.T[0];
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
hipError_t segment_history_attribution_compact_ragged(const nvrx_segchistattr_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    if (a.top < 1 || a.top > NVRX_MAX_ATTRIBUTION) return hipErrorInvalidValue;
    int64_t kper;
    const int64_t splits = row_splits(a.R, a.K, SCA_TRIP, SCA_TARGET_WGS, &kper);
    const dim3 grid((unsigned)a.R, (unsigned)splits);
    const dim3 rows((unsigned)a.R), b(256);
    const RaggedSegs segs{a.ns, a.seg_off, a.seg_len, a.cap};
    hipLaunchKernelGGL(segchist_loss_kernel, grid, dim3(SCA_THREADS), 0, st, segs, a, kper);
    dispatch_top(a.top, [&](auto t) {
        hipLaunchKernelGGL(segchist_select_kernel<decltype(t)::value>, rows, b, 0, st, segs, a);
    });
    return hipGetLastError();
}

}  // namespace nvrx
