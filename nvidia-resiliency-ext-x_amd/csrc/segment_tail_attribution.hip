// segment_tail_attribution.hip -- tail score attribution straight from ragged segments, on gfx950.
//
// No reference counterpart.  segment_tail.hip gives the tail scores of record streams without the
// counts[R][K][240] matrix; histogram_attribution.hip names the kernels behind a tail score, but
// from that matrix.  The loss of the relative leg is made of exact integer sums over a segment's
// samples and three f64 operations,
//     tail  = sum_{x : bucket(x) > T} w(bucket(x))      total = sum_x w(bucket(x))
//     loss  = tail - total * (btail / btotal)                                     (f64, ns)
// over the retained window of segment r K + k, with T = thr[u], {btail, btotal} = base[u] and
// u = thr_index ? thr_index[k] : k, so it needs the matrix no more than the scores do: by
// definition the outputs are what nvrx_histogram_tail_attribution(NVRX_ATTR_RELATIVE) writes on
// the counts nvrx_segment_histogram_ragged would put into a zeroed matrix (include/
// nvrx_straggler.h).  Segments are addressed as there (segment_addr.h).  Two kernels:
//
//   segment_loss_kernel     grid (rows, splits of K), the split rule and 256-column granule of
//          segment_tail_kernel.  A lane takes a column per trip, so seg_off / seg_len / thr_index /
//          base of a row are coalesced reads.  The two treatments of segment_tail.hip: a retained
//          run <= ST_LANE_MAX is walked by its lane alone, four loads in flight, and the lane
//          finishes its loss itself; longer runs are taken by the whole wave one after the other
//          (ballot), per-lane u64 accumulators, two u64 wave reductions and one loss per segment,
//          kept by the segment's lane.  The wave's 64 losses go out as one coalesced f64 store,
//          NaN where the element is not taken: loss_all is written in full, no clear.
//   segment_select_kernel   one 256-thread workgroup per row over loss_all[r][:]: the scheme of
//          tail_select_kernel (topk_select.h: sorted candidates in registers, `top` rounds of DPP +
//          LDS argmax).  Then wave v recomputes winners v, v + 4, ... from the samples with the
//          wave treatment (valid for any length >= 1: a lane past the end re-reads the last sample
//          and is masked) and lane 0 stores every per-winner output.  What is stored comes from
//          the inputs, the key only orders; integer sums do not depend on their order, so the
//          recomputed loss is the loss that ranked the winner.
// Every (r, k) has one owner: no atomics, no scratch, no clear.  Every loop is bounded by a
// segment length or K.  No kernel uses scratch memory (make asm).

#include "histogram_wave.h"
#include "segment_addr.h"
#include "topk_select.h"

namespace nvrx {
namespace {

constexpr int SA_THREADS = 256;
constexpr int SA_WAVES = SA_THREADS / 64;
constexpr int SA_TRIP = SA_THREADS;  // columns per workgroup trip: a split's granule
constexpr int SA_TARGET_WGS = 2048;  // 256 CUs x 8 workgroups

// columns [blockIdx.y * kper, + kper) of row blockIdx.x
__global__ __launch_bounds__(SA_THREADS)
void segment_loss_kernel(RaggedSegs segs, nvrx_segtailattr_args a, int64_t kper) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const int64_t ks = (int64_t)blockIdx.y * kper;
    const int64_t ke = min(K, ks + kper);
    double* const out = a.loss_all + r * K;
    for (int64_t kb = ks + wave * 64; kb < ke; kb += SA_TRIP) {  // wave-uniform
        const int64_t k = kb + lane;
        int T = -1, n = 0;
        u64 bl = 0, bt = 0;
        const uint32_t* p = nullptr;
        if (k < ke) {
            const int64_t u = a.thr_index ? (int64_t)a.thr_index[k] : k;
            if (u >= 0) T = a.thr[u];
            if (T >= 0) {
                bl = a.base[2 * u];
                bt = a.base[2 * u + 1];
                segs.get(r * K + k, p, n);
            }
        }
        // a skipped or empty (r, k) keeps NaN; a wave-class one is set below
        double loss = __builtin_nan("");
        if (n > 0 && n <= ST_LANE_MAX) {
            TailAcc<false> acc;
            for (int i = 0; i < n; i += ST_UNROLL) {
                unsigned x[ST_UNROLL];
                lane_load(p, n, i, x);
#pragma unroll
                for (int u = 0; u < ST_UNROLL; ++u)
                    if (i + u < n) acc.add(x[u], T);
            }
            double share;
            loss = excess(acc.tail, acc.total, bl, bt, share);
        }
        uint64_t longs = __ballot(n > ST_LANE_MAX);
        while (longs) {  // wave-uniform
            const int l = __builtin_ctzll(longs);
            longs &= longs - 1;
            const uint32_t* q = rl_ptr(p, l);
            const int m = (int)rl((unsigned)n, l);
            const int t = (int)rl((unsigned)T, l);
            TailAcc<false> acc;
            for (int base = 0; base < m; base += 64 * ST_UNROLL) {
                unsigned x[ST_UNROLL];
                wave_load(q, m, base, x);
#pragma unroll
                for (int u = 0; u < ST_UNROLL; ++u)
                    if (base + u * 64 + lane < m) acc.add(x[u], t);
            }
            const u64 total = wave_sum_u64(acc.total);
            const u64 tail = wave_sum_u64(acc.tail);
            double share;
            const double v = excess(tail, total, rl_u64(bl, l), rl_u64(bt, l), share);  // uniform
            if (lane == l) loss = v;
        }
        if (k < ke) out[k] = loss == loss ? loss : __builtin_nan("");
    }
}

template <int TOP>
__global__ __launch_bounds__(256)
void segment_select_kernel(RaggedSegs segs, nvrx_segtailattr_args a) {
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const double* __restrict__ row = a.loss_all + r * K;
    const int top = a.top < TOP ? a.top : TOP;
    NVRX_TOPK_WINNERS(TOP, row, K, top, win);

    // wave v recomputes winners v, v + 4, ... from the samples and stores their outputs
    for (int j = wave; j < top; j += 4) {
        const int col = __builtin_amdgcn_readfirstlane(win[j]);
        u64 tail = 0, total = 0;
        unsigned calls = 0;
        int T = -1;
        double share = __builtin_nan(""), loss = share;
        if (col >= 0) {  // wave-uniform, as everything up to the stores
            const int64_t u = a.thr_index ? (int64_t)a.thr_index[col] : (int64_t)col;
            if (u >= 0) T = a.thr[u];
            const uint32_t* q = nullptr;
            int m = 0;
            if (T >= 0) segs.get(r * K + col, q, m);
            if (m > 0) {
                TailAcc<true> acc;
                for (int base = 0; base < m; base += 64 * ST_UNROLL) {
                    unsigned x[ST_UNROLL];
                    wave_load(q, m, base, x);
#pragma unroll
                    for (int v = 0; v < ST_UNROLL; ++v)
                        if (base + v * 64 + lane < m) acc.add(x[v], T);
                }
                total = wave_sum_u64(acc.total);
                tail = wave_sum_u64(acc.tail);
                calls = wave_sum_u32(acc.calls);
                loss = excess(tail, total, a.base[2 * u], a.base[2 * u + 1], share);
            }
        }
        if (lane != 0) continue;
        store_winner(a, r * a.top + j, loss == loss, col, loss, tail, total, calls, T, share);
    }
}

}  // namespace

// Argument checks happen in abi.cpp before this runs.
hipError_t segment_tail_attribution_ragged(const nvrx_segtailattr_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    if (a.top < 1 || a.top > NVRX_MAX_ATTRIBUTION) return hipErrorInvalidValue;
    int64_t kper;
    const int64_t splits = row_splits(a.R, a.K, SA_TRIP, SA_TARGET_WGS, &kper);
    const dim3 grid((unsigned)a.R, (unsigned)splits);
    const dim3 rows((unsigned)a.R), b(256);
    const RaggedSegs segs{a.ns, a.seg_off, a.seg_len, a.cap};
    hipLaunchKernelGGL(segment_loss_kernel, grid, dim3(SA_THREADS), 0, st, segs, a, kper);
    dispatch_top(a.top, [&](auto t) {
        hipLaunchKernelGGL(segment_select_kernel<decltype(t)::value>, rows, b, 0, st, segs, a);
    });
    return hipGetLastError();
}

}  // namespace nvrx
