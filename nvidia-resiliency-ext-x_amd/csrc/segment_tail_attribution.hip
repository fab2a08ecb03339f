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

#include <type_traits>

#include "histogram_wave.h"
#include "segment_addr.h"
#include "topk_select.h"

namespace nvrx {
namespace {

// The sample helpers of segment_tail.hip, restated: that file keeps them in its anonymous
// namespace, and it compiles to the same assembly as long as it is not touched.
constexpr int ST_LANE_MAX = 16;  // the longest retained run a lane walks alone
constexpr int ST_UNROLL = 4;     // loads in flight per lane

// segment_histogram.hip's bucket expression: sh = e - 3 for x >= 8, 0 below
__device__ __forceinline__ unsigned bucket_of(unsigned x) {
    const unsigned sh = 28u - (unsigned)__builtin_clz(x | 8u);
    return (sh << 3) + (x >> sh);
}

__device__ __forceinline__ const uint32_t* rl_ptr(const uint32_t* p, int l) {
    const uint64_t b = (uint64_t)(uintptr_t)p;
    return (const uint32_t*)(uintptr_t)(((uint64_t)rl((unsigned)(b >> 32), l) << 32) | rl((unsigned)b, l));
}

// samples [base, base + 64 ST_UNROLL) of a segment of m, 64 consecutive ones per load; a lane past
// the end re-reads the last sample (its slot is then masked by the caller)
__device__ __forceinline__ void wave_load(const uint32_t* q, int m, int base, unsigned (&x)[ST_UNROLL]) {
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u)
        x[u] = __builtin_nontemporal_load(q + min(base + u * 64 + lane_id(), m - 1));
}
// samples [i, i + ST_UNROLL) of a lane's own segment of n
__device__ __forceinline__ void lane_load(const uint32_t* p, int n, int i, unsigned (&x)[ST_UNROLL]) {
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) x[u] = p[min(i + u, n - 1)];
}

constexpr int SA_THREADS = 256;
constexpr int SA_WAVES = SA_THREADS / 64;
constexpr int SA_TRIP = SA_THREADS;  // columns per workgroup trip: a split's granule
constexpr int SA_TARGET_WGS = 2048;  // 256 CUs x 8 workgroups

// one element's integer sums; CALLS adds the count above the threshold bucket
template <bool CALLS>
struct LossAcc {
    u64 total = 0, tail = 0;
    unsigned calls = 0;
    __device__ __forceinline__ void add(unsigned x, int t) {
        const int b = (int)bucket_of(x);
        const u64 w = weight_of(b);
        const bool hit = b > t;
        total += w;
        tail += hit ? w : 0ull;
        if (CALLS) calls += hit;
    }
};

// the three f64 operations of the definition, each rounded separately (-ffp-contract=off): both
// kernels call it, so a winner's stored loss is the loss that ranked it
__device__ __forceinline__ double excess(u64 tail, u64 total, u64 btail, u64 btotal, double& share) {
    share = (double)btail / (double)btotal;
    return (double)tail - (double)total * share;
}

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
            LossAcc<false> acc;
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
            LossAcc<false> acc;
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
    __shared__ uint64_t best_k[2][4];
    __shared__ int32_t best_c[2][4];
    __shared__ int32_t win[NVRX_MAX_ATTRIBUTION];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const double* __restrict__ row = a.loss_all + r * K;

    // this thread's candidates, best first; every index below is a compile-time constant
    uint64_t ck[TOP];
    int32_t cc[TOP];
#pragma unroll
    for (int i = 0; i < TOP; ++i) {
        ck[i] = 0;
        cc[i] = NO_COL;
    }
    constexpr int SC = 8;  // every load of a batch is issued before any is used
    // FIRST: the thread's first batch, whose element c finds at most c candidates held
    auto batch = [&](const int64_t k0, auto first) {
        constexpr bool FIRST = decltype(first)::value;
        double v[SC];
#pragma unroll
        for (int c = 0; c < SC; ++c) {
            const int64_t k = k0 + c * 256;
            v[c] = k < K ? row[k] : __builtin_nan("");
        }
#pragma unroll
        for (int c = 0; c < SC; ++c) {
            const uint64_t key = v[c] == v[c] ? loss_key(v[c]) : 0ull;  // NaN: not taken
            const int32_t col = (int32_t)(k0 + c * 256);
            const int n = FIRST && c + 1 < TOP ? c + 1 : TOP;  // positions from n on are empty
            if (__builtin_amdgcn_ballot_w64(key > ck[n - 1]) == 0) continue;  // wave-uniform skip
            NVRX_TOPK_INSERT(TOP, ck, cc, key, col, n);
        }
    };
    batch(tid, std::true_type{});
    for (int64_t k0 = (int64_t)tid + 256 * SC; k0 < K; k0 += 256 * SC) batch(k0, std::false_type{});

    // `top` rounds of workgroup argmax over the threads' heads
    const int top = a.top < TOP ? a.top : TOP;
    for (int j = 0; j < top; ++j) {
        uint64_t k = ck[0];
        int32_t c = cc[0];
        wave_best(k, c);
        const int b = j & 1;
        if (lane == 0) {
            best_k[b][wave] = k;
            best_c[b][wave] = c;
        }
        __syncthreads();
        uint64_t wk = best_k[b][0];
        int32_t wc = best_c[b][0];
#pragma unroll
        for (int v = 1; v < 4; ++v) {
            const uint64_t ok = best_k[b][v];
            const int32_t oc = best_c[b][v];
            const bool take = before(ok, oc, wk, wc);
            wk = take ? ok : wk;
            wc = take ? oc : wc;
        }
        if (tid == 0) win[j] = wk != 0 ? wc : -1;
        // the winner pops its head (columns are distinct, so one thread at most holds wc); the
        // three waves without it skip the shift
        const bool pop = wk != 0 && cc[0] == wc;
        if (__builtin_amdgcn_ballot_w64(pop) == 0) continue;
        NVRX_TOPK_POP(TOP, ck, cc, pop);
    }
    __syncthreads();

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
                LossAcc<true> acc;
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
        const bool taken = loss == loss;
        const int64_t o = r * a.top + j;
        const double qnan = __builtin_nan("");
        a.idx[o] = taken ? col : -1;
        a.loss[o] = taken ? loss : qnan;
        a.tail_ns[o] = taken ? tail : 0ull;
        a.total_ns[o] = taken ? total : 0ull;
        a.tail_calls[o] = taken ? calls : 0u;
        a.thr_bucket[o] = taken ? T : -1;
        a.base_share[o] = taken ? share : qnan;
    }
}

}  // namespace

// Argument checks happen in abi.cpp before this runs.
hipError_t segment_tail_attribution_ragged(const nvrx_segtailattr_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    if (a.top < 1 || a.top > NVRX_MAX_ATTRIBUTION) return hipErrorInvalidValue;
    // the split rule of segment_tail_scores_ragged: about SA_TARGET_WGS workgroups over rows x
    // splits, a split no shorter than one workgroup trip and a whole number of trips
    int64_t splits = (SA_TARGET_WGS + a.R - 1) / a.R;
    splits = min(splits, (a.K + SA_TRIP - 1) / SA_TRIP);
    int64_t kper = (a.K + splits - 1) / splits;
    kper = (kper + SA_TRIP - 1) / SA_TRIP * SA_TRIP;
    splits = (a.K + kper - 1) / kper;  // <= SA_TARGET_WGS: fits grid.y
    const dim3 grid((unsigned)a.R, (unsigned)splits);
    const dim3 rows((unsigned)a.R), b(256);
    const RaggedSegs segs{a.ns, a.seg_off, a.seg_len, a.cap};
    hipLaunchKernelGGL(segment_loss_kernel, grid, dim3(SA_THREADS), 0, st, segs, a, kper);
    if (a.top <= 1)
        hipLaunchKernelGGL(segment_select_kernel<1>, rows, b, 0, st, segs, a);
    else if (a.top <= 4)
        hipLaunchKernelGGL(segment_select_kernel<4>, rows, b, 0, st, segs, a);
    else if (a.top <= 8)
        hipLaunchKernelGGL(segment_select_kernel<8>, rows, b, 0, st, segs, a);
    else
        hipLaunchKernelGGL(segment_select_kernel<16>, rows, b, 0, st, segs, a);
    return hipGetLastError();
}

}  // namespace nvrx
