// segment_history_attribution.hip -- individual tail score attribution straight from ragged
// segments, on gfx950.
//
// No reference counterpart.  segment_history.hip scores a rank against its own histogram history
// from the bucketed samples, without the counts[R][K][240] matrix; histogram_attribution.hip names
// the kernels behind that score (NVRX_ATTR_INDIVIDUAL), but from the matrix.  The loss needs it no
// more than the score does: per (rank r, kernel k) with history slot s and the retained samples x
// of segment r K + k,
//     T      = the bucket of the history's sample of rank (pm (N - 1)) / 1000          (H alone)
//     btail  = sum_{b > T} H[r][s][b] w(b)                 btotal = sum_b H[r][s][b] w(b)
//     tail   = sum_{x : bucket(x) > T} w(bucket(x))        total  = sum_x w(bucket(x))
//     loss   = tail - total * (btail / btotal)                                     (f64, ns)
// are integer sums over the samples and the history's bins plus three f64 operations: by definition
// the outputs are what nvrx_histogram_tail_attribution(NVRX_ATTR_INDIVIDUAL) writes on the counts
// nvrx_segment_histogram_ragged would put into a zeroed matrix (include/nvrx_straggler.h).
// Segments are addressed as there (segment_addr.h); hist is read only.  Two kernels:
//
//   seghist_loss_kernel     grid (rows, splits of K), 256 threads, the split rule and the
//          16-element workgroup trip of seghist_kernel.  A wave takes one (row, kernel) at a time,
//          SHA_UNROLL in flight -- here the SHA_UNROLL consecutive kernels from k0 + 4 wave, so
//          that their losses are neighbours in loss_all.  Slot, offset and length are
//          wave-uniform; an ineligible or empty element costs them and a NaN, its history is not
//          read.  For the others 60 lanes load one 16-byte vector of H (all SHA_UNROLL loads
//          issued before any is used); the u64 DPP prefix, a ballot and the walk over one lane's
//          four bins give T, the lane's constant weights its share of btail / btotal; the retained
//          run is read 64 consecutive samples per load, SHA_LOADS loads in flight, a lane past
//          the end masked, into per-lane u64 tail / total.  The per-lane partial sums of the
//          elements in flight are kept until all their samples are read; then their 4 SHA_UNROLL
//          u64 wave reductions stand next to each other as independent DPP chains, the three f64
//          operations finish each loss, lane u keeps the loss of element u and lanes 0..3 store
//          the trip's losses with one 32-byte store.  NaN where the element is not taken:
//          loss_all is written in full, no clear.
//   seghist_select_kernel   one 256-thread workgroup per row over loss_all[r][:]: the scheme of
//          segment_select_kernel (topk_select.h: sorted candidates in registers, `top` rounds of
//          DPP + LDS argmax).  Then wave v recomputes winners v, v + 4, ... from H and the samples
//          with the element function and the `excess` of the loss kernel, the calls from a ballot
//          and a population count, and lane 0 stores every per-winner output.  What is stored
//          comes from the inputs, the key only orders; integer sums do not depend on their order,
//          so the recomputed loss is the loss that ranked the winner.
// Every (r, k) has one owner: no atomics, no scratch, no clear.  bucket_of, lane_bins, slot_of and
// `excess` are histogram_wave.h's; the select's first half (NVRX_TOPK_WINNERS), the winner's
// stores and the choice of TOP are topk_select.h's.  Every loop is bounded by K or a retained
// length.  No kernel uses scratch memory (make asm).

#include "histogram_wave.h"
#include "segment_addr.h"
#include "topk_select.h"

namespace nvrx {
namespace {

constexpr int SHA_THREADS = 256;
constexpr int SHA_WAVES = SHA_THREADS / 64;
constexpr int SHA_UNROLL = 4;                      // elements in flight per wave
constexpr int SHA_TRIP = SHA_WAVES * SHA_UNROLL;   // elements per workgroup trip: a split's granule
constexpr int SHA_TARGET_WGS = 2048;               // 256 CUs x 8 workgroups
constexpr int SHA_LOADS = 4;                       // sample loads in flight per lane

// One element before its wave reductions: the lane's part of the four sums; T, the calls and
// whether the history holds a sample at all (N > 0) are wave-uniform.
struct Partial {
    u64 tail, total, btail, btotal;
    unsigned calls;
    int T;
    bool elig;
};

// The element function of both kernels: g the lane's vector of H[r][s] (zeros in lanes 60..63), q
// the retained run of m > 0 samples.  CALLS adds the count above T.
template <bool CALLS>
__device__ __forceinline__ Partial element_partials(const u32x4 g, const uint32_t* q, int m, int pm,
                                                    const LaneBins& w, int lane) {
    Partial p = {0ull, 0ull, 0ull, 0ull, 0u, -1, false};
    const u64 local = ((u64)g.x + g.y) + ((u64)g.z + g.w);
    const u64 incl = wave_incl_scan_u64(local);
    const u64 N = rl_u64(incl, 63);
    if (N == 0) return p;  // wave-uniform
    p.elig = true;
    // (pm (N - 1)) / 1000 without the product leaving 64 bits
    const u64 d = (N - 1) / 1000ull, mm = (N - 1) % 1000ull;
    const u64 rank = (u64)pm * d + ((u64)pm * mm) / 1000ull;
    // incl is non-decreasing and incl[59] = N > rank: the lanes at or below rank are a prefix
    const int L = (int)__popcll(__ballot(incl <= rank));
    u64 e = incl - local;
    int j = 0;
    e += g.x;
    j += e <= rank;
    e += g.y;
    j += e <= rank;
    e += g.z;
    j += e <= rank;
    const int t = (int)rl((unsigned)(w.b0 + j), L);
    p.T = t;
    const bool t0 = w.b0 > t, t1 = w.b0 + 1 > t, t2 = w.b0 + 2 > t, t3 = w.b0 + 3 > t;
    const u64 o0 = (u64)g.x * w.w0, o1 = (u64)g.y * w.w1, o2 = (u64)g.z * w.w2, o3 = (u64)g.w * w.w3;
    p.btotal = (o0 + o1) + (o2 + o3);
    p.btail = ((t0 ? o0 : 0ull) + (t1 ? o1 : 0ull)) + ((t2 ? o2 : 0ull) + (t3 ? o3 : 0ull));
    for (int base = 0; base < m; base += 64 * SHA_LOADS) {
        unsigned x[SHA_LOADS];
#pragma unroll
        for (int v = 0; v < SHA_LOADS; ++v) {
            const int i = base + v * 64 + lane;
            x[v] = i < m ? __builtin_nontemporal_load(q + i) : 0u;
        }
#pragma unroll
        for (int v = 0; v < SHA_LOADS; ++v) {
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
__global__ __launch_bounds__(SHA_THREADS)
void seghist_loss_kernel(RaggedSegs segs, nvrx_seghistattr_args a, int64_t kper) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const int64_t kb = (int64_t)blockIdx.y * kper;
    const int64_t ke = min(K, kb + kper);
    const int64_t stride = a.hist_stride ? a.hist_stride : K;
    const LaneBins w = lane_bins(lane);
    const u32x4* hrow = (const u32x4*)(a.hist + r * stride * HB) + lane;
    double* const out = a.loss_all + r * K;
    const int pm = a.permille;
    const double qnan = __builtin_nan("");
    for (int64_t k0 = kb + wave * SHA_UNROLL; k0 < ke; k0 += SHA_TRIP) {  // wave-uniform
        u32x4 h[SHA_UNROLL];
        const uint32_t* run[SHA_UNROLL];
        int len[SHA_UNROLL];
#pragma unroll
        for (int u = 0; u < SHA_UNROLL; ++u) {
            const int64_t k = k0 + u;  // wave-uniform, and so is all that follows from it
            h[u] = (u32x4){0u, 0u, 0u, 0u};
            run[u] = nullptr;
            len[u] = 0;
            if (k < ke) {
                const int64_t s = slot_of(a, k);
                if (s >= 0) segs.get(r * K + k, run[u], len[u]);
                if (len[u] <= 0) len[u] = 0;  // an empty element: no loss, no read of H
                else if (lane < HV) h[u] = hrow[s * HV];
            }
        }
        Partial p[SHA_UNROLL];
        bool any = false;
#pragma unroll
        for (int u = 0; u < SHA_UNROLL; ++u) {
            p[u] = Partial{0ull, 0ull, 0ull, 0ull, 0u, -1, false};
            if (len[u] > 0) p[u] = element_partials<false>(h[u], run[u], len[u], pm, w, lane);
            any |= p[u].elig;
        }
        double loss = qnan;
        if (any) {  // wave-uniform; the 4 SHA_UNROLL reductions are independent of each other
#pragma unroll
            for (int u = 0; u < SHA_UNROLL; ++u) {
                const u64 tail = wave_sum_u64(p[u].tail), total = wave_sum_u64(p[u].total);
                const u64 bl = wave_sum_u64(p[u].btail), bt = wave_sum_u64(p[u].btotal);
                double share;
                const double v = excess(tail, total, bl, bt, share);
                if (lane == u) loss = p[u].elig && v == v ? v : qnan;
            }
        }
        if (lane < SHA_UNROLL && k0 + lane < ke) out[k0 + lane] = loss;
    }
}

template <int TOP>
__global__ __launch_bounds__(256)
void seghist_select_kernel(RaggedSegs segs, nvrx_seghistattr_args a) {
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const double* __restrict__ row = a.loss_all + r * K;
    const int top = a.top < TOP ? a.top : TOP;
    NVRX_TOPK_WINNERS(TOP, row, K, top, win);

    // wave v recomputes winners v, v + 4, ... from H and the samples and stores their outputs
    const int64_t stride = a.hist_stride ? a.hist_stride : K;
    const LaneBins w = lane_bins(lane);
    const u32x4* hrow = (const u32x4*)(a.hist + r * stride * HB) + lane;
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
                u32x4 g = (u32x4){0u, 0u, 0u, 0u};
                if (lane < HV) g = hrow[s * HV];
                const Partial p = element_partials<true>(g, q, m, a.permille, w, lane);
                if (p.elig) {
                    tail = wave_sum_u64(p.tail);
                    total = wave_sum_u64(p.total);
                    const u64 bl = wave_sum_u64(p.btail), bt = wave_sum_u64(p.btotal);
                    calls = p.calls;
                    T = p.T;
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
hipError_t segment_history_attribution_ragged(const nvrx_seghistattr_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    if (a.top < 1 || a.top > NVRX_MAX_ATTRIBUTION) return hipErrorInvalidValue;
    int64_t kper;
    const int64_t splits = row_splits(a.R, a.K, SHA_TRIP, SHA_TARGET_WGS, &kper);
    const dim3 grid((unsigned)a.R, (unsigned)splits);
    const dim3 rows((unsigned)a.R), b(256);
    const RaggedSegs segs{a.ns, a.seg_off, a.seg_len, a.cap};
    hipLaunchKernelGGL(seghist_loss_kernel, grid, dim3(SHA_THREADS), 0, st, segs, a, kper);
    dispatch_top(a.top, [&](auto t) {
        hipLaunchKernelGGL(seghist_select_kernel<decltype(t)::value>, rows, b, 0, st, segs, a);
    });
    return hipGetLastError();
}

}  // namespace nvrx
