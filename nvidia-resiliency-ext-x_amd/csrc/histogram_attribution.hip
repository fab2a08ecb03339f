// histogram_attribution.hip -- tail score attribution: the kernels behind a rank's tail score, gfx950.
//
// No reference counterpart.  histogram_scores.hip (a rank against the fleet) and
// histogram_history.hip (a rank against its own history) flag a row that is slow on every n-th
// call; tail_calls counts its calls above the threshold bucket, and a count is not a cost.  Here,
// per (row r, kernel k), in exact integers over the same T as the score of that leg:
//     tail   = sum_{b>T} C[r][k][b] w(b)      total  = sum_b C[r][k][b] w(b)
//     btail  = the base's sum over b > T      btotal = the base's sum over all b
//     loss   = tail - total * (btail / btotal)                                   (f64, ns)
// with the base the fleet row (relative) or the row's own history slot (individual), and per row
// the `top` largest losses (include/nvrx_straggler.h has the full definition).  Three kernels:
//
//   tail_base_kernel     one wave per fleet kernel, 4 bins per lane on 60 lanes: {btail, btotal} of
//                        the relative leg, once per kernel and not once per (row, kernel).
//   tail_loss_kernel     grid (rows, splits of K), 256 threads, the split rule of history_kernel.
//                        A wave takes one (row, kernel) per trip, HA_UNROLL in flight: 60 lanes load
//                        one 16-byte vector of C (and one of H, individual), the lane weights are
//                        constants of the launch.  Relative: T and the base sums are wave-uniform
//                        scalar loads.  Individual: the u64 DPP prefix, ballot and bin walk of
//                        history_kernel.  One f64 store per (row, kernel) into loss_all, NaN where
//                        the element is not taken.  Every (r, k) has one owner: no atomics.
//   tail_select_kernel   one 256-thread workgroup per row over loss_all[r][:], 8 B per element:
//                        per-thread sorted candidates in registers and `top` rounds of DPP + LDS
//                        argmax (topk_select.h, shared with attribution.hip).  Then wave v
//                        recomputes winners v, v + 4, ... from the inputs with the element function
//                        of the loss kernel and stores every per-winner output: what is stored
//                        comes from the inputs, the key only orders.
// Partial top lists per split would need scratch the entry may not allocate, plus a merge; the
// caller's dense [R][K] f64 costs 8 B per element against the 960 / 1,920 B read, and is itself a
// useful output.  Every loop is bounded by K.  No kernel uses scratch memory (make asm).

#include "histogram_wave.h"
#include "topk_select.h"

namespace nvrx {
namespace {

constexpr int HA_THREADS = 256;
constexpr int HA_WAVES = HA_THREADS / 64;
constexpr int HA_UNROLL = 4;                     // (row, kernel) elements in flight per wave
constexpr int HA_TRIP = HA_WAVES * HA_UNROLL;    // kernels per workgroup trip: a split's granule
constexpr int HA_TARGET_WGS = 2048;              // 256 CUs x 8 workgroups

__global__ __launch_bounds__(256)
void tail_base_kernel(const u64* __restrict__ fleet, int64_t K, const int32_t* __restrict__ thr,
                      u64* base) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t k = (int64_t)blockIdx.x * 4 + wave;
    if (k >= K) return;  // wave-uniform; the kernel has no workgroup barrier
    const int T = __builtin_amdgcn_readfirstlane(thr[k]);
    u64 total = 0, tail = 0;
    if (T >= 0) {
        u64 h[4] = {0ull, 0ull, 0ull, 0ull};
        if (lane < HV) {
            const u64x2* p = (const u64x2*)(fleet + k * HB + 4 * lane);
            const u64x2 a = p[0], b = p[1];
            h[0] = a.x;
            h[1] = a.y;
            h[2] = b.x;
            h[3] = b.y;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = 4 * lane + i;
            const u64 t = h[i] * (u64)weight_of(b);
            total += t;
            tail += b > T ? t : 0ull;
        }
        total = wave_sum_u64(total);
        tail = wave_sum_u64(tail);
    }
    if (lane == 0) *(u64x2*)(base + 2 * k) = (u64x2){tail, total};
}

// What a wave holds of one (row, kernel) before the arithmetic: q / g the lane's vector of C / H
// (zeros in lanes 60..63 and where the element has no base), ok whether it has a base at all, and
// for the relative leg T and the fleet row's sums.  Everything but q and g is wave-uniform.
struct ElementIn {
    u32x4 q, g;
    bool ok;
    int T;
    u64 btail, btotal;
};
template <bool IND>
__device__ __forceinline__ ElementIn element_inputs(const nvrx_tailattr_args& a, const u32x4* crow,
                                                    const u32x4* hrow, int64_t k, int lane) {
    ElementIn e;
    e.q = (u32x4){0u, 0u, 0u, 0u};
    e.g = (u32x4){0u, 0u, 0u, 0u};
    e.T = -1;
    e.btail = e.btotal = 0ull;
    if (IND) {
        const int64_t s = slot_of(a, k);
        e.ok = s >= 0;
        if (e.ok && lane < HV) {
            e.q = __builtin_nontemporal_load(crow + k * HV);
            e.g = hrow[s * HV];
        }
    } else {
        const int64_t u = a.thr_index ? (int64_t)a.thr_index[k] : k;
        if (u >= 0) e.T = a.thr[u];
        e.ok = e.T >= 0;
        if (e.ok) {
            e.btail = a.base[2 * u];
            e.btotal = a.base[2 * u + 1];
            if (lane < HV) e.q = __builtin_nontemporal_load(crow + k * HV);
        }
    }
    return e;
}

struct TailTerms {
    u64 tail, total;
    unsigned calls;
    int T;
    double share, loss;
};

// One element's terms, computed by the whole wave (every lane returns the same); false when the
// element is not taken (no base, no samples, an empty history, a NaN loss).  Both kernels call it,
// so a winner's stored loss is the loss that ranked it.  FULL adds the call count.
template <bool IND, bool FULL>
__device__ __forceinline__ bool tail_element(const ElementIn& e, int pm, const LaneBins& w,
                                             TailTerms& o) {
    const u32x4 q = e.q, g = e.g;
    o.tail = o.total = 0ull;
    o.calls = 0u;
    o.T = -1;
    o.share = o.loss = __builtin_nan("");
    const bool any = __ballot((q.x | q.y | q.z | q.w) != 0u) != 0ull;
    if (!(e.ok && any)) return false;  // wave-uniform
    int t = e.T;
    u64 bl = e.btail, bt = e.btotal;
    if (IND) {
        // lanes 60..63 hold zeros
        const u64 local = ((u64)g.x + g.y) + ((u64)g.z + g.w);
        const u64 incl = wave_incl_scan_u64(local);
        const u64 N = rl_u64(incl, 63);
        if (N == 0) return false;
        // (pm (N - 1)) / 1000 without the product leaving 64 bits
        const u64 d = (N - 1) / 1000ull, m = (N - 1) % 1000ull;
        const u64 rank = (u64)pm * d + ((u64)pm * m) / 1000ull;
        // incl is non-decreasing and incl[59] = N > rank: the lanes at or below rank are a prefix
        const int L = (int)__popcll(__ballot(incl <= rank));
        u64 c = incl - local;
        int j = 0;
        c += g.x;
        j += c <= rank;
        c += g.y;
        j += c <= rank;
        c += g.z;
        j += c <= rank;
        t = (int)rl((unsigned)(w.b0 + j), L);
    }
    const bool t0 = w.b0 > t, t1 = w.b0 + 1 > t, t2 = w.b0 + 2 > t, t3 = w.b0 + 3 > t;
    if (IND) {
        const u64 o0 = (u64)g.x * w.w0, o1 = (u64)g.y * w.w1, o2 = (u64)g.z * w.w2,
                  o3 = (u64)g.w * w.w3;
        bt = wave_sum_u64((o0 + o1) + (o2 + o3));
        bl = wave_sum_u64(((t0 ? o0 : 0ull) + (t1 ? o1 : 0ull)) + ((t2 ? o2 : 0ull) + (t3 ? o3 : 0ull)));
    }
    const u64 p0 = (u64)q.x * w.w0, p1 = (u64)q.y * w.w1, p2 = (u64)q.z * w.w2, p3 = (u64)q.w * w.w3;
    o.total = wave_sum_u64((p0 + p1) + (p2 + p3));
    o.tail = wave_sum_u64(((t0 ? p0 : 0ull) + (t1 ? p1 : 0ull)) + ((t2 ? p2 : 0ull) + (t3 ? p3 : 0ull)));
    if (FULL)
        o.calls = wave_sum_u32(((t0 ? q.x : 0u) + (t1 ? q.y : 0u)) + ((t2 ? q.z : 0u) + (t3 ? q.w : 0u)));
    o.T = t;
    o.loss = excess(o.tail, o.total, bl, bt, o.share);
    return o.loss == o.loss;
}

// kernels [blockIdx.y * kper, + kper) of row blockIdx.x
template <bool IND>
__global__ __launch_bounds__(HA_THREADS) void tail_loss_kernel(nvrx_tailattr_args a, int64_t kper) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const int64_t kb = (int64_t)blockIdx.y * kper;
    const int64_t ke = min(K, kb + kper);
    const int64_t stride = a.hist_stride ? a.hist_stride : K;
    const LaneBins w = lane_bins(lane);
    const u32x4* crow = (const u32x4*)(a.counts + r * K * HB) + lane;
    const u32x4* hrow = IND ? (const u32x4*)(a.hist + r * stride * HB) + lane : nullptr;
    double* out = a.loss_all + r * K;
    for (int64_t k0 = kb + wave; k0 < ke; k0 += HA_TRIP) {
        ElementIn e[HA_UNROLL];
#pragma unroll
        for (int u = 0; u < HA_UNROLL; ++u) {
            const int64_t k = k0 + u * HA_WAVES;  // wave-uniform
            if (k < ke) e[u] = element_inputs<IND>(a, crow, hrow, k, lane);
        }
#pragma unroll
        for (int u = 0; u < HA_UNROLL; ++u) {
            const int64_t k = k0 + u * HA_WAVES;
            if (k >= ke) continue;
            TailTerms t;
            const bool taken = tail_element<IND, false>(e[u], a.permille, w, t);
            if (lane == 0) out[k] = taken ? t.loss : __builtin_nan("");
        }
    }
}

template <bool IND, int TOP>
__global__ __launch_bounds__(256) void tail_select_kernel(nvrx_tailattr_args a) {
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const double* __restrict__ row = a.loss_all + r * K;
    const int top = a.top < TOP ? a.top : TOP;
    NVRX_TOPK_WINNERS(TOP, row, K, top, win);

    // wave v recomputes winners v, v + 4, ... from the inputs and stores their outputs
    const int64_t stride = a.hist_stride ? a.hist_stride : K;
    const LaneBins w = lane_bins(lane);
    const u32x4* crow = (const u32x4*)(a.counts + r * K * HB) + lane;
    const u32x4* hrow = IND ? (const u32x4*)(a.hist + r * stride * HB) + lane : nullptr;
    for (int j = wave; j < top; j += 4) {
        const int col = __builtin_amdgcn_readfirstlane(win[j]);
        TailTerms t;
        bool taken = false;
        if (col >= 0) {
            const ElementIn e = element_inputs<IND>(a, crow, hrow, (int64_t)col, lane);
            taken = tail_element<IND, true>(e, a.permille, w, t);
        }
        if (lane != 0) continue;
        store_winner(a, r * a.top + j, taken, col, t.loss, t.tail, t.total, t.calls, t.T, t.share);
    }
}

template <bool IND>
void launch_select(const nvrx_tailattr_args& a, hipStream_t st) {
    const dim3 g((unsigned)a.R), b(256);
    dispatch_top(a.top, [&](auto t) {
        hipLaunchKernelGGL((tail_select_kernel<IND, decltype(t)::value>), g, b, 0, st, a);
    });
}

}  // namespace

// Argument checks happen in abi.cpp before these run.
hipError_t histogram_tail_base(const uint64_t* fleet, int64_t K, const int32_t* thr, uint64_t* base,
                               hipStream_t st) {
    if (K <= 0) return hipSuccess;
    hipLaunchKernelGGL(tail_base_kernel, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, st,
                       (const u64*)fleet, K, thr, (u64*)base);
    return hipGetLastError();
}

hipError_t histogram_tail_attribution(const nvrx_tailattr_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    if (a.top < 1 || a.top > NVRX_MAX_ATTRIBUTION) return hipErrorInvalidValue;
    if (a.kind != NVRX_ATTR_RELATIVE && a.kind != NVRX_ATTR_INDIVIDUAL) return hipErrorInvalidValue;
    int64_t kper;
    const int64_t splits = row_splits(a.R, a.K, HA_TRIP, HA_TARGET_WGS, &kper);
    const dim3 grid((unsigned)a.R, (unsigned)splits);
    if (a.kind == NVRX_ATTR_INDIVIDUAL) {
        hipLaunchKernelGGL(tail_loss_kernel<true>, grid, dim3(HA_THREADS), 0, st, a, kper);
        launch_select<true>(a, st);
    } else {
        hipLaunchKernelGGL(tail_loss_kernel<false>, grid, dim3(HA_THREADS), 0, st, a, kper);
        launch_select<false>(a, st);
    }
    return hipGetLastError();
}

}  // namespace nvrx
