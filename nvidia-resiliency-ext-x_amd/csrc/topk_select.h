// topk_select.h -- what the two top-k kernels share (attribution.hip: the kernels behind a GPU
// score; histogram_attribution.hip: the kernels behind a tail score): an order-preserving 64-bit
// key of an f64 loss, the per-thread sorted candidate list in registers (insert / pop), and the
// wave argmax over (key, column) on DPP.  For the five tail attributions (histogram_attribution,
// segment_tail_attribution, segment_history_attribution, segment_history_compact_attribution,
// histogram_history_compact_attribution) also the select's first half (NVRX_TOPK_WINNERS), the
// winner's stores and the host's choice of TOP.
#pragma once
#include <type_traits>

#include "nvrx_common.h"

namespace nvrx {
namespace {

// Larger loss <=> larger key (unsigned).  NaN losses never get a key, so key 0 (the pattern of a
// negative NaN with every bit set) is free to mean "no candidate".  -0.0 and +0.0 share +0.0's key:
// they compare equal, so their order is the column order.
__device__ __forceinline__ uint64_t loss_key(double loss) {
    const uint64_t b = loss == 0.0 ? 0ull : (uint64_t)__double_as_longlong(loss);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

constexpr int32_t NO_COL = 0x7FFFFFFF;

// (ka, ca) ranks before (kb, cb): larger key, then lower column
__device__ __forceinline__ bool before(uint64_t ka, int32_t ca, uint64_t kb, int32_t cb) {
    return ka > kb || (ka == kb && ca < cb);
}

template <int CTRL>
__device__ __forceinline__ void best_step(uint64_t& k, int32_t& c) {
    const unsigned lo = dpp<CTRL>((unsigned)k), hi = dpp<CTRL>((unsigned)(k >> 32));
    const uint64_t ok = ((uint64_t)hi << 32) | lo;
    const int32_t oc = (int32_t)dpp<CTRL>((unsigned)c);
    const bool take = before(ok, oc, k, c);
    k = take ? ok : k;
    c = take ? oc : c;
}

__device__ __forceinline__ uint64_t rl64(uint64_t x, int l) {
    const unsigned lo = rl((unsigned)x, l), hi = rl((unsigned)(x >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// The wave's best (key, column): after the four in-row steps every lane holds its row's best; the
// four rows are combined from lanes 0 / 16 / 32 / 48 (uniform).
__device__ __forceinline__ void wave_best(uint64_t& k, int32_t& c) {
    best_step<0xB1>(k, c);
    best_step<0x4E>(k, c);
    best_step<0x141>(k, c);
    best_step<0x140>(k, c);
    uint64_t bk = rl64(k, 0);
    int32_t bc = (int32_t)rl((unsigned)c, 0);
#pragma unroll
    for (int l = 16; l < 64; l += 16) {
        const uint64_t ok = rl64(k, l);
        const int32_t oc = (int32_t)rl((unsigned)c, l);
        const bool take = before(ok, oc, bk, bc);
        bk = take ? ok : bk;
        bc = take ? oc : bc;
    }
    k = bk;
    c = bc;
}

}  // namespace
}  // namespace nvrx

// A thread's candidates ck[TOP] (keys) / cc[TOP] (columns), best first, in registers: every index
// is a compile-time constant once the loops are unrolled.  The two steps are statement macros, not
// functions: passed to a function by reference the arrays are promoted to registers along another
// path and attribution_kernel's code changes (register numbering, one wait); expanded in place the
// kernel's assembly is what it was before the steps moved here.
//
// insert: a thread meets its columns in increasing order, so a new candidate goes behind the
// equal keys it already holds (strict >); a key of 0 goes nowhere.  Positions from n on are known
// to be empty (n = TOP when nothing is known).  Skip it when no lane's key beats position n - 1.
#define NVRX_TOPK_INSERT(TOP, ck, cc, key, col, n)                        \
    do {                                                                  \
        bool gt_[TOP];                                                    \
        _Pragma("unroll") for (int i = 0; i < TOP; ++i) gt_[i] = (key) > ck[i]; \
        _Pragma("unroll") for (int i = TOP - 1; i >= 0; --i) {            \
            if (i >= (n)) continue;                                       \
            const bool shift_ = i > 0 && gt_[i > 0 ? i - 1 : 0];          \
            const uint64_t pk_ = ck[i > 0 ? i - 1 : 0];                   \
            const int32_t pc_ = cc[i > 0 ? i - 1 : 0];                    \
            ck[i] = shift_ ? pk_ : (gt_[i] ? (key) : ck[i]);              \
            cc[i] = shift_ ? pc_ : (gt_[i] ? (col) : cc[i]);              \
        }                                                                 \
    } while (0)

// pop: the thread that holds the round's winner drops its head.  Skip it in the waves without it.
#define NVRX_TOPK_POP(TOP, ck, cc, pop)                                   \
    do {                                                                  \
        _Pragma("unroll") for (int i = 0; i < TOP - 1; ++i) {             \
            ck[i] = (pop) ? ck[i + 1] : ck[i];                            \
            cc[i] = (pop) ? cc[i + 1] : cc[i];                            \
        }                                                                 \
        ck[TOP - 1] = (pop) ? 0ull : ck[TOP - 1];                         \
        cc[TOP - 1] = (pop) ? NO_COL : cc[TOP - 1];                       \
    } while (0)

// The select of the tail attributions, by one 256-thread workgroup: the columns of the `top`
// (<= TOP) largest losses of row[0, K) (const double*), best first, into win[] in LDS; -1 where
// fewer are taken (a NaN loss is not).  Ties go to the lower column.  Ends with a workgroup
// barrier: every thread may read win[] afterwards.  It declares the kernel's LDS (best_k, best_c:
// the two rounds' per-wave bests; win) and reads the kernel's tid, wave and lane.
//
// A statement macro like the two steps above, and for their reason: as a __forceinline__ function
// each select kernel kept its register, LDS and occupancy figures but not its instructions (the
// order of the LDS arrays, and the exit test of the rounds' loop inverted); expanded in place the
// four select kernels' assembly is what it was with this block written out in each.
//   per thread: candidates best first, every index a compile-time constant; batches of SC = 8
//   loads, all issued before any is used; FIRST: the thread's first batch, whose element c finds
//   at most c candidates held (positions from n on are empty); a NaN is not taken; the insert is
//   skipped where no lane's key beats position n - 1 (wave-uniform).
//   then `top` rounds of workgroup argmax over the threads' heads: the winner pops its head
//   (columns are distinct, so one thread at most holds wc); the three waves without it skip the
//   shift.
#define NVRX_TOPK_WINNERS(TOP, row, K, top, win)                                                   \
    __shared__ uint64_t best_k[2][4];                                                              \
    __shared__ int32_t best_c[2][4];                                                               \
    __shared__ int32_t win[NVRX_MAX_ATTRIBUTION];                                                  \
    do {                                                                                           \
        uint64_t ck[TOP];                                                                          \
        int32_t cc[TOP];                                                                           \
        _Pragma("unroll") for (int i = 0; i < TOP; ++i) {                                          \
            ck[i] = 0;                                                                             \
            cc[i] = NO_COL;                                                                        \
        }                                                                                          \
        constexpr int SC = 8;                                                                      \
        auto batch = [&](const int64_t k0, auto first) {                                           \
            constexpr bool FIRST = decltype(first)::value;                                         \
            double v[SC];                                                                          \
            _Pragma("unroll") for (int c = 0; c < SC; ++c) {                                       \
                const int64_t k = k0 + c * 256;                                                    \
                v[c] = k < (K) ? (row)[k] : __builtin_nan("");                                     \
            }                                                                                      \
            _Pragma("unroll") for (int c = 0; c < SC; ++c) {                                       \
                const uint64_t key = v[c] == v[c] ? loss_key(v[c]) : 0ull;                         \
                const int32_t col = (int32_t)(k0 + c * 256);                                       \
                const int n = FIRST && c + 1 < TOP ? c + 1 : TOP;                                  \
                if (__builtin_amdgcn_ballot_w64(key > ck[n - 1]) == 0) continue;                   \
                NVRX_TOPK_INSERT(TOP, ck, cc, key, col, n);                                        \
            }                                                                                      \
        };                                                                                         \
        batch(tid, std::true_type{});                                                              \
        for (int64_t k0 = (int64_t)tid + 256 * SC; k0 < (K); k0 += 256 * SC)                       \
            batch(k0, std::false_type{});                                                          \
        for (int j = 0; j < (top); ++j) {                                                          \
            uint64_t k = ck[0];                                                                    \
            int32_t c = cc[0];                                                                     \
            wave_best(k, c);                                                                       \
            const int b = j & 1;                                                                   \
            if (lane == 0) {                                                                       \
                best_k[b][wave] = k;                                                               \
                best_c[b][wave] = c;                                                               \
            }                                                                                      \
            __syncthreads();                                                                       \
            uint64_t wk = best_k[b][0];                                                            \
            int32_t wc = best_c[b][0];                                                             \
            _Pragma("unroll") for (int v = 1; v < 4; ++v) {                                        \
                const uint64_t ok = best_k[b][v];                                                  \
                const int32_t oc = best_c[b][v];                                                   \
                const bool take = before(ok, oc, wk, wc);                                          \
                wk = take ? ok : wk;                                                               \
                wc = take ? oc : wc;                                                               \
            }                                                                                      \
            if (tid == 0) win[j] = wk != 0 ? wc : -1;                                              \
            const bool pop = wk != 0 && cc[0] == wc;                                               \
            if (__builtin_amdgcn_ballot_w64(pop) == 0) continue;                                   \
            NVRX_TOPK_POP(TOP, ck, cc, pop);                                                       \
        }                                                                                          \
        __syncthreads();                                                                           \
    } while (0)

namespace nvrx {
namespace {

// what a select kernel stores for winner slot o of its args: the terms when taken, else the empty
// slot
template <typename Args>
__device__ __forceinline__ void store_winner(const Args& a, int64_t o, bool taken, int col, double loss,
                                             uint64_t tail, uint64_t total, unsigned calls, int T,
                                             double share) {
    const double qnan = __builtin_nan("");
    a.idx[o] = taken ? col : -1;
    a.loss[o] = taken ? loss : qnan;
    a.tail_ns[o] = taken ? tail : 0ull;
    a.total_ns[o] = taken ? total : 0ull;
    a.tail_calls[o] = taken ? calls : 0u;
    a.thr_bucket[o] = taken ? T : -1;
    a.base_share[o] = taken ? share : qnan;
}

// Host side: f(std::integral_constant<int, TOP>) with the smallest TOP of 1 / 4 / 8 / 16 that
// holds `top`
template <typename F>
inline void dispatch_top(int top, F&& f) {
    if (top <= 1)
        f(std::integral_constant<int, 1>{});
    else if (top <= 4)
        f(std::integral_constant<int, 4>{});
    else if (top <= 8)
        f(std::integral_constant<int, 8>{});
    else
        f(std::integral_constant<int, 16>{});
}

}  // namespace
}  // namespace nvrx
