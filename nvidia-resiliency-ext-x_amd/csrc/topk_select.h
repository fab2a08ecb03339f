// topk_select.h -- what the two top-k kernels share (attribution.hip: the kernels behind a GPU
// score; histogram_attribution.hip: the kernels behind a tail score): an order-preserving 64-bit
// key of an f64 loss, the per-thread sorted candidate list in registers (insert / pop), and the
// wave argmax over (key, column) on DPP.
#pragma once
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
