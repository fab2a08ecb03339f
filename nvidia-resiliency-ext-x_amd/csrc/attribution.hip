// attribution.hip -- score attribution on gfx950: per rank row, the `top` kernels that cost
// the row most of its GPU score.  No reference counterpart (the reference reports the score only).
//
// The score of a row is sum_k s_k*w_k / sum_k w_k with s_k = base_k / MED_k and w_k = NUM_k*AVG_k
// (scores.hip), so 1 - score = sum_k w_k*(1 - s_k) / sum_k w_k.  loss_k = w_k*(1 - s_k) is the
// weighted time the row lost on kernel k; the kernel selects the `top` largest per row, ties to
// the lower column.  Element terms are f64 with separately rounded operations (-ffp-contract=off),
// the same arrays and eligibility rules as scores_kernel; the history is read, never written.
//
// Shape: one 256-thread workgroup per row.  Threads stride over the columns with batched loads
// (as scores_kernel) and each keeps its best TOP candidates in registers, sorted; a candidate is
// an order-preserving 64-bit key of the loss plus its column (3 VGPRs).  Then `top` rounds of
// workgroup argmax over the threads' heads: a DPP butterfly per wave, the four wave results
// through LDS (double-buffered: one barrier per round), and the winning thread pops its head.
// Thread j remembers the winner of round j; after the rounds threads 0..top-1 recompute their
// element's loss and s from the inputs and store the row's outputs in parallel, so the values
// stored are the ones computed from the inputs (the key only orders them).
#include <type_traits>

#include "nvrx_common.h"
#include "nvrx_internal.h"
#include "score_element.h"
#include "topk_select.h"

namespace nvrx {

template <typename T, int TOP>
__global__ __launch_bounds__(256) void attribution_kernel(nvrx_attribution_args a) {
    __shared__ uint64_t best_k[2][4];
    __shared__ int32_t best_c[2][4];
    __shared__ double wred[4];
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const int64_t hs = a.hist_stride > 0 ? a.hist_stride : K;
    const bool rel = a.kind == NVRX_ATTR_RELATIVE;
    const int32_t* __restrict__ num = a.num + r * K;
    const T* __restrict__ med = (const T*)a.med + r * K;
    const T* __restrict__ avg = (const T*)a.avg + r * K;
    const T* __restrict__ hist = (const T*)a.hist + (rel ? 0 : r * hs);

    // this thread's candidates, best first; every index below is a compile-time constant
    uint64_t ck[TOP];
    int32_t cc[TOP];
#pragma unroll
    for (int i = 0; i < TOP; ++i) {
        ck[i] = 0;
        cc[i] = NO_COL;
    }
    double wsum = 0.0;
    bool zero_med = false;

    constexpr int SC = 8;  // as scores_kernel: every load of a batch is issued before any is used
    // FIRST: the thread's first batch, whose element c finds at most c candidates held, so its
    // insertion looks at positions 0..c only (at K <= 2048 that is every insertion of the row)
    auto batch = [&](const int64_t k0, auto first) {
        constexpr bool FIRST = decltype(first)::value;
        int32_t nm[SC];
        T mt[SC], av[SC];
        double bs[SC];
        bool ok[SC];
#pragma unroll
        for (int c = 0; c < SC; ++c) {
            const int64_t k = k0 + c * 256;
            const bool in = k < K;
            nm[c] = in ? num[k] : 0;
            ok[c] = in && (!a.col_valid || a.col_valid[k]);
            mt[c] = in ? med[k] : (T)1;
            av[c] = in ? avg[k] : (T)0;
            bs[c] = 0.0;
            if (in && rel) {
                const int64_t ri = a.ref_index ? a.ref_index[k] : k;
                const float rf = a.ref[ri];
                // -1 / NaN / flagged missing => no reference, as scores_kernel
                ok[c] = ok[c] && rf >= 0.0f && !(a.ref_missing && a.ref_missing[ri]);
                bs[c] = (double)rf;
            } else if (in) {
                bs[c] = (double)hist[a.hist_index ? a.hist_index[k] : k];
            }
        }
#pragma unroll
        for (int c = 0; c < SC; ++c) {
            double w, s, loss;
            bool zm;
            const bool take = element_terms<T>(ok[c] && nm[c] > 0, nm[c], mt[c], av[c], bs[c], w, s,
                                               loss, zm);
            zero_med |= zm;
            wsum = wsum + (take ? w : 0.0);
            // insert: a thread meets its columns in increasing order, so a new candidate goes
            // behind the equal keys it already holds (strict >); a key of 0 goes nowhere
            const uint64_t key = take ? loss_key(loss) : 0ull;
            const int32_t col = (int32_t)(k0 + c * 256);
            const int n = FIRST && c + 1 < TOP ? c + 1 : TOP;  // positions from n on are empty
            if (__builtin_amdgcn_ballot_w64(key > ck[n - 1]) == 0) continue;  // wave-uniform skip
            NVRX_TOPK_INSERT(TOP, ck, cc, key, col, n);
        }
    };
    batch(tid, std::true_type{});
    for (int64_t k0 = (int64_t)tid + 256 * SC; k0 < K; k0 += 256 * SC) batch(k0, std::false_type{});

    // the row's weight: lanes by DPP, the four waves in wave order (deterministic)
    wsum = wave_sum_f64(wsum);
    const bool anyzero = __ballot(zero_med) != 0;
    if (lane == 0) {
        wred[wave] = wsum;
        if (anyzero && a.err) atomicOr(a.err, 1);
    }

    // `top` rounds of workgroup argmax over the threads' heads
    uint64_t mine_k = 0;
    int32_t mine_c = NO_COL;
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
        if (tid == j) {
            mine_k = wk;
            mine_c = wc;
        }
        // the winner pops its head (columns are distinct, so one thread at most holds wc); the
        // three waves without it skip the shift
        const bool pop = wk != 0 && cc[0] == wc;
        if (__builtin_amdgcn_ballot_w64(pop) == 0) continue;
        NVRX_TOPK_POP(TOP, ck, cc, pop);
    }

    if (tid < top) {
        const double qnan = __builtin_nan("");
        int32_t oi = -1;
        double ol = qnan, os = qnan;
        if (mine_k != 0) {
            const int64_t k = mine_c;
            double base;
            if (rel)
                base = (double)a.ref[a.ref_index ? a.ref_index[k] : k];
            else
                base = (double)hist[a.hist_index ? a.hist_index[k] : k];
            double w, s, loss;
            bool zm;
            element_terms<T>(true, num[k], med[k], avg[k], base, w, s, loss, zm);
            oi = mine_c;
            ol = loss;
            os = s;
        }
        const int64_t o = r * a.top + tid;
        a.idx[o] = oi;
        a.loss[o] = ol;
        a.score[o] = os;
    }
    if (tid == 0 && a.wsum) a.wsum[r] = ((wred[0] + wred[1]) + wred[2]) + wred[3];
}

template <typename T>
static void launch_attribution(const nvrx_attribution_args& a, hipStream_t st) {
    const dim3 g((unsigned)a.R), b(256);
    if (a.top <= 1)
        hipLaunchKernelGGL((attribution_kernel<T, 1>), g, b, 0, st, a);
    else if (a.top <= 4)
        hipLaunchKernelGGL((attribution_kernel<T, 4>), g, b, 0, st, a);
    else if (a.top <= 8)
        hipLaunchKernelGGL((attribution_kernel<T, 8>), g, b, 0, st, a);
    else
        hipLaunchKernelGGL((attribution_kernel<T, 16>), g, b, 0, st, a);
}

hipError_t score_attribution(const nvrx_attribution_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    if (a.R > 0x7FFFFFFF || a.K > 0x7FFFFFFF) return hipErrorInvalidValue;
    if (a.top < 1 || a.top > NVRX_MAX_ATTRIBUTION) return hipErrorInvalidValue;
    if (a.value_f64)
        launch_attribution<double>(a, st);
    else
        launch_attribution<float>(a, st);
    return hipGetLastError();
}

}  // namespace nvrx
