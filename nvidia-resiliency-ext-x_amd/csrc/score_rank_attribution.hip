// score_rank_attribution.hip -- the ranks behind a kernel's score loss: per COLUMN (kernel) of the
// statistics num / med / avg [R][K] the `top` rows (ranks) with the largest loss w*(1 - s) of the
// median scores, on gfx950.  No reference counterpart.
//
// attribution.hip names, per rank, the kernels behind its score; this is the converse.  The
// definition is in include/nvrx_straggler.h ("Score rank attribution"): the outputs are what
// nvrx_rank_attribution writes for the matrix L[r][k] of nvrx_score_attribution's element losses
// (NaN where it would not take the element), plus the winners' s.  L never exists: a lane that
// owns a column forms each element's loss in registers from three (individual kind: four) loads
// and ranks it.  The element terms are score_element.h's, the copy attribution.hip uses.
//
// The kernels' bodies, the partial-list layout and the launch plan are rank_select.h's (shared with
// rank_attribution.hip): same tiles, same splits, same `work`.  This file supplies
//   StatSource<T, TOP>   per lane, once: col_valid[k], and for the relative kind ref[ref_index[k]],
//          ref_missing, the rf >= 0 test and the base as f64; for the individual kind the history
//          slot.  Per row: num, med, avg (a wave's load of one row is three contiguous runs) and,
//          individual kind, hist[r][slot].  A column that is not eligible loads nothing.  An
//          eligible MED == 0 is a per-wave ballot and one atomicOr into err.
//   ScoreFinalOut<T>     the winner's loss and s recomputed from the inputs at (row, column), as
//          attribution.hip does: never rebuilt from the sort key, so a -0.0 loss stays -0.0.
// No atomics other than the err OR, no clear, no scratch (make asm).

#include "nvrx_internal.h"
#include "rank_select.h"
#include "score_element.h"
#include "topk_select.h"

namespace nvrx {
namespace {

// rows in flight per lane: an element is up to 28 bytes of registers (f64, individual kind) next
// to TOP candidates of 12.  f64 at TOP 16 holds 8 rows without scratch too, but at 173 VGPRs, two
// waves per SIMD; with 4 rows it is 114 and the three that its 50 KiB of LDS allow
template <typename T, int TOP>
constexpr int stat_batch() {
    return sizeof(T) == 8 && TOP == 16 ? 4 : RA_BATCH;
}

template <typename T>
struct StatView {
    const int32_t* __restrict__ num;
    const T* __restrict__ med;
    const T* __restrict__ avg;
    const T* __restrict__ hist;
    int64_t K, hs;
    bool rel;
    __device__ __forceinline__ explicit StatView(const nvrx_scorerank_args& a)
        : num(a.num), med((const T*)a.med), avg((const T*)a.avg), hist((const T*)a.hist), K(a.K),
          hs(a.hist_stride > 0 ? a.hist_stride : a.K), rel(a.kind == NVRX_ATTR_RELATIVE) {}
};

// what is constant per column: is the column eligible at all, and its base or history slot
struct StatLane {
    int64_t col, slot;
    double base;
    bool ok;
};

template <typename T>
__device__ __forceinline__ StatLane stat_lane(const nvrx_scorerank_args& a, bool rel, int64_t col,
                                              bool live) {
    StatLane ln{live ? col : 0, 0, 0.0, live && (!a.col_valid || a.col_valid[live ? col : 0])};
    if (rel) {
        const int64_t ri = live && a.ref_index ? a.ref_index[col] : ln.col;
        const float rf = live ? a.ref[ri] : -1.0f;
        // -1 / NaN / flagged missing => no reference, as scores_kernel
        ln.ok = ln.ok && rf >= 0.0f && !(a.ref_missing && a.ref_missing[ri]);
        ln.base = (double)rf;
    } else {
        ln.slot = live && a.hist_index ? a.hist_index[col] : ln.col;
    }
    return ln;
}

template <typename T, int TOP>
struct StatSource {
    static constexpr int BATCH = stat_batch<T, TOP>();
    const nvrx_scorerank_args& a;
    StatView<T> v;
    using Lane = StatLane;
    struct Elem {
        int32_t nm;
        T mt, av, hs;
    };
    __device__ __forceinline__ explicit StatSource(const nvrx_scorerank_args& args) : a(args), v(args) {}
    __device__ __forceinline__ Lane lane(int64_t col, bool live) const {
        return stat_lane<T>(a, v.rel, col, live);
    }
    // a row that is off, or a column that is not eligible, reads nothing: num 0 is an absent kernel
    __device__ __forceinline__ Elem load(const Lane& ln, int64_t r, bool on) const {
        const bool in = on && ln.ok;
        const int64_t o = r * v.K + ln.col;
        Elem e;
        e.nm = in ? v.num[o] : 0;
        e.mt = in ? v.med[o] : (T)1;
        e.av = in ? v.avg[o] : (T)0;
        e.hs = in && !v.rel ? v.hist[r * v.hs + ln.slot] : (T)0;
        return e;
    }
    __device__ __forceinline__ double value(const Lane& ln, const Elem& e, bool& zm) const {
        double w, s, loss;
        bool z;
        const bool take = element_terms<T>(e.nm > 0, e.nm, e.mt, e.av, v.rel ? ln.base : (double)e.hs,
                                           w, s, loss, z);
        zm |= z;
        return take ? loss : __builtin_nan("");
    }
    __device__ __forceinline__ void finish(bool zm, int lane) const {
        const bool anyzero = __ballot(zm) != 0;
        if (lane == 0 && anyzero && a.err) atomicOr(a.err, 1);
    }
};

// One column's final outputs, round j: the winner's row, and its loss and s from the inputs.
template <typename T>
struct ScoreFinalOut {
    const nvrx_scorerank_args& a;
    __device__ __forceinline__ void entry(int64_t col, int j, uint64_t key, int32_t row) const {
        const double qnan = __builtin_nan("");
        int32_t oi = -1;
        double ol = qnan, os = qnan;
        if (key != 0) {
            const StatView<T> v(a);
            const int64_t o = (int64_t)row * v.K + col;
            double base;
            if (v.rel)
                base = (double)a.ref[a.ref_index ? a.ref_index[col] : col];
            else
                base = (double)v.hist[(int64_t)row * v.hs + (a.hist_index ? a.hist_index[col] : col)];
            double w, s, loss;
            bool z;
            element_terms<T>(true, v.num[o], v.med[o], v.avg[o], base, w, s, loss, z);
            oi = row;
            ol = loss;
            os = s;
        }
        a.idx[col * a.top + j] = oi;
        a.loss[col * a.top + j] = ol;
        a.score[col * a.top + j] = os;
    }
    __device__ __forceinline__ void counts(int64_t col, int32_t taken, int32_t positive) const {
        a.taken[col] = taken;
        a.positive[col] = positive;
    }
};

// rows [blockIdx.y * rper, + rper) of the columns of tile blockIdx.x; FINAL: the plan's one split
template <typename T, int TOP, bool FINAL>
__global__ __launch_bounds__(RA_THREADS)
void scorerank_rows_kernel(nvrx_scorerank_args a, int64_t rper, int64_t splits) {
    const int64_t s = blockIdx.y;
    const int64_t rb = s * rper;
    const int64_t re = min(a.R, rb + rper);
    const StatSource<T, TOP> src(a);
    if constexpr (FINAL) {
        rows_body<TOP>(a, src, rb, re, ScoreFinalOut<T>{a});
    } else {
        rows_body<TOP>(a, src, rb, re, PartialOut{work_view(a.work, splits, a.K, a.top), s, a.K, a.top});
    }
}

template <typename T, int TOP>
__global__ __launch_bounds__(RA_THREADS)
void scorerank_merge_kernel(nvrx_scorerank_args a, int64_t splits) {
    merge_body<TOP>(a, splits, ScoreFinalOut<T>{a});
}

template <typename T>
void launch_score_rank(const nvrx_scorerank_args& a, const RankPlan& p, hipStream_t st) {
    const dim3 grid((unsigned)p.tiles, (unsigned)p.splits), tiles((unsigned)p.tiles), b(RA_THREADS);
    dispatch_top(a.top, [&](auto t) {
        constexpr int TOP = decltype(t)::value;
        if (p.splits == 1) {
            hipLaunchKernelGGL((scorerank_rows_kernel<T, TOP, true>), grid, b, 0, st, a, p.rper, p.splits);
        } else {
            hipLaunchKernelGGL((scorerank_rows_kernel<T, TOP, false>), grid, b, 0, st, a, p.rper, p.splits);
            hipLaunchKernelGGL((scorerank_merge_kernel<T, TOP>), tiles, b, 0, st, a, p.splits);
        }
    });
}

}  // namespace

// Argument checks happen in abi.cpp before this runs.  The plan is rank_attribution's.
hipError_t score_rank_attribution(const nvrx_scorerank_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    if (a.R > 0x7FFFFFFF || a.K > 0x7FFFFFFF) return hipErrorInvalidValue;
    if (a.top < 1 || a.top > NVRX_MAX_ATTRIBUTION) return hipErrorInvalidValue;
    const RankPlan p = plan_of(a.R, a.K, a.top);
    if (p.splits > 1 && !a.work) return hipErrorInvalidValue;
    if (a.value_f64)
        launch_score_rank<double>(a, p, st);
    else
        launch_score_rank<float>(a, p, st);
    return hipGetLastError();
}

}  // namespace nvrx
