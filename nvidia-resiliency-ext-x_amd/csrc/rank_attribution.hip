// rank_attribution.hip -- the ranks behind a kernel's tail loss: per COLUMN of a row-major f64
// loss matrix the `top` rows with the largest loss, on gfx950.
//
// No reference counterpart.  The six tail attributions leave loss_all[R][K] on the device (every
// (rank, kernel)'s excess tail time, NaN where not taken) and name, per rank, the kernels behind its
// score.  This answers the converse: per kernel, the ranks that lose time on it, and how many.
// The definition is in include/nvrx_straggler.h ("Rank attribution").  The row-wise select of
// topk_select.h reads a row contiguously with one workgroup; a column of a row-major matrix is a
// strided walk, so the work is laid out the other way round: a LANE owns a column and the wave's
// load of one row is 512 contiguous bytes.  The matrix is read once.
//
// The kernels' bodies, the partial-list layout and the launch plan are rank_select.h's (shared with
// score_rank_attribution.hip); this file supplies the element source (the matrix) and the final
// outputs (idx, the loss re-read from the input at the winner's row, so its bits are the input's;
// taken, positive):
//   rankattr_rows_kernel<TOP, FINAL>   rows_body over MatrixSource; FINAL: the plan's one split
//          writes the outputs, else the split's partial list goes into `work`.
//   rankattr_merge_kernel<TOP>         merge_body with the final outputs.  Not launched when the
//          plan says one split.
// Every (column, split) has one owner: no atomics, no clear, no scratch (make asm).

#include "nvrx_internal.h"
#include "rank_select.h"
#include "topk_select.h"

namespace nvrx {
namespace {

// The element source: loss[r][col] as it stands; a NaN is not taken.
struct MatrixSource {
    static constexpr int BATCH = RA_BATCH;
    const double* loss;
    int64_t ld;
    using Lane = const double*;
    using Elem = double;
    __device__ __forceinline__ Lane lane(int64_t col, bool live) const { return loss + (live ? col : 0); }
    __device__ __forceinline__ Elem load(Lane base, int64_t r, bool on) const {
        return on ? base[r * ld] : __builtin_nan("");
    }
    __device__ __forceinline__ double value(Lane, Elem e, bool&) const { return e; }
    __device__ __forceinline__ void finish(bool, int) const {}
};

// One column's final outputs, round j: the winner's row and its loss as it stands in the input.
struct FinalOut {
    nvrx_rankattr_args a;
    int64_t ld;
    __device__ __forceinline__ void entry(int64_t col, int j, uint64_t key, int32_t row) const {
        const bool taken = key != 0;
        a.idx[col * a.top + j] = taken ? row : -1;
        a.loss_out[col * a.top + j] = taken ? a.loss[(int64_t)row * ld + col] : __builtin_nan("");
    }
    __device__ __forceinline__ void counts(int64_t col, int32_t taken, int32_t positive) const {
        a.taken[col] = taken;
        a.positive[col] = positive;
    }
};

// rows [blockIdx.y * rper, + rper) of the columns of tile blockIdx.x; FINAL: the plan's one split
template <int TOP, bool FINAL>
__global__ __launch_bounds__(RA_THREADS)
void rankattr_rows_kernel(nvrx_rankattr_args a, int64_t ld, int64_t rper, int64_t splits) {
    const int64_t s = blockIdx.y;
    const int64_t rb = s * rper;
    const int64_t re = min(a.R, rb + rper);
    const MatrixSource src{a.loss, ld};
    if constexpr (FINAL) {
        rows_body<TOP>(a, src, rb, re, FinalOut{a, ld});
    } else {
        rows_body<TOP>(a, src, rb, re, PartialOut{work_view(a.work, splits, a.K, a.top), s, a.K, a.top});
    }
}

template <int TOP>
__global__ __launch_bounds__(RA_THREADS)
void rankattr_merge_kernel(nvrx_rankattr_args a, int64_t ld, int64_t splits) {
    merge_body<TOP>(a, splits, FinalOut{a, ld});
}

}  // namespace

// The launch plan: the one place that decides the grid (nvrx_rank_attribution_plan).
void rank_attribution_plan(int64_t R, int64_t K, int top, int64_t* tiles, int64_t* splits,
                           int64_t* work_bytes) {
    const RankPlan p = plan_of(R, K, top);
    if (tiles) *tiles = p.tiles;
    if (splits) *splits = p.splits;
    if (work_bytes) *work_bytes = p.work_bytes;
}

// Argument checks happen in abi.cpp before this runs.
hipError_t rank_attribution(const nvrx_rankattr_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    if (a.top < 1 || a.top > NVRX_MAX_ATTRIBUTION) return hipErrorInvalidValue;
    const RankPlan p = plan_of(a.R, a.K, a.top);
    if (p.splits > 1 && !a.work) return hipErrorInvalidValue;
    const int64_t ld = a.ld ? a.ld : a.K;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.splits), tiles((unsigned)p.tiles), b(RA_THREADS);
    dispatch_top(a.top, [&](auto t) {
        constexpr int TOP = decltype(t)::value;
        if (p.splits == 1) {
            hipLaunchKernelGGL((rankattr_rows_kernel<TOP, true>), grid, b, 0, st, a, ld, p.rper, p.splits);
        } else {
            hipLaunchKernelGGL((rankattr_rows_kernel<TOP, false>), grid, b, 0, st, a, ld, p.rper, p.splits);
            hipLaunchKernelGGL(rankattr_merge_kernel<TOP>, tiles, b, 0, st, a, ld, p.splits);
        }
    });
    return hipGetLastError();
}

}  // namespace nvrx
