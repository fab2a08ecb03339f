// rank_select.h -- the column-wise top-k that the two rank attributions share (rank_attribution.hip:
// the ranks behind a kernel's tail loss, from a loss matrix; score_rank_attribution.hip: the ranks
// behind a kernel's score loss, from the statistics): the launch plan, the layout of the partial
// lists in `work`, and the bodies of the two kernels.  What differs between the two is where an
// element comes from (a SOURCE policy) and what the final outputs hold (an OUT functor).
//
//   rows_body<TOP>     grid (column tiles of 64, row splits), 256 threads.  Lane l of every wave
//          owns column 64 tile + l; wave w takes the split's rows w, w + 4, ... in batches of
//          Src::BATCH loads, all issued before any is used.  row_valid[r] is wave-uniform.  A lane
//          keeps its best TOP (key, row) in registers, best first (loss_key / NVRX_TOPK_INSERT of
//          topk_select.h): it meets its rows in increasing order, so the strict > of the insert
//          keeps ties in row order; the insert is skipped where no lane's key beats its last
//          candidate (wave-uniform).  taken / positive are per-lane integer counts.  Then
//          `merge_waves`.
//   merge_waves<TOP>   the four waves' lists and counts go to LDS ([wave][i][lane]: a wave's
//          access is 64 neighbouring words, no bank conflicts; 50 KiB at TOP 16), and wave 0
//          merges them per column: four heads in registers, `top` rounds of before(key, row) --
//          larger key, then lower row -- each reloading the one head that advanced.
//   What a round emits depends on the plan: with one split the caller's FINAL outputs; with
//   several the split's partial list into `work` (PartialOut):
//          keys u64 [splits][top][K] | rows i32 [splits][top][K] | counts i32 [splits][2][K]
//   so that neighbouring lanes write, and later read, neighbouring words.
//   merge_body<TOP>    grid (column tiles), 256 threads: the same shape one level up.  Wave w takes
//          splits w, w + 4, ...: a split's `top` entries are loaded together and inserted in list
//          order.  Splits come in increasing row order and a list is ordered by before(key, row),
//          so the strict > again keeps ties in row order.  Then `merge_waves` with the final
//          outputs.  Not launched when the plan says one split.
//
// A SOURCE gives, for the lane's column:
//          BATCH                       rows in flight per lane (constexpr)
//          Lane  lane(col, live)       what is constant per column, loaded once
//          Elem  load(lane, r, on)     row r's element; `on` false: nothing is read
//          double value(lane, e, zm)   its loss, NaN where not taken; zm |= an error to report
//          void  finish(zm, lane)      reports the wave's zm (one atomicOr at most)
// An OUT gives entry(col, j, key, row) and counts(col, taken, positive).
// The split rule lives in plan_of alone.  Every (column, split) has one owner: no atomics, no
// clear, no scratch.  Every loop is bounded by R, by the splits or by top.
#pragma once
#include "nvrx_internal.h"
#include "topk_select.h"

namespace nvrx {
namespace {

constexpr int RA_THREADS = 256;
constexpr int RA_WAVES = RA_THREADS / 64;
constexpr int RA_TILE = 64;           // columns per workgroup: one per lane
constexpr int RA_BATCH = 8;           // loads in flight per lane
constexpr int RA_MIN_ROWS = 64;       // a split is no shorter (16 rows per wave)
constexpr int RA_TARGET_WGS = 2048;   // 256 CUs x 8 workgroups

struct RankPlan {
    int64_t tiles, splits, rper, work_bytes;
};

// where a split's partial list lives in `work` (8-byte aligned)
struct WorkView {
    uint64_t* keys;  // [splits][top][K]
    int32_t* rows;   // [splits][top][K]
    int32_t* cnt;    // [splits][2][K]: taken, positive
};
__host__ __device__ __forceinline__ WorkView work_view(void* work, int64_t splits, int64_t K, int top) {
    WorkView v;
    v.keys = (uint64_t*)work;
    v.rows = (int32_t*)(v.keys + splits * top * K);
    v.cnt = v.rows + splits * top * K;
    return v;
}

// One column's partial list of split s.
struct PartialOut {
    WorkView w;
    int64_t s, K;
    int top;
    __device__ __forceinline__ void entry(int64_t col, int j, uint64_t key, int32_t row) const {
        w.keys[(s * top + j) * K + col] = key;
        w.rows[(s * top + j) * K + col] = row;
    }
    __device__ __forceinline__ void counts(int64_t col, int32_t taken, int32_t positive) const {
        w.cnt[(s * 2 + 0) * K + col] = taken;
        w.cnt[(s * 2 + 1) * K + col] = positive;
    }
};

// The four waves' sorted lists ck / cc (best first) and counts, merged per column by wave 0 and
// handed to `out` for the columns below K.  Ends the kernel's work: no barrier after it.
template <int TOP, typename Out>
__device__ __forceinline__ void merge_waves(const uint64_t (&ck)[TOP], const int32_t (&cc)[TOP],
                                            int32_t taken, int32_t positive, int wave, int lane,
                                            int64_t col, int64_t K, int top, const Out& out) {
    __shared__ uint64_t sk[RA_WAVES][TOP][RA_TILE];
    __shared__ int32_t sr[RA_WAVES][TOP][RA_TILE];
    __shared__ int32_t sc[RA_WAVES][2][RA_TILE];
#pragma unroll
    for (int i = 0; i < TOP; ++i) {
        sk[wave][i][lane] = ck[i];
        sr[wave][i][lane] = cc[i];
    }
    sc[wave][0][lane] = taken;
    sc[wave][1][lane] = positive;
    __syncthreads();
    if (wave != 0 || col >= K) return;
    out.counts(col, (sc[0][0][lane] + sc[1][0][lane]) + (sc[2][0][lane] + sc[3][0][lane]),
               (sc[0][1][lane] + sc[1][1][lane]) + (sc[2][1][lane] + sc[3][1][lane]));
    uint64_t hk[RA_WAVES];
    int32_t hr[RA_WAVES];
    int p[RA_WAVES];
#pragma unroll
    for (int w = 0; w < RA_WAVES; ++w) {
        hk[w] = sk[w][0][lane];
        hr[w] = sr[w][0][lane];
        p[w] = 0;
    }
    for (int j = 0; j < top; ++j) {
        uint64_t bk = hk[0];
        int32_t br = hr[0];
        int bw = 0;
#pragma unroll
        for (int w = 1; w < RA_WAVES; ++w) {
            const bool take = before(hk[w], hr[w], bk, br);
            bk = take ? hk[w] : bk;
            br = take ? hr[w] : br;
            bw = take ? w : bw;
        }
        out.entry(col, j, bk, br);
        // the winner's list advances; an exhausted or empty list shows the empty head
#pragma unroll
        for (int w = 0; w < RA_WAVES; ++w) {
            if (bw != w) continue;
            p[w] += 1;
            const bool more = p[w] < TOP;
            const int q = more ? p[w] : TOP - 1;
            const uint64_t nk = sk[w][q][lane];
            const int32_t nr = sr[w][q][lane];
            hk[w] = more ? nk : 0ull;
            hr[w] = more ? nr : NO_COL;
        }
    }
}

// rows [rb, re) of the columns of tile blockIdx.x, their elements from `src`
template <int TOP, typename Args, typename Src, typename Out>
__device__ __forceinline__ void rows_body(const Args& a, const Src& src, int64_t rb, int64_t re,
                                          const Out& out) {
    constexpr int BATCH = Src::BATCH;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int64_t K = a.K;
    const int64_t col = (int64_t)blockIdx.x * RA_TILE + lane;
    const bool live = col < K;
    const typename Src::Lane ln = src.lane(col, live);
    uint64_t ck[TOP];
    int32_t cc[TOP];
#pragma unroll
    for (int i = 0; i < TOP; ++i) {
        ck[i] = 0;
        cc[i] = NO_COL;
    }
    int32_t taken = 0, positive = 0;
    bool zm = false;
    for (int64_t r0 = rb + wave; r0 < re; r0 += RA_WAVES * BATCH) {  // wave-uniform
        typename Src::Elem e[BATCH];
#pragma unroll
        for (int c = 0; c < BATCH; ++c) {
            const int64_t r = r0 + c * RA_WAVES;
            const bool on = r < re && (!a.row_valid || a.row_valid[r < re ? r : rb] != 0);  // wave-uniform
            e[c] = src.load(ln, r, on && live);
        }
#pragma unroll
        for (int c = 0; c < BATCH; ++c) {
            const double v = src.value(ln, e[c], zm);
            const bool t = v == v;
            const uint64_t key = t ? loss_key(v) : 0ull;
            const int32_t row = (int32_t)(r0 + c * RA_WAVES);
            taken += t ? 1 : 0;
            positive += v > 0.0 ? 1 : 0;
            if (__builtin_amdgcn_ballot_w64(key > ck[TOP - 1]) == 0) continue;
            NVRX_TOPK_INSERT(TOP, ck, cc, key, row, TOP);
        }
    }
    src.finish(zm, lane);
    merge_waves<TOP>(ck, cc, taken, positive, wave, lane, col, K, a.top, out);
}

// the splits' partial lists in `work`, merged per column into `out`
template <int TOP, typename Args, typename Out>
__device__ __forceinline__ void merge_body(const Args& a, int64_t splits, const Out& out) {
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int64_t K = a.K;
    const int64_t col = (int64_t)blockIdx.x * RA_TILE + lane;
    const bool live = col < K;
    const int top = a.top;
    const WorkView w = work_view(a.work, splits, K, top);
    uint64_t ck[TOP];
    int32_t cc[TOP];
#pragma unroll
    for (int i = 0; i < TOP; ++i) {
        ck[i] = 0;
        cc[i] = NO_COL;
    }
    int32_t taken = 0, positive = 0;
    for (int64_t s = wave; s < splits; s += RA_WAVES) {  // wave-uniform
        uint64_t k[TOP];
        int32_t r[TOP];
#pragma unroll
        for (int j = 0; j < TOP; ++j) {
            const bool in = live && j < top;
            const int64_t o = (s * top + (j < top ? j : 0)) * K + (live ? col : 0);
            k[j] = in ? w.keys[o] : 0ull;
            r[j] = in ? w.rows[o] : NO_COL;
        }
        taken += live ? w.cnt[(s * 2 + 0) * K + col] : 0;
        positive += live ? w.cnt[(s * 2 + 1) * K + col] : 0;
#pragma unroll
        for (int j = 0; j < TOP; ++j) {
            if (__builtin_amdgcn_ballot_w64(k[j] > ck[TOP - 1]) == 0) continue;
            NVRX_TOPK_INSERT(TOP, ck, cc, k[j], r[j], TOP);
        }
    }
    merge_waves<TOP>(ck, cc, taken, positive, wave, lane, col, K, top, out);
}

// The launch plan of a shape: the one place that decides the grid of both entries.
inline RankPlan plan_of(int64_t R, int64_t K, int top) {
    RankPlan p{0, 1, 0, 0};
    if (R <= 0 || K <= 0) return p;
    p.tiles = (K + RA_TILE - 1) / RA_TILE;
    const int64_t by_rows = (R + RA_MIN_ROWS - 1) / RA_MIN_ROWS;
    const int64_t by_grid = (RA_TARGET_WGS + p.tiles - 1) / p.tiles;
    p.splits = by_rows < by_grid ? by_rows : by_grid;  // monotone in R
    p.rper = (R + p.splits - 1) / p.splits;  // the last splits may be short, or empty
    if (p.splits > 1) p.work_bytes = p.splits * K * ((int64_t)top * 12 + 8);
    return p;
}

}  // namespace
}  // namespace nvrx
