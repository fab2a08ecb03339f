// segment_history_compact.hip -- individual tail scores straight from ragged segments against a
// compact history, on gfx950.
//
// No reference counterpart.  segment_history.hip scores a rank against a dense history of 240 u32
// bins per (rank, kernel): 960 B, of which a real kernel uses one to three bins.  Here an element
// is 64 B (include/nvrx_straggler.h, "compact history"): u32 count[12], u8 bucket[12], u32 n, the
// used entries in ascending bucket order.  SCORE is segment_history.hip's score with H the dense
// expansion of the element; UPDATE admits the interval's new buckets in ascending order while
// entries are free and folds every other sample into the nearest kept bucket at or below it (the
// lowest kept one if there is none), counting the folded samples per row.
//
//   segchist_kernel    the grid (rows, splits of K), the split rule and the 16-element workgroup
//                      trip of seghist_kernel.  A wave takes SC_UNROLL = 4 (row, kernel) elements
//                      per trip and loads them with ONE instruction: DPP row u (lanes 16u..16u+15)
//                      holds element u, one dword per lane -- lanes 0..11 a count, 12..14 the
//                      bucket bytes, 15 n.  A bpermute inside the row hands each count lane its
//                      bucket byte; the u64 row_shr prefix over the counts gives N in the row's
//                      last lane, a ballot over the row the entry that holds the sample of rank
//                      (pm (N - 1)) / 1000, a readlane its bucket T.  The base sums are
//                      count * weight_of(bucket) per lane.  The retained run is walked as in
//                      segment_history.hip: 64 samples per load, SC_LOADS loads in flight, per-lane
//                      u64 total / tail, the calls by ballot and population count.
//                      With UPDATE the interval's bins are counted in a wave-private LDS histogram
//                      of 256 words (count_wave of segment_history.hip), chosen over carrying
//                      count_wave's leaders in registers because the merge needs every bin in
//                      bucket order and the 16 words behind the 240 bins hold the element being
//                      built.  The merge: a lane owns four bins; the used buckets mark their lanes
//                      (a loop over n <= 12 entries, readlanes); the new buckets are ranked by a
//                      wave prefix over the population counts and admitted while entries are free;
//                      a second prefix over the kept buckets gives every bin the index of its
//                      target entry, to which its count is added in LDS (u32: a run is at most
//                      2^30 samples); the lane that owns a kept bucket then adds the old count,
//                      saturating, and writes count and bucket byte at the entry's index.  16 lanes
//                      store the 64 B.  Each (row, slot) has one owner: no atomics on the history.
//                      Row sums and folded: DPP + LDS reduction, the non-zero sums added with
//                      64-bit device atomics (cleared by a kernel on the stream first).  Integer
//                      adds are exact in any order: the result is the same on every run.
//   tail_score_finalize_kernel<nvrx_segchist_args>   the three separately rounded f64 operations
//                      and strag (histogram_wave.h, as the clear, clear4_folded_kernel).
// bucket_of, sat_add, count_wave and slot_of are histogram_wave.h's too; the element's load and
// decode and lds_order live in chist_wave.h, shared with histogram_history_compact.hip and
// segment_history_compact_attribution.hip.  Every loop is bounded by K, by the retained length or
// by 12.  No kernel uses scratch memory (make asm).

#include "chist_wave.h"
#include "segment_addr.h"

namespace nvrx {
namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_UNROLL = 4;                     // elements per wave trip: one per DPP row
constexpr int SC_TRIP = SC_WAVES * SC_UNROLL;    // elements per workgroup trip: a split's granule
constexpr int SC_TARGET_WGS = 2048;              // 256 CUs x 8 workgroups
constexpr int SC_LOADS = 4;                      // sample loads in flight per lane
constexpr int SC_HW = 256;                       // LDS words per wave: 240 bins + the element built
constexpr int SC_E = CH_E;
constexpr int SC_WORDS = CH_WORDS;               // 16: one DPP row
constexpr unsigned SC_NONE = HB;                 // the bucket of a lane past the run's end
static_assert(SC_WORDS == 16 && SC_UNROLL * SC_WORDS == NVRX_WAVE, "an element is one DPP row");
static_assert(SC_HW == HB + SC_WORDS && SC_HW == 4 * NVRX_WAVE, "one 16-byte vector per lane clears it");
static_assert(4 * SC_E + SC_E + 4 == NVRX_CHIST_BYTES, "count[12], bucket[12], n");

// kernels [blockIdx.y * kper, + kper) of row blockIdx.x
template <bool SCORE, bool UPDATE, bool CALLS>
__global__ __launch_bounds__(SC_THREADS)
void segchist_kernel(RaggedSegs segs, nvrx_segchist_args a, int64_t kper) {
    static_assert(SCORE || UPDATE, "nothing to do");
    static_assert(SCORE || !CALLS, "tail_calls belong to the score");
    __shared__ u64 red[SC_WAVES][4];
    __shared__ __attribute__((aligned(16))) unsigned bins[UPDATE ? SC_WAVES * SC_HW : 4];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int row = lane >> 4, j = lane & 15;  // the element of the trip this lane holds a word of
    const int64_t r = blockIdx.x;
    const int64_t K = a.K;
    const bool absorb = UPDATE && !(a.skip_rows && a.skip_rows[r]);  // workgroup-uniform
    const int64_t kb = (int64_t)blockIdx.y * kper;
    // a skipped row of the update-only pass has no work
    const int64_t ke = SCORE || absorb ? min(K, kb + kper) : kb;
    const int64_t stride = a.hist_stride ? a.hist_stride : K;
    unsigned* const crow = (unsigned*)a.chist + r * stride * SC_WORDS;
    const int pm = a.permille;
    unsigned* const hb = bins + (UPDATE ? wave * SC_HW : 0);
    u64 total = 0, tail = 0, btotal = 0, btail = 0, fold = 0;
    for (int64_t k0 = kb + wave; k0 < ke; k0 += SC_TRIP) {
        int64_t slot[SC_UNROLL];
        const uint32_t* run[SC_UNROLL];
        int len[SC_UNROLL];
#pragma unroll
        for (int u = 0; u < SC_UNROLL; ++u) {
            const int64_t k = k0 + u * SC_WAVES;  // wave-uniform, and so is all that follows from it
            slot[u] = -1;
            run[u] = nullptr;
            len[u] = 0;
            if (k < ke) {
                int64_t s = slot_of(a, k);
                if (s >= 0) segs.get(r * K + k, run[u], len[u]);
                if (len[u] <= 0) s = -1;  // an empty element: no score, no update, no read of the history
                slot[u] = s;
            }
        }
        // the trip's four elements in one load: row u, word j
        const int64_t sl = row == 0 ? slot[0] : row == 1 ? slot[1] : row == 2 ? slot[2] : slot[3];
        const unsigned word = sl >= 0 ? crow[sl * SC_WORDS + j] : 0u;
        // lanes 0..11 of a row: the entry's count and bucket (zero beyond n, by the canonical form)
        unsigned cnt, bkt;
        chist_entry(word, lane, j, cnt, bkt);
        const u64 incl = SCORE ? row_incl_scan_u64((u64)cnt) : 0ull;
        const u64 wsum = (u64)cnt * weight_of((int)bkt);
#pragma unroll
        for (int u = 0; u < SC_UNROLL; ++u) {
            const int64_t k = k0 + u * SC_WAVES;
            const int64_t s = slot[u];
            if (s < 0) {  // wave-uniform
                if (CALLS && k < ke && lane == 0) a.tail_calls[r * K + k] = 0u;
                continue;
            }
            const uint32_t* const q = run[u];
            const int m = len[u];
            const bool mine = row == u;
            const bool count = UPDATE && absorb;
            bool elig = false;
            int t = HB;  // no bucket lies above it
            if (SCORE) {
                const u64 N = rl_u64(incl, 16 * u + 15);  // lanes 12..15 add nothing
                if (N != 0) {
                    elig = true;
                    t = chist_threshold(incl, bkt, mine, u, pm, N);
                    if (mine) {
                        btotal += wsum;
                        btail += (int)bkt > t ? wsum : 0ull;
                    }
                }
            }
            if (count) {
                *(u32x4*)(hb + 4 * lane) = (u32x4){0u, 0u, 0u, 0u};
                lds_order();
            }
            unsigned calls = 0;
            if (elig || count) {  // wave-uniform
                for (int base = 0; base < m; base += 64 * SC_LOADS) {
                    unsigned x[SC_LOADS];
#pragma unroll
                    for (int v = 0; v < SC_LOADS; ++v) {
                        const int i = base + v * 64 + lane;
                        x[v] = i < m ? __builtin_nontemporal_load(q + i) : 0u;
                    }
#pragma unroll
                    for (int v = 0; v < SC_LOADS; ++v) {
                        if (base + v * 64 >= m) break;  // wave-uniform
                        const bool live = base + v * 64 + lane < m;
                        const unsigned b = bucket_of(x[v]);
                        if (SCORE && elig) {
                            const u64 w = live ? (u64)weight_of((int)b) : 0ull;
                            const bool hit = live && (int)b > t;
                            total += w;
                            tail += hit ? w : 0ull;
                            if (CALLS) calls += (unsigned)__popcll(__ballot(hit));
                        }
                        if (count) count_wave<SC_NONE>(live ? b : SC_NONE, hb);
                    }
                }
            }
            if (CALLS && lane == 0) a.tail_calls[r * K + k] = calls;
            if (count) {
                lds_order();
                // this lane's four bins (lanes 60..63 read the zeroed words behind the bins)
                const u32x4 c = *(const u32x4*)(hb + 4 * lane);
                const int n = (int)rl(word, 16 * u + 15);  // <= 12 by the canonical form
                unsigned used = 0, o0 = 0, o1 = 0, o2 = 0, o3 = 0;  // S and its counts, by bin
                for (int e = 0; e < min(n, SC_E); ++e) {
                    const unsigned eb = rl(bkt, 16 * u + e), ec = rl(cnt, 16 * u + e);
                    if (lane == (int)(eb >> 2)) {
                        const unsigned w = eb & 3u;
                        used |= 1u << w;
                        o0 = w == 0 ? ec : o0;
                        o1 = w == 1 ? ec : o1;
                        o2 = w == 2 ? ec : o2;
                        o3 = w == 3 ? ec : o3;
                    }
                }
                const unsigned have = (c.x ? 1u : 0u) | (c.y ? 2u : 0u) | (c.z ? 4u : 0u) | (c.w ? 8u : 0u);
                // admission: the new buckets in ascending order while entries are free
                const unsigned fresh = have & ~used;
                const unsigned nf = (unsigned)__builtin_popcount(fresh);
                const unsigned before = wave_incl_scan_u32(nf) - nf;
                const unsigned room = (unsigned)(SC_E - min(n, SC_E));
                unsigned kept = used;
#pragma unroll
                for (int w = 0; w < 4; ++w)
                    if (((fresh >> w) & 1u) && before + (unsigned)__builtin_popcount(fresh & ((1u << w) - 1u)) < room)
                        kept |= 1u << w;
                // the entry index of every kept bucket, and through it every bin's target
                const unsigned nk = (unsigned)__builtin_popcount(kept);
                const unsigned below = wave_incl_scan_u32(nk) - nk;
                const unsigned n2 = rl(below + nk, 63);  // |S'| >= 1: the run has a sample
                const unsigned cc[4] = {c.x, c.y, c.z, c.w};
                const unsigned oo[4] = {o0, o1, o2, o3};
                unsigned at[4];
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    // kept buckets at or below bin 4 lane + w; none: the lowest kept one
                    const unsigned upto = below + (unsigned)__builtin_popcount(kept & ((2u << w) - 1u));
                    at[w] = max(upto, 1u) - 1u;
                    if (cc[w]) {
                        atomicAdd(&hb[HB + at[w]], cc[w]);
                        if (!((kept >> w) & 1u)) fold += cc[w];
                    }
                }
                lds_order();
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    if ((kept >> w) & 1u) {  // the one owner of entry at[w]
                        hb[HB + at[w]] = sat_add(oo[w], hb[HB + at[w]]);
                        ((unsigned char*)(hb + HB + SC_E))[at[w]] = (unsigned char)(4 * lane + w);
                    }
                }
                if (lane == 0) hb[HB + SC_WORDS - 1] = n2;
                lds_order();
                if (lane < SC_WORDS) crow[s * SC_WORDS + lane] = hb[HB + lane];
            }
        }
    }
    if (UPDATE) {
        fold = wave_sum_u64(fold);
        if (lane == 0 && fold) atomicAdd((u64*)a.folded + r, fold);
    }
    if (!SCORE) return;  // the update-only instantiation has no barrier
    total = wave_sum_u64(total);
    tail = wave_sum_u64(tail);
    btotal = wave_sum_u64(btotal);
    btail = wave_sum_u64(btail);
    if (lane == 0) {
        red[wave][0] = tail;
        red[wave][1] = total;
        red[wave][2] = btail;
        red[wave][3] = btotal;
    }
    __syncthreads();
    if (threadIdx.x >= 4) return;
    u64 v = 0;
#pragma unroll
    for (int w = 0; w < SC_WAVES; ++w) v += red[w][threadIdx.x];
    uint64_t* const dst = threadIdx.x == 0 ? a.tail_ns : threadIdx.x == 1 ? a.total_ns
                        : threadIdx.x == 2 ? a.base_tail_ns : a.base_total_ns;
    if (v) atomicAdd((u64*)dst + r, v);
}

template <bool SCORE, bool UPDATE, bool CALLS>
void launch_segchist(const nvrx_segchist_args& a, dim3 grid, int64_t kper, hipStream_t st) {
    hipLaunchKernelGGL((segchist_kernel<SCORE, UPDATE, CALLS>), grid, dim3(SC_THREADS), 0, st,
                       RaggedSegs{a.ns, a.seg_off, a.seg_len, a.cap}, a, kper);
}

}  // namespace

// Argument checks happen in abi.cpp before this runs.
hipError_t segment_history_scores_compact_ragged(const nvrx_segchist_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    const bool score = a.mode & NVRX_HTAIL_SCORE, update = a.mode & NVRX_HTAIL_UPDATE;
    int64_t kper;
    const int64_t splits = row_splits(a.R, a.K, SC_TRIP, SC_TARGET_WGS, &kper);
    const dim3 grid((unsigned)a.R, (unsigned)splits);
    const dim3 rows((unsigned)((a.R + 255) / 256));
    hipLaunchKernelGGL(clear4_folded_kernel<u64>, rows, dim3(256), 0, st,
                       score ? (u64*)a.tail_ns : nullptr, (u64*)a.total_ns, (u64*)a.base_tail_ns,
                       (u64*)a.base_total_ns, update ? (u64*)a.folded : nullptr, a.R);
    if (!score)
        launch_segchist<false, true, false>(a, grid, kper, st);
    else if (update)
        a.tail_calls ? launch_segchist<true, true, true>(a, grid, kper, st)
                     : launch_segchist<true, true, false>(a, grid, kper, st);
    else
        a.tail_calls ? launch_segchist<true, false, true>(a, grid, kper, st)
                     : launch_segchist<true, false, false>(a, grid, kper, st);
    if (score)
        hipLaunchKernelGGL(tail_score_finalize_kernel<nvrx_segchist_args>, rows, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace nvrx
