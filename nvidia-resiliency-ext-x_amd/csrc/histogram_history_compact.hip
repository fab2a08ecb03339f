// histogram_history_compact.hip -- individual tail scores from [R][K][240] counts against the
// compact history, and the conversion between the dense and the compact history, on gfx950.
//
// No reference counterpart.  histogram_history.hip scores counts against a dense history of 960 B
// per (rank, kernel); segment_history_compact.hip scores record streams against the compact one of
// 64 B (include/nvrx_straggler.h, "compact history").  Here the interval arrives as counts and the
// history is compact: SCORE is histogram_history.hip's with H the dense expansion of the element,
// UPDATE the compact history's with c[b] = C[r][k][b].
//
//   histchist_kernel   the grid (rows, splits of K), the split rule and the 16-element workgroup
//                      trip of history_kernel: a wave takes HC_UNROLL = 4 (row, kernel) elements
//                      per trip.  60 lanes load one 16-byte vector of C per element, nontemporal:
//                      lane l owns bins 4l..4l+3 with constant weights.  The trip's four compact
//                      elements arrive in ONE load, one per DPP row (chist_wave.h): a bpermute for
//                      the bucket byte, the u64 row_shr prefix, a ballot and a readlane for T.  The
//                      base sums come from the count lanes; tail, total and the calls from the bin
//                      lanes against the wave-uniform T.
//                      The merge needs no LDS histogram: the interval's bins sit in registers in
//                      bucket order.  The used buckets mark a 4-bit mask in their owning lane (a
//                      loop over n <= 12 entries, readlanes); a wave prefix over the population
//                      counts of nonzero & ~used admits the first 12 - n new buckets; a second
//                      prefix over the kept mask gives every bin its target entry.  A bin is a full
//                      u32 and up to 240 of them fold into one entry, so the per-target sums are
//                      u64: 12 LDS words per wave, added with 64-bit LDS atomics; the lane that owns
//                      a kept bucket adds the old count, saturates and writes count and bucket byte
//                      at the entry's index.  16 lanes store the 64 B.  Each (row, slot) has one
//                      owner: no atomics on the history.  Row sums and folded: DPP + LDS reduction,
//                      the non-zero sums added with 64-bit device atomics (cleared by a kernel on
//                      the stream first).  Integer adds are exact in any order: the result is the
//                      same on every run.
//   tail_score_finalize_kernel<nvrx_histchist_args>   the three separately rounded f64 operations
//                      and strag (histogram_wave.h, as the clear, clear4_folded_kernel).
//   from_dense_kernel  chist = UPDATE of the empty element with the dense counts: the merge above
//                      with no used bucket.  The [R][stride] elements are one flat array; a wave
//                      owns a contiguous run and has HC_UNROLL loads in flight.  Every element is
//                      written in full (an empty one as zeros).
//   to_dense_kernel    the dense expansion: four elements per load as above, per element a loop
//                      over its n <= 12 entries puts each count into the lane that owns its bin,
//                      and 60 lanes store 16 bytes each, zeros included.
// Every loop is bounded by K (R * stride for the conversions), 12 or 4.  No kernel uses scratch
// memory (make asm).

#include "chist_wave.h"

namespace nvrx {
namespace {

constexpr int HC_THREADS = 256;
constexpr int HC_WAVES = HC_THREADS / 64;
constexpr int HC_UNROLL = 4;                     // elements per wave trip: one per DPP row
constexpr int HC_TRIP = HC_WAVES * HC_UNROLL;    // elements per workgroup trip: a split's granule
constexpr int HC_TARGET_WGS = 2048;              // 256 CUs x 8 workgroups
static_assert(HC_UNROLL * CH_WORDS == NVRX_WAVE, "a trip's elements are one load");

// a wave's private LDS for the merge: the u64 sums per target entry and the element being built
struct MergeLds {
    u64 acc[CH_E];
    unsigned out[CH_WORDS];
};

// UPDATE of one element with the interval's bins c (this lane's four, in bucket order).  used: the
// 4-bit mask of this lane's bins that are entries of the element, o their counts, n the element's
// number of entries.  Returns in lanes 0..15 the words of the new element; adds to fold this
// lane's folded samples.  The wave must hold at least one sample.
__device__ __forceinline__ unsigned chist_merge(const u32x4 c, unsigned used, const unsigned (&oo)[4],
                                                int n, MergeLds* m, int lane, u64& fold) {
    if (lane < CH_E) m->acc[lane] = 0ull;
    if (lane < CH_WORDS) m->out[lane] = 0u;
    lds_order();
    const unsigned cc[4] = {c.x, c.y, c.z, c.w};
    const unsigned have = (c.x ? 1u : 0u) | (c.y ? 2u : 0u) | (c.z ? 4u : 0u) | (c.w ? 8u : 0u);
    // admission: the new buckets in ascending order while entries are free
    const unsigned fresh = have & ~used;
    const unsigned nf = (unsigned)__builtin_popcount(fresh);
    const unsigned before = wave_incl_scan_u32(nf) - nf;
    const unsigned room = (unsigned)(CH_E - min(n, CH_E));
    unsigned kept = used;
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (((fresh >> w) & 1u) && before + (unsigned)__builtin_popcount(fresh & ((1u << w) - 1u)) < room)
            kept |= 1u << w;
    // the entry index of every kept bucket, and through it every bin's target
    const unsigned nk = (unsigned)__builtin_popcount(kept);
    const unsigned below = wave_incl_scan_u32(nk) - nk;
    const unsigned n2 = rl(below + nk, 63);  // |S'| >= 1: the interval has a sample
    unsigned at[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        // kept buckets at or below bin 4 lane + w; none: the lowest kept one
        const unsigned upto = below + (unsigned)__builtin_popcount(kept & ((2u << w) - 1u));
        at[w] = max(upto, 1u) - 1u;  // < n2 <= 12
        if (cc[w]) {
            atomicAdd(&m->acc[at[w]], (u64)cc[w]);  // 64 bits: 240 full u32 bins cannot wrap it
            if (!((kept >> w) & 1u)) fold += cc[w];
        }
    }
    lds_order();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if ((kept >> w) & 1u) {  // the one owner of entry at[w]
            const u64 s = (u64)oo[w] + m->acc[at[w]];
            m->out[at[w]] = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)s;
            ((unsigned char*)(m->out + CH_E))[at[w]] = (unsigned char)(4 * lane + w);
        }
    }
    if (lane == 0) m->out[CH_WORDS - 1] = n2;
    lds_order();
    return lane < CH_WORDS ? m->out[lane] : 0u;
}

// kernels [blockIdx.y * kper, + kper) of row blockIdx.x
template <bool SCORE, bool UPDATE, bool CALLS>
__global__ __launch_bounds__(HC_THREADS) void histchist_kernel(nvrx_histchist_args a, int64_t kper) {
    static_assert(SCORE || UPDATE, "nothing to do");
    static_assert(SCORE || !CALLS, "tail_calls belong to the score");
    __shared__ u64 red[HC_WAVES][4];
    __shared__ __attribute__((aligned(16))) MergeLds merge[UPDATE ? HC_WAVES : 1];
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
    const int b0 = 4 * lane;
    const unsigned w0 = weight_of(b0), w1 = weight_of(b0 + 1), w2 = weight_of(b0 + 2),
                   w3 = weight_of(b0 + 3);
    const u32x4* const crow = (const u32x4*)(a.counts + r * K * HB) + lane;
    unsigned* const hrow = (unsigned*)a.chist + r * stride * CH_WORDS;
    const int pm = a.permille;
    MergeLds* const m = merge + (UPDATE ? wave : 0);
    u64 total = 0, tail = 0, btotal = 0, btail = 0, fold = 0;
    for (int64_t k0 = kb + wave; k0 < ke; k0 += HC_TRIP) {
        u32x4 c[HC_UNROLL];
        int64_t slot[HC_UNROLL];
#pragma unroll
        for (int u = 0; u < HC_UNROLL; ++u) {
            const int64_t k = k0 + u * HC_WAVES;  // wave-uniform
            c[u] = (u32x4){0u, 0u, 0u, 0u};
            slot[u] = -1;
            if (k < ke) {
                int64_t s = a.hist_index ? (int64_t)a.hist_index[k] : k;
                if (a.col_valid && !a.col_valid[k]) s = -1;
                slot[u] = s;
                if (s >= 0 && lane < HV) c[u] = __builtin_nontemporal_load(crow + k * HV);
            }
        }
        // the trip's four elements in one load: row u, word j
        const int64_t sl = row == 0 ? slot[0] : row == 1 ? slot[1] : row == 2 ? slot[2] : slot[3];
        const unsigned word = sl >= 0 ? hrow[sl * CH_WORDS + j] : 0u;
        unsigned cnt, bkt;
        chist_entry(word, lane, j, cnt, bkt);
        const u64 incl = SCORE ? row_incl_scan_u64((u64)cnt) : 0ull;
        const u64 wsum = (u64)cnt * weight_of((int)bkt);
#pragma unroll
        for (int u = 0; u < HC_UNROLL; ++u) {
            const int64_t k = k0 + u * HC_WAVES;
            const int64_t s = slot[u];
            const u32x4 q = c[u];
            // lanes 60..63 hold zeros; an interval without samples is neither scored nor absorbed
            const bool any = s >= 0 && __ballot((q.x | q.y | q.z | q.w) != 0u) != 0ull;  // wave-uniform
            if (SCORE) {
                unsigned calls = 0;
                const u64 N = rl_u64(incl, 16 * u + 15);  // lanes 12..15 add nothing
                if (any && N != 0) {
                    const bool mine = row == u;
                    const int t = chist_threshold(incl, bkt, mine, u, pm, N);
                    if (mine) {
                        btotal += wsum;
                        btail += (int)bkt > t ? wsum : 0ull;
                    }
                    const bool t0 = b0 > t, t1 = b0 + 1 > t, t2 = b0 + 2 > t, t3 = b0 + 3 > t;
                    const u64 p0 = (u64)q.x * w0, p1 = (u64)q.y * w1, p2 = (u64)q.z * w2,
                              p3 = (u64)q.w * w3;
                    total += (p0 + p1) + (p2 + p3);
                    tail += ((t0 ? p0 : 0ull) + (t1 ? p1 : 0ull)) + ((t2 ? p2 : 0ull) + (t3 ? p3 : 0ull));
                    if (CALLS)
                        calls = wave_sum_u32(((t0 ? q.x : 0u) + (t1 ? q.y : 0u)) +
                                             ((t2 ? q.z : 0u) + (t3 ? q.w : 0u)));
                }
                if (CALLS && k < ke && lane == 0) a.tail_calls[r * K + k] = calls;
            }
            if (UPDATE) {
                if (absorb && any) {  // wave-uniform
                    const int n = (int)rl(word, 16 * u + 15);  // <= 12 by the canonical form
                    unsigned used = 0, o0 = 0, o1 = 0, o2 = 0, o3 = 0;  // S and its counts, by bin
                    for (int e = 0; e < min(n, CH_E); ++e) {
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
                    const unsigned oo[4] = {o0, o1, o2, o3};
                    const unsigned out = chist_merge(q, used, oo, n, m, lane, fold);
                    if (lane < CH_WORDS) hrow[s * CH_WORDS + lane] = out;
                }
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
    for (int w = 0; w < HC_WAVES; ++w) v += red[w][threadIdx.x];
    uint64_t* const dst = threadIdx.x == 0 ? a.tail_ns : threadIdx.x == 1 ? a.total_ns
                        : threadIdx.x == 2 ? a.base_tail_ns : a.base_total_ns;
    if (v) atomicAdd((u64*)dst + r, v);
}

template <bool SCORE, bool UPDATE, bool CALLS>
void launch_histchist(const nvrx_histchist_args& a, dim3 grid, int64_t kper, hipStream_t st) {
    hipLaunchKernelGGL((histchist_kernel<SCORE, UPDATE, CALLS>), grid, dim3(HC_THREADS), 0, st, a, kper);
}

__global__ __launch_bounds__(256) void convert_clear_kernel(u64* folded, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) folded[i] = 0ull;
}

// elements [w * per_wave, + per_wave) of the E = R * stride elements belong to wave w of the grid
__global__ __launch_bounds__(HC_THREADS)
void from_dense_kernel(const u32x4* __restrict__ hist, unsigned* __restrict__ chist, int64_t E,
                       int64_t stride, int64_t per_wave, u64* folded) {
    __shared__ __attribute__((aligned(16))) MergeLds merge[HC_WAVES];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t begin = ((int64_t)blockIdx.x * HC_WAVES + wave) * per_wave;
    if (begin >= E) return;  // wave-uniform
    const int64_t end = min(E, begin + per_wave);
    const int lane = lane_id();
    MergeLds* const m = merge + wave;
    const unsigned none[4] = {0u, 0u, 0u, 0u};
    for (int64_t e0 = begin; e0 < end; e0 += HC_UNROLL) {
        u32x4 h[HC_UNROLL];
#pragma unroll
        for (int u = 0; u < HC_UNROLL; ++u) {
            h[u] = (u32x4){0u, 0u, 0u, 0u};
            if (e0 + u < end && lane < HV) h[u] = __builtin_nontemporal_load(hist + (e0 + u) * HV + lane);
        }
#pragma unroll
        for (int u = 0; u < HC_UNROLL; ++u) {
            const int64_t e = e0 + u;
            if (e >= end) break;  // wave-uniform
            const u32x4 q = h[u];
            unsigned out = 0u;  // an empty dense element: the all-zero element
            if (__ballot((q.x | q.y | q.z | q.w) != 0u) != 0ull) {  // wave-uniform
                u64 fold = 0;
                out = chist_merge(q, 0u, none, 0, m, lane, fold);
                if (folded) {
                    fold = wave_sum_u64(fold);
                    if (lane == 0 && fold) atomicAdd(folded + e / stride, fold);
                }
            }
            if (lane < CH_WORDS) chist[e * CH_WORDS + lane] = out;
        }
    }
}

__global__ __launch_bounds__(HC_THREADS)
void to_dense_kernel(const unsigned* __restrict__ chist, u32x4* __restrict__ hist, int64_t E,
                     int64_t per_wave) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t begin = ((int64_t)blockIdx.x * HC_WAVES + wave) * per_wave;
    if (begin >= E) return;  // wave-uniform
    const int64_t end = min(E, begin + per_wave);
    const int lane = lane_id();
    const int row = lane >> 4, j = lane & 15;
    for (int64_t e0 = begin; e0 < end; e0 += HC_UNROLL) {
        const int64_t el = e0 + row;
        const unsigned word = el < end ? chist[el * CH_WORDS + j] : 0u;
        unsigned cnt, bkt;
        chist_entry(word, lane, j, cnt, bkt);
#pragma unroll
        for (int u = 0; u < HC_UNROLL; ++u) {
            const int64_t e = e0 + u;
            if (e >= end) break;  // wave-uniform
            const int n = (int)rl(word, 16 * u + 15);  // <= 12 by the canonical form
            unsigned o0 = 0, o1 = 0, o2 = 0, o3 = 0;
            for (int i = 0; i < min(n, CH_E); ++i) {
                const unsigned eb = rl(bkt, 16 * u + i), ec = rl(cnt, 16 * u + i);
                if (lane == (int)(eb >> 2)) {
                    const unsigned w = eb & 3u;
                    o0 = w == 0 ? ec : o0;
                    o1 = w == 1 ? ec : o1;
                    o2 = w == 2 ? ec : o2;
                    o3 = w == 3 ? ec : o3;
                }
            }
            if (lane < HV) hist[e * HV + lane] = (u32x4){o0, o1, o2, o3};
        }
    }
}

// a wave's contiguous run of the E elements: about HC_TARGET_WGS workgroups, a whole number of trips
void convert_grid(int64_t E, int64_t& per_wave, dim3& grid) {
    int64_t waves = min((E + HC_UNROLL - 1) / HC_UNROLL, (int64_t)HC_TARGET_WGS * HC_WAVES);
    per_wave = (E + waves - 1) / waves;
    per_wave = (per_wave + HC_UNROLL - 1) / HC_UNROLL * HC_UNROLL;
    waves = (E + per_wave - 1) / per_wave;
    grid = dim3((unsigned)((waves + HC_WAVES - 1) / HC_WAVES));
}

}  // namespace

// Argument checks happen in abi.cpp before this runs.
hipError_t histogram_history_scores_compact(const nvrx_histchist_args& a, hipStream_t st) {
    if (a.R <= 0 || a.K <= 0) return hipSuccess;
    const bool score = a.mode & NVRX_HTAIL_SCORE, update = a.mode & NVRX_HTAIL_UPDATE;
    int64_t kper;
    const int64_t splits = row_splits(a.R, a.K, HC_TRIP, HC_TARGET_WGS, &kper);
    const dim3 grid((unsigned)a.R, (unsigned)splits);
    const dim3 rows((unsigned)((a.R + 255) / 256));
    hipLaunchKernelGGL(clear4_folded_kernel<u64>, rows, dim3(256), 0, st,
                       score ? (u64*)a.tail_ns : nullptr, (u64*)a.total_ns, (u64*)a.base_tail_ns,
                       (u64*)a.base_total_ns, update ? (u64*)a.folded : nullptr, a.R);
    if (!score)
        launch_histchist<false, true, false>(a, grid, kper, st);
    else if (update)
        a.tail_calls ? launch_histchist<true, true, true>(a, grid, kper, st)
                     : launch_histchist<true, true, false>(a, grid, kper, st);
    else
        a.tail_calls ? launch_histchist<true, false, true>(a, grid, kper, st)
                     : launch_histchist<true, false, false>(a, grid, kper, st);
    if (score)
        hipLaunchKernelGGL(tail_score_finalize_kernel<nvrx_histchist_args>, rows, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t compact_history_from_dense(const uint32_t* hist, void* chist, int64_t R, int64_t stride,
                                      uint64_t* folded, hipStream_t st) {
    if (R <= 0 || stride <= 0) return hipSuccess;
    int64_t per_wave;
    dim3 grid;
    convert_grid(R * stride, per_wave, grid);
    if (folded)
        hipLaunchKernelGGL(convert_clear_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st,
                           (u64*)folded, R);
    hipLaunchKernelGGL(from_dense_kernel, grid, dim3(HC_THREADS), 0, st, (const u32x4*)hist,
                       (unsigned*)chist, R * stride, stride, per_wave, (u64*)folded);
    return hipGetLastError();
}

hipError_t compact_history_to_dense(const void* chist, uint32_t* hist, int64_t R, int64_t stride,
                                    hipStream_t st) {
    if (R <= 0 || stride <= 0) return hipSuccess;
    int64_t per_wave;
    dim3 grid;
    convert_grid(R * stride, per_wave, grid);
    hipLaunchKernelGGL(to_dense_kernel, grid, dim3(HC_THREADS), 0, st, (const unsigned*)chist,
                       (u32x4*)hist, R * stride, per_wave);
    return hipGetLastError();
}

}  // namespace nvrx
