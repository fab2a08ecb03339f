// history_age.hip -- aging of the tail histories on gfx950: every count shifted right, what
// reaches zero forgotten.
//
// No reference counterpart.  The individual tail scores compare a rank with its own history
// (histogram_history.hip, segment_history.hip: dense, 240 u32 bins per element;
// segment_history_compact.hip: compact, 64 B per element), and that history only grows.  Here it
// decays (include/nvrx_straggler.h, "Aging the tail histories"):
//
//   chist_age_kernel   the compact history.  As in segment_history_compact.hip a wave takes four
//                      elements per trip, one per DPP row, with ONE load: lanes 0..11 of a row hold
//                      a count, 12..14 the bucket bytes, 15 n.  A bpermute inside the row hands
//                      each count lane its bucket byte.  The count lanes shift; a ballot gives the
//                      row's 12-bit keep mask; the population count of the mask below a lane is a
//                      kept entry's new index, and an evicted entry takes the index n' + (its rank
//                      among the evicted), pushing zeros: the 12 count lanes form a permutation of
//                      the row, so two ds_permute (count, byte) with every lane active compact the
//                      element and zero its tail at once.  The bytes are re-packed by two quad
//                      DPP ORs and one bpermute into lanes 12..14; lane 15 takes the mask's
//                      population count.  One dword store per lane, the rows of empty elements
//                      (n = 0) masked off.
//                      Deviation from segchist_kernel's grid: aging concerns slots, not columns,
//                      so the [R][stride] elements are one flat array and every WAVE owns one
//                      contiguous run of it (a multiple of 16 elements, HA_UNROLL = 4 trips loaded
//                      before the first is processed); there is no (row, split) grid and no
//                      16-element workgroup trip.  A wave may straddle rows: lane 15 of each DPP
//                      row carries the evicted / full sums of the row it is in and adds them with
//                      a 64-bit device atomic when its run leaves the row (non-zero sums only;
//                      integer adds commute, so every run gives the same result).
//   hist_age_kernel    the dense history: 16-byte vectors, HA_UNROLL loads in flight per lane, a
//                      vector stored only if it held a non-zero word.
// No LDS allocation, no scratch, no atomics on a history (each element has one owner).  Every loop
// is bounded by R * stride (times 60 vectors for the dense history) or by 12.
#include "history_age.h"
#include "histogram_wave.h"

namespace nvrx {
namespace {

constexpr int HA_THREADS = 256;
constexpr int HA_WAVES = HA_THREADS / 64;
constexpr int HA_ROWS = 4;                      // elements per wave trip: one per DPP row
constexpr int HA_UNROLL = 4;                    // trips (compact) / vectors (dense) in flight
constexpr int HA_GRANULE = HA_ROWS * HA_UNROLL; // a wave's run is a whole number of these
constexpr int HA_TARGET_WGS = 2048;             // 256 CUs x 8 workgroups
constexpr int HA_E = NVRX_CHIST_ENTRIES;
constexpr int HA_WORDS = NVRX_CHIST_BYTES / 4;  // 16: one DPP row
static_assert(HA_WORDS == 16 && HA_ROWS * HA_WORDS == NVRX_WAVE, "an element is one DPP row");
static_assert(4 * HA_E + HA_E + 4 == NVRX_CHIST_BYTES && HA_E % 4 == 0, "count[12], bucket[12], n");

__global__ __launch_bounds__(256) void age_clear_kernel(u64* evicted, u64* full, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (evicted) evicted[i] = 0ull;
    if (full) full[i] = 0ull;
}

// elements [w * per_wave, + per_wave) of the E = R * stride elements belong to wave w of the grid
template <bool COUNTS>
__global__ __launch_bounds__(HA_THREADS)
void chist_age_kernel(unsigned* __restrict__ chist, unsigned E, unsigned stride, unsigned per_wave,
                      int shift, u64* evicted, u64* full) {
    const unsigned w = blockIdx.x * HA_WAVES + (unsigned)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u64 first = (u64)w * per_wave;
    if (first >= E) return;  // wave-uniform
    const unsigned begin = (unsigned)first;
    const unsigned end = min(E, begin + per_wave);  // E < 2^31 and per_wave <= E + 15: no wrap
    const int lane = lane_id();
    const unsigned row = lane >> 4, j = lane & 15, rbase = lane & 48;
    const bool entry = j < HA_E;
    // lane 15 of a DPP row: the sums of table row cur_r, whose elements end before row_end
    unsigned cur_r = 0, row_end = 0;
    u64 ev = 0, fu = 0;
    for (unsigned e0 = begin; e0 < end; e0 += HA_GRANULE) {
        unsigned in[HA_UNROLL];
#pragma unroll
        for (int v = 0; v < HA_UNROLL; ++v) {
            const unsigned e = e0 + v * HA_ROWS + row;
            in[v] = e < end ? chist[(size_t)e * HA_WORDS + j] : 0u;
        }
#pragma unroll
        for (int v = 0; v < HA_UNROLL; ++v) {
            if (e0 + v * HA_ROWS >= end) break;  // wave-uniform
            const unsigned e = e0 + v * HA_ROWS + row;
            const unsigned word = in[v];
            // count lanes: the word of lanes 12..14 that holds their bucket byte
            const unsigned got = (unsigned)__builtin_amdgcn_ds_bpermute(
                4 * (int)(rbase + (entry ? HA_E + (j >> 2) : 15u)), (int)word);
            const unsigned bkt = entry ? (got >> (8 * (j & 3))) & 0xFFu : 0u;
            const unsigned c = entry ? word >> shift : 0u;
            // only the count decides: bucket byte 0 with a count is a used entry
            const unsigned km = (unsigned)(__ballot(c != 0u) >> rbase) & ((1u << HA_E) - 1u);
            const uint64_t used = __ballot(j == 15 && word != 0u);  // n != 0
            const bool live = (used >> (rbase + 15)) & 1u;
            const unsigned n2 = (unsigned)__builtin_popcount(km);
            const unsigned below = (unsigned)__builtin_popcount(km & ((1u << j) - 1u));
            const bool keep = (km >> j) & 1u;  // never in lanes 12..15
            // a permutation of the row: the kept entries to the front in order, the evicted ones
            // behind them (they push zeros), lanes 12..15 onto themselves
            const unsigned dst = rbase + (!entry ? j : keep ? below : n2 + (j - below));
            const unsigned c2 = (unsigned)__builtin_amdgcn_ds_permute(4 * (int)dst, (int)c);
            const unsigned b2 = (unsigned)__builtin_amdgcn_ds_permute(4 * (int)dst, (int)(keep ? bkt : 0u));
            // four bytes per word: every lane of a quad ends with the quad's word
            unsigned pk = b2 << (8 * (j & 3));
            pk |= dpp<0xB1>(pk);
            pk |= dpp<0x4E>(pk);
            const unsigned packed = (unsigned)__builtin_amdgcn_ds_bpermute(
                4 * (int)(rbase + (entry ? j : 4u * (j & 3))), (int)pk);
            const unsigned out = entry ? c2 : j == 15 ? n2 : packed;
            if (e < end && live) chist[(size_t)e * HA_WORDS + j] = out;
            if (COUNTS && j == 15 && e < end) {
                if (e >= row_end) {
                    if (ev && evicted) atomicAdd(evicted + cur_r, ev);
                    if (fu && full) atomicAdd(full + cur_r, fu);
                    ev = fu = 0;
                    cur_r = e / stride;
                    row_end = (cur_r + 1u) * stride;  // <= E
                }
                if (live) {
                    ev += word - n2;  // word is n
                    fu += n2 == (unsigned)HA_E ? 1u : 0u;
                }
            }
        }
    }
    if (COUNTS && j == 15) {
        if (ev && evicted) atomicAdd(evicted + cur_r, ev);
        if (fu && full) atomicAdd(full + cur_r, fu);
    }
}

__global__ __launch_bounds__(HA_THREADS)
void hist_age_kernel(u32x4* __restrict__ hist, int64_t nvec, int shift) {
    const int64_t step = (int64_t)gridDim.x * HA_THREADS;
    for (int64_t i0 = (int64_t)blockIdx.x * HA_THREADS + threadIdx.x; i0 < nvec; i0 += HA_UNROLL * step) {
        u32x4 x[HA_UNROLL];
#pragma unroll
        for (int v = 0; v < HA_UNROLL; ++v) {
            const int64_t i = i0 + v * step;
            x[v] = i < nvec ? hist[i] : (u32x4){0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int v = 0; v < HA_UNROLL; ++v) {
            const int64_t i = i0 + v * step;
            const u32x4 y = x[v];
            if (i < nvec && (y.x | y.y | y.z | y.w))
                hist[i] = (u32x4){y.x >> shift, y.y >> shift, y.z >> shift, y.w >> shift};
        }
    }
}

}  // namespace

// Argument checks happen in abi.cpp before this runs: shift in 1..31, R * stride below 2^31.
hipError_t compact_history_age(void* chist, int64_t R, int64_t stride, int shift, uint64_t* evicted,
                               uint64_t* full, hipStream_t st) {
    if (R <= 0 || stride <= 0) return hipSuccess;
    const int64_t E = R * stride;
    // about HA_TARGET_WGS workgroups; a wave's run is a whole number of granules
    int64_t waves = min((E + HA_GRANULE - 1) / HA_GRANULE, (int64_t)HA_TARGET_WGS * HA_WAVES);
    int64_t per_wave = (E + waves - 1) / waves;
    per_wave = (per_wave + HA_GRANULE - 1) / HA_GRANULE * HA_GRANULE;
    waves = (E + per_wave - 1) / per_wave;
    const dim3 grid((unsigned)((waves + HA_WAVES - 1) / HA_WAVES));
    const bool counts = evicted || full;
    if (counts)
        hipLaunchKernelGGL(age_clear_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st,
                           (u64*)evicted, (u64*)full, R);
    if (counts)
        hipLaunchKernelGGL(chist_age_kernel<true>, grid, dim3(HA_THREADS), 0, st, (unsigned*)chist,
                           (unsigned)E, (unsigned)stride, (unsigned)per_wave, shift, (u64*)evicted,
                           (u64*)full);
    else
        hipLaunchKernelGGL(chist_age_kernel<false>, grid, dim3(HA_THREADS), 0, st, (unsigned*)chist,
                           (unsigned)E, (unsigned)stride, (unsigned)per_wave, shift, (u64*)nullptr,
                           (u64*)nullptr);
    return hipGetLastError();
}

hipError_t histogram_history_age(uint32_t* hist, int64_t R, int64_t stride, int shift, hipStream_t st) {
    if (R <= 0 || stride <= 0) return hipSuccess;
    const int64_t nvec = R * stride * HV;  // below 2^31
    const int64_t per_wg = (int64_t)HA_THREADS * HA_UNROLL;
    const int64_t wgs = min((nvec + per_wg - 1) / per_wg, (int64_t)HA_TARGET_WGS);
    hipLaunchKernelGGL(hist_age_kernel, dim3((unsigned)wgs), dim3(HA_THREADS), 0, st, (u32x4*)hist,
                       nvec, shift);
    return hipGetLastError();
}

}  // namespace nvrx
