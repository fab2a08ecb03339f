// chist_wave.h -- what the kernels on the compact history share (segment_history_compact.hip:
// record streams; histogram_history_compact.hip: [R][K][240] counts and the dense / compact
// conversion; segment_history_compact_attribution.hip and
// histogram_history_compact_attribution.hip: the base of four elements side by side, rows_base): a
// wave holds four 64-byte elements, one per DPP row, one dword per lane -- lanes 0..11 of a row a
// count, 12..14 the bucket bytes, 15 n (include/nvrx_straggler.h, "Element layout").
#pragma once
#include "histogram_wave.h"

namespace nvrx {
namespace {

constexpr int CH_E = NVRX_CHIST_ENTRIES;
constexpr int CH_WORDS = NVRX_CHIST_BYTES / 4;  // 16: one DPP row
constexpr int CH_ROWS = NVRX_WAVE / CH_WORDS;   // 4: the elements a wave holds
static_assert(CH_WORDS == 16 && 4 * CH_WORDS == NVRX_WAVE, "an element is one DPP row");
static_assert(4 * CH_E + CH_E + 4 == NVRX_CHIST_BYTES && CH_E % 4 == 0, "count[12], bucket[12], n");

// the wave's LDS operations before this are done and visible before those after it
__device__ __forceinline__ void lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// inclusive u64 prefix inside each 16-lane row (row_shr zero-fills at the row's start)
__device__ __forceinline__ u64 row_incl_scan_u64(u64 v) {
    v += dpp_u64<0x111>(v);
    v += dpp_u64<0x112>(v);
    v += dpp_u64<0x114>(v);
    v += dpp_u64<0x118>(v);
    return v;
}

// word: this lane's dword (j = lane & 15) of its row's element.  Lanes 0..11 of a row get the
// entry's count and bucket (zero beyond n, by the canonical form), lanes 12..15 zeros: a bpermute
// inside the row hands each count lane the word that holds its bucket byte.
__device__ __forceinline__ void chist_entry(unsigned word, int lane, int j, unsigned& cnt, unsigned& bkt) {
    const unsigned bytes = (unsigned)__builtin_amdgcn_ds_bpermute(4 * ((lane & 48) + CH_E + (j >> 2)),
                                                                  (int)word);
    const bool entry = j < CH_E;
    cnt = entry ? word : 0u;
    bkt = entry ? (bytes >> (8 * (j & 3))) & 0xFFu : 0u;
}

// T of the element in row u with N > 0 samples: the bucket of its sample of 0-based rank
// (pm (N - 1)) / 1000.  incl: row_incl_scan_u64 of the counts; mine: this lane is in row u.
__device__ __forceinline__ int chist_threshold(u64 incl, unsigned bkt, bool mine, int u, int pm, u64 N) {
    // (pm (N - 1)) / 1000 without the product leaving 64 bits
    const u64 d = (N - 1) / 1000ull, mm = (N - 1) % 1000ull;
    const u64 rank = (u64)pm * d + ((u64)pm * mm) / 1000ull;
    // incl is non-decreasing over the row and incl[11] = N > rank: the entries at
    // or below rank are a prefix, and the entry after them has a count
    const int L = (int)__popcll(__ballot(mine && incl <= rank));
    return (int)rl(bkt, 16 * u + L);
}

// What the two attributions against the compact history share
// (segment_history_compact_attribution.hip, histogram_history_compact_attribution.hip): the base
// of a trip's four elements, side by side in the rows.

// the sum of each 16-lane row in every lane of the row: the DPP steps of wave_sum_u64
__device__ __forceinline__ u64 row_sum_u64(u64 v) {
    v += dpp_u64<0xB1>(v);
    v += dpp_u64<0x4E>(v);
    v += dpp_u64<0x141>(v);
    v += dpp_u64<0x140>(v);
    return v;
}

// a wave-uniform value per row, picked by the lane's row
template <typename T>
__device__ __forceinline__ T by_row(int row, T v0, T v1, T v2, T v3) {
    return row == 0 ? v0 : row == 1 ? v1 : row == 2 ? v2 : v3;
}

// What four elements' histories give, side by side: btail / btotal are the row's sums (in every
// lane of row u for element u); T and elig (N > 0) are wave-uniform.
struct RowBase {
    u64 btail, btotal;
    int T[CH_ROWS];
    bool elig[CH_ROWS];
};

// word: row u, lane j holds dword j of element u (zero: the empty history)
__device__ __forceinline__ RowBase rows_base(unsigned word, int pm, int lane) {
    const int row = lane >> 4, j = lane & 15;
    // lanes 0..11 of a row: the entry's count and bucket (zero beyond n, by the canonical form)
    const unsigned bytes = (unsigned)__builtin_amdgcn_ds_bpermute(4 * ((lane & 48) + CH_E + (j >> 2)),
                                                                  (int)word);
    const bool entry = j < CH_E;
    const unsigned cnt = entry ? word : 0u;
    const unsigned bkt = entry ? (bytes >> (8 * (j & 3))) & 0xFFu : 0u;
    const u64 incl = row_incl_scan_u64((u64)cnt);
    // lanes 12..15 add nothing: the row's last lane holds N
    const u64 n0 = rl_u64(incl, 15), n1 = rl_u64(incl, 31), n2 = rl_u64(incl, 47), n3 = rl_u64(incl, 63);
    const u64 N = by_row(row, n0, n1, n2, n3);
    // (pm (N - 1)) / 1000 without the product leaving 64 bits (N == 0: no rank, nothing below it)
    const u64 N1 = N ? N - 1 : 0ull;
    const u64 d = N1 / 1000ull, mm = N1 % 1000ull;
    const u64 rank = (u64)pm * d + ((u64)pm * mm) / 1000ull;
    // incl is non-decreasing over the row and incl[11] = N > rank: the entries at or below rank
    // are a prefix, and the entry after them has a count
    const uint64_t below = __ballot(entry && N != 0 && incl <= rank);
    RowBase b;
    b.elig[0] = n0 != 0;
    b.elig[1] = n1 != 0;
    b.elig[2] = n2 != 0;
    b.elig[3] = n3 != 0;
#pragma unroll
    for (int u = 0; u < CH_ROWS; ++u) {
        const int L = __builtin_popcount((unsigned)(below >> (16 * u)) & 0xFFFFu);  // <= 11
        b.T[u] = b.elig[u] ? (int)rl(bkt, 16 * u + L) : -1;
    }
    const int t = by_row(row, b.T[0], b.T[1], b.T[2], b.T[3]);
    const u64 wsum = (u64)cnt * weight_of((int)bkt);
    b.btotal = row_sum_u64(wsum);
    b.btail = row_sum_u64((int)bkt > t ? wsum : 0ull);
    return b;
}

}  // namespace
}  // namespace nvrx
