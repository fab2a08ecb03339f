// chist_wave.h -- what the kernels on the compact history share (segment_history_compact.hip:
// record streams; histogram_history_compact.hip: [R][K][240] counts and the dense / compact
// conversion; segment_history_compact_attribution.hip: the row prefix): a wave holds four 64-byte elements, one per DPP row, one dword per lane -- lanes
// 0..11 of a row a count, 12..14 the bucket bytes, 15 n (include/nvrx_straggler.h, "Element
// layout").
#pragma once
#include "histogram_wave.h"

namespace nvrx {
namespace {

constexpr int CH_E = NVRX_CHIST_ENTRIES;
constexpr int CH_WORDS = NVRX_CHIST_BYTES / 4;  // 16: one DPP row
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

}  // namespace
}  // namespace nvrx
