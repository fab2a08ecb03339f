// segment_wave.h -- one wave per segment held in registers: the buffer loads, the histogram
// geometry and lean_core (FAST mode; see segment_stats.hip for the algorithm).
#pragma once
#include <type_traits>

#include "segment_addr.h"

namespace nvrx {

constexpr int BINS_PER_SAMPLE_SHORT = 16;  // bins per lane-sample, PL <= 8
template <int PL>
struct Bins {
    // bins per wave: 16 per lane-sample for short segments (PL <= 16: C3's 1024 samples take
    // 256 bins -- fewer bucket-mates of the median to compact and rank, 3-5 % faster than 128,
    // while 512 was slower), 8 above (PL = 32 was fastest at 256)
    static constexpr int PB = PL <= 8 ? BINS_PER_SAMPLE_SHORT * PL : PL <= 16 ? 16 * PL : 8 * PL;
    static constexpr int NB = PB < 64 ? 64 : PB > 512 ? 512 : PB;
    static constexpr int BPL = NB / 64;                     // bins per lane
    static constexpr int LOG = (NB == 64) ? 6 : (NB == 128) ? 7 : (NB == 256) ? 8 : (NB == 512) ? 9 : 10;
    static_assert((1 << LOG) == NB, "NB must be a power of two <= 1024");
};

// Locate the bucket holding relative rank ta in the wave's histogram (one read of the bins):
// bucket index, elements in lower buckets, count of the bucket.  Vector work is the row-wise
// inclusive prefix of the lanes' bin sums (DPP row shifts) and one compare; the row holding ta,
// the lane inside it (ballot), that lane's bins (readlanes) and the walk over them are scalar.
template <int PL>
__device__ __forceinline__ void hist_locate1(const unsigned* hist, unsigned ta, unsigned& ba,
                                             unsigned& bfa, unsigned& ca) {
    constexpr int BPL = Bins<PL>::BPL;
    const int lane = lane_id();
    unsigned h[BPL];
    unsigned local = 0;
#pragma unroll
    for (int j = 0; j < BPL; ++j) {
        h[j] = hist[lane * BPL + j];
        local += h[j];
    }
    unsigned v = local;  // inclusive prefix inside the lane's 16-lane row
    v += dpp<0x111>(v);
    v += dpp<0x112>(v);
    v += dpp<0x114>(v);
    v += dpp<0x118>(v);
    const unsigned t0 = rl(v, 15), t1 = t0 + rl(v, 31), t2 = t1 + rl(v, 47);
    const int row = ta < t0 ? 0 : ta < t1 ? 1 : ta < t2 ? 2 : 3;
    const unsigned rbase = row == 0 ? 0u : row == 1 ? t0 : row == 2 ? t1 : t2;
    const uint64_t before = __ballot(v <= ta - rbase) & (0xFFFFull << (16 * row));
    const int La = min(16 * row + (int)__popcll(before), 63);
    unsigned hs[BPL], loc = 0;
#pragma unroll
    for (int j = 0; j < BPL; ++j) {
        hs[j] = rl(h[j], La);
        loc += hs[j];
    }
    unsigned run = rbase + rl(v, La) - loc;  // elements below lane La's first bin
    ba = (unsigned)(La * BPL + BPL - 1);
    bfa = run;
    ca = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < BPL; ++j) {
        const unsigned nxt = run + hs[j];
        if (!found && nxt > ta) {
            found = true;
            ba = (unsigned)(La * BPL + j);
            bfa = run;
            ca = hs[j];
        }
        run = nxt;
    }
}

// Occupancy target per PL: the samples take PL VGPRs; ask the register allocator for
// enough waves per SIMD that HBM latency is covered by other waves' segments.
template <int PL>
struct Occ {
    static constexpr int W = PL >= 128 ? 3 : PL >= 64 ? 4 : PL >= 32 ? 6 : 8;
};
template <int PL, bool FULL>
struct OccV {  // the masked PL=128 variant gets the whole 256-register budget
    static constexpr int W = (!FULL && PL >= 128) ? 2 : Occ<PL>::W;
};

// cache policy of the once-read sample stream (buffer-load aux bits)
constexpr int LOAD_AUX = 2;  // nt: measured +1.5-2% on C2/C3 over the default policy

// One wave per segment held in registers (v: 64*PL slots, lane-interleaved in 16-B vectors;
// register i of lane L holds slot e = 256 (i >> 2) + 4 L + (i & 3) - m0).  MIN / MAX by wave
// reductions; d = x - MIN in place; exact sums; MED by radix select on d with a wave-private LDS
// histogram, the median's bucket resolved by candidate compaction and rank-by-compare, or by
// the wrapped extremes of two buckets, or by another level.  The masked (!FULL) segments take
// the same body (below).  Per sample:
//   * the exact sum is one 32-bit add when the segment spans < 2^24 ns (64*PL*2^24 < 2^32:
//     no carry chain); wider segments take lane_sums / lane_sums_f64;
//   * the squares are packed f32 (v_pk_add / v_pk_fma on sample pairs: d, c < 2^24 convert
//     exactly, so (float)d - (float)c == (float)(int)(d - c));
//   * when ranks t0, t1 fall in different buckets b0 < b1, s[t0] = max{d < hi(b0)} and
//     s[t1] = min{d >= lo(b1)} come from one wrapped max / min per sample: d - hi (mod 2^32)
//     puts every sample below hi above every sample at or above it, so the wave max of
//     d - hi is the largest sample below hi (likewise the min of d - lo), for any range.
// The wave reductions finish with row_bcast (wave_*_b).
template <int PL>
struct LeanOut {
    // the exact sum of d: an integer for PL <= 16 (the group kernel's epilogue takes it from
    // scalar registers), its (exact) f64 value above
    using Sd = typename std::conditional<(PL <= 16), uint64_t, double>::type;
    unsigned mn, mx, d0, d1, c;  // d0 / d1: the two middle ranks, relative to mn
    Sd sd;
    double sq;
};
// LeanOut::sd through a 64-bit register pair (the group epilogues' lane-held results)
__device__ __forceinline__ uint64_t sd_bits(uint64_t sd) { return sd; }
__device__ __forceinline__ uint64_t sd_bits(double sd) { return (uint64_t)__double_as_longlong(sd); }
template <int PL>
__device__ __forceinline__ double sd_value(uint64_t b) {
    if constexpr (PL <= 16)
        return (double)b;
    else
        return __longlong_as_double((long long)b);
}

// The pivot of the squares is the median of three probes, the samples p[0], p[n / 2] and
// p[n - 1]: a sample, as the masked bodies' padding has to be, and one that a single outlier
// cannot be.  The f32 squares round relative to sigma^2 + (pivot - mean)^2, so a pivot far from
// the bulk costs STD its accuracy; with sample 0 as the pivot a ring whose first call was the
// slow one did that.
__device__ __forceinline__ unsigned median3(unsigned a, unsigned b, unsigned c) {
    return max(min(a, b), min(max(a, b), c));
}

// !FULL: a segment of n < 64 * PL samples starting m0 slots into its first 16-byte vector
// (finish_loads_pivot set every other slot to x0, the pivot, a sample: neutral for MIN / MAX,
// d - c = 0 in the squares).  The pad = 64 * PL - n copies of x0 are taken out again where they
// count: pad * c from the exact sum; -pad as the initial count of the pivot's bin at every
// histogram level whose window holds it; and from the candidates of the pivot's bucket (a
// masked compaction, only when the median's bucket is the pivot's).  The wrapped max / min of
// two buckets need nothing: x0 is a sample, so its copies change neither.
// KB: level-0 bins kept in registers (PL more VGPRs).
template <int PL, bool FULL = true, bool KB = (PL <= 16)>
__device__ __forceinline__ LeanOut<PL> lean_core(unsigned (&v)[PL], int n, int m0, unsigned x0,
                                                 unsigned* hist) {
    using Sd = typename LeanOut<PL>::Sd;
    constexpr int NB = Bins<PL>::NB;
    constexpr int LOGNB = Bins<PL>::LOG;
    constexpr int BPL = Bins<PL>::BPL;
    const int lane = lane_id();
    const unsigned pad = FULL ? 0u : (unsigned)(64 * PL - n);
    const int eb = 4 * lane - m0;  // slot of register i: eb + 256 (i >> 2) + (i & 3)
    const auto real = [&](int i) { return FULL || (unsigned)(eb + 256 * (i >> 2) + (i & 3)) < (unsigned)n; };

    unsigned lmn = v[0], lmx = v[0];
#pragma unroll
    for (int i = 1; i < PL; ++i) {
        lmn = min(lmn, v[i]);
        lmx = max(lmx, v[i]);
    }
    const unsigned mn = wave_min_b(lmn);
    const unsigned mx = wave_max_b(lmx);
    const unsigned range = mx - mn;
    // Segments spanning < 2^23 ns (every configs[] shape) hold x = d + B, B = 0x4B000000 = the
    // f32 bits of 2^23: x is then the bit pattern of the float 2^23 + d, so the squares take
    // the registers as they are (no int -> float conversion per sample).  Selection is
    // translation invariant -- the histogram takes bits [shift, shift + LOGNB) of x (those of
    // d: bits(range) <= 23), the walk starts at wlo = B -- and B leaves the results at the end.
    const unsigned B = range < (1u << 23) ? 0x4B000000u : 0u;
    const unsigned off = B - mn;
#pragma unroll
    for (int i = 0; i < PL; ++i) v[i] += off;

    // ---- exact sum + squares about the pivot c (lane_sums order: pairs, groups of 16) ----
    // FULL: x0 is sample 0 and the other two probes of the pivot (slots 32 PL and 64 PL - 1, see
    // issue_probes) are read here, from registers that already hold d (+ B): taken before MIN is
    // known they would make the wave wait for its last load ahead of the MIN / MAX pass, which
    // otherwise runs while the loads land.  !FULL: x0 is the pivot already (and the padding).
    unsigned cp = x0 - mn;  // the pivot's (and the padding's) d
    if constexpr (FULL) {
        constexpr int EM = 32 * PL;  // slot n / 2: register 4 (EM >> 8) of lane (EM & 255) >> 2
        cp = median3(cp, rl(v[4 * (EM >> 8)], (EM & 255) >> 2) - B, rl(v[PL - 1], 63) - B);
    }
    unsigned c = cp;
    Sd sd;
    double acc;
    if (range < (1u << 24)) {
        constexpr int G = PL < 16 ? PL : 16;
        unsigned ls = 0;
        acc = 0.0;
        if (B) {
            // (2^23 + d) - (2^23 + c): both exact in f32, and so is the difference
            const float fc = __builtin_bit_cast(float, B + c);
            const f32x2 cc = {fc, fc};
#pragma unroll
            for (int g = 0; g < PL; g += G) {
                f32x2 q = {0.0f, 0.0f};
#pragma unroll
                for (int i = 0; i < G; i += 2) {
                    ls += v[g + i];
                    ls += v[g + i + 1];
                    const f32x2 e = (f32x2){__builtin_bit_cast(float, v[g + i]),
                                            __builtin_bit_cast(float, v[g + i + 1])} - cc;
                    q = __builtin_elementwise_fma(e, e, q);
                }
                acc += (double)q.x + (double)q.y;
            }
            ls -= (unsigned)PL * B;  // sum d mod 2^32, exact: PL * 2^23 < 2^32
        } else {
            const f32x2 cc = {(float)c, (float)c};
#pragma unroll
            for (int g = 0; g < PL; g += G) {
                f32x2 q = {0.0f, 0.0f};
#pragma unroll
                for (int i = 0; i < G; i += 2) {
                    ls += v[g + i];
                    ls += v[g + i + 1];
                    const f32x2 e = (f32x2){(float)v[g + i], (float)v[g + i + 1]} - cc;
                    q = __builtin_elementwise_fma(e, e, q);
                }
                acc += (double)q.x + (double)q.y;
            }
        }
        if (PL <= 16) {
            // integer reduction: a row of 16 lanes sums to < 16 * 16 * 2^24 = 2^32 (no
            // u32 wrap), the four row sums combine in 64 bits -- exact, as the f64 sum
            unsigned r = ls;
            r += dpp<0xB1>(r);
            r += dpp<0x4E>(r);
            r += dpp<0x141>(r);
            r += dpp<0x140>(r);
            sd = (Sd)(((uint64_t)rl(r, 0) + rl(r, 16)) + ((uint64_t)rl(r, 32) + rl(r, 48)) -
                      (uint64_t)pad * cp);
        } else {
            sd = (Sd)(wave_sum_f64_b((double)ls) - (double)((uint64_t)pad * cp));  // exact
        }
    } else {  // rare: a ring spanning >= 16.7 ms
        uint64_t sdi;
        if (range < 0x80000000u) {
            lane_sums<PL>(v, c, sdi, acc);
        } else {
            c = 0u;
            lane_sums_f64<PL>(v, sdi, acc);
            if (!FULL) acc -= lane == 0 ? (double)pad * ((double)cp * (double)cp) : 0.0;
        }
        sd = (Sd)(wave_sum_f64_b((double)sdi) - (double)((uint64_t)pad * cp));
    }
    const double sq = wave_sum_f64_b(acc);

    // ---- first histogram level ----
    // KEEPBIN (short segments, registers to spare): every sample's level-0 bin stays in a
    // register, so the level-0 candidate test is one compare instead of a subtract, a shift
    // and a compare
    constexpr bool KEEPBIN = KB;
    unsigned hb[KEEPBIN ? PL : 1];
    const int bits = 32 - __clz((int)range);
    int shift = bits > LOGNB ? bits - LOGNB : 0;
    const unsigned xc = B + cp;  // the padding's value
    // the padding's bin starts at -pad: at level 0 bin ubfe(x, shift, LOGNB) (the window is
    // every value; NB << shift may be 2^32), below it [wlo, wlo + NB << shift) if it holds xc
    const auto clear_bins = [&](unsigned wlo_, int shift_, bool level0) {
        const unsigned q = xc - wlo_;
        const unsigned pb = !(!FULL && pad) ? 0xFFFFFFFFu
                            : level0 ? __builtin_amdgcn_ubfe(xc, (unsigned)shift_, (unsigned)LOGNB)
                            : q < ((unsigned)NB << shift_) ? q >> shift_ : 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < BPL; ++j) hist[lane * BPL + j] = (unsigned)(lane * BPL + j) == pb ? 0u - pad : 0u;
    };
    if (FULL) {
#pragma unroll
        for (int j = 0; j < BPL; ++j) hist[lane * BPL + j] = 0u;
    } else {
        clear_bins(B, shift, true);
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < PL; ++i) {
        const unsigned h = __builtin_amdgcn_ubfe(v[i], (unsigned)shift, (unsigned)LOGNB);  // d >> shift
        if (KEEPBIN) hb[KEEPBIN ? i : 0] = h;
        atomicAdd(&hist[h], 1u);
    }
    __builtin_amdgcn_wave_barrier();

    const unsigned t0 = (unsigned)((n & 1) ? n / 2 : n / 2 - 1);
    const unsigned t1 = (unsigned)(n / 2);
    unsigned wlo = B, below = 0, d0 = 0, d1 = 0;
    // every level narrows the window by LOGNB bits and shift reaches 0 (an exit) by level
    // ceil(32 / LOGNB): the bound only makes that explicit, so no wave can spin here (round 3's
    // gfx950 hang was a loop of this shape with control flow merged into its exits)
    constexpr int LEVELS = (32 + LOGNB - 1) / LOGNB + 1;
#pragma unroll 1
    for (int level = 0; level < LEVELS; ++level) {
        if (level > 0) {
            if (FULL) {
#pragma unroll
                for (int j = 0; j < BPL; ++j) hist[lane * BPL + j] = 0u;
            } else {
                clear_bins(wlo, shift, false);
            }
            __builtin_amdgcn_wave_barrier();
            const unsigned span = (unsigned)NB << shift;
#pragma unroll
            for (int i = 0; i < PL; ++i) {
                const unsigned q = v[i] - wlo;
                if (q < span) atomicAdd(&hist[q >> shift], 1u);
            }
            __builtin_amdgcn_wave_barrier();
        }
        // rank t1 = t0 or t0 + 1: usually in t0's bucket, so locate t0 alone and t1 only
        // when it lies past that bucket (a wave-uniform branch)
        unsigned b0, c0, n0, b1;
        hist_locate1<PL>(hist, t0 - below, b0, c0, n0);
        if (t1 - below < c0 + n0) {
            b1 = b0;
        } else {
            unsigned c1, n1;
            hist_locate1<PL>(hist, t1 - below, b1, c1, n1);
        }
        if (b0 != b1) {
            const unsigned hi0 = wlo + ((b0 + 1) << shift);
            const unsigned lo1 = wlo + (b1 << shift);
            unsigned a = 0u, z = 0xFFFFFFFFu;
#pragma unroll
            for (int i = 0; i < PL; i += 2) {
                a = max(a, max(v[i] - hi0, v[i + 1] - hi0));
                z = min(z, min(v[i] - lo1, v[i + 1] - lo1));
            }
            d0 = wave_max_b(a) + hi0;
            d1 = wave_min_b(z) + lo1;
            break;
        }
        if (shift == 0) {
            d0 = d1 = wlo + b0;
            break;
        }
        if (n0 <= 64u) {
            // compact the <= 64 candidates of bucket b0 into LDS (the histogram is consumed)
            __builtin_amdgcn_wave_barrier();
            unsigned base = 0;
            const unsigned lo0 = wlo + (b0 << shift);
            const unsigned width = 1u << shift;
            const bool masked = !FULL && pad && xc - lo0 < width;  // the padding is in bucket b0
            if (masked) {
#pragma unroll
                for (int i = 0; i < PL; ++i) {
                    const bool in = v[i] - lo0 < width && real(i);
                    const uint64_t bm = __ballot(in);
                    if (in) hist[base + mbcnt(bm)] = v[i];
                    base += (unsigned)__popcll(bm);
                }
            } else if (KEEPBIN && level == 0) {
#pragma unroll
                for (int i = 0; i < PL; ++i) {
                    const bool in = hb[KEEPBIN ? i : 0] == b0;
                    const uint64_t bm = __ballot(in);
                    if (in) hist[base + mbcnt(bm)] = v[i];
                    base += (unsigned)__popcll(bm);
                }
            } else {
#pragma unroll
                for (int i = 0; i < PL; ++i) {
                    const bool in = v[i] - lo0 < width;
                    const uint64_t bm = __ballot(in);
                    if (in) hist[base + mbcnt(bm)] = v[i];
                    base += (unsigned)__popcll(bm);
                }
            }
            __builtin_amdgcn_wave_barrier();
            const unsigned ci = (lane < (int)n0) ? hist[lane] : 0xFFFFFFFFu;
            unsigned rank = 0;
            if (shift <= 26) {
                // unique keys (candidate - lo0, lane) in one word: rank = keys below mine, one
                // compare per candidate; lanes >= n0 hold the maximum and never count
                const unsigned key = (lane < (int)n0) ? ((ci - lo0) << 6) | (unsigned)lane : 0xFFFFFFFFu;
                for (int j = 0; j < (int)n0; j += 4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) rank += (rl(key, j + u) < key) ? 1u : 0u;
                }
            } else {
                for (int j = 0; j < (int)n0; ++j) {
                    const unsigned cj = __builtin_amdgcn_readlane(ci, j);
                    rank += (cj < ci || (cj == ci && j < lane)) ? 1u : 0u;
                }
            }
            const unsigned r0 = t0 - below - c0, r1 = t1 - below - c0;
            const int L0 = __builtin_ffsll(__ballot(lane < (int)n0 && rank == r0)) - 1;
            const int L1 = __builtin_ffsll(__ballot(lane < (int)n0 && rank == r1)) - 1;
            d0 = __builtin_amdgcn_readlane(ci, L0);
            d1 = __builtin_amdgcn_readlane(ci, L1);
            break;
        }
        below += c0;
        wlo += b0 << shift;
        shift = shift > LOGNB ? shift - LOGNB : 0;
    }
    return LeanOut<PL>{mn, mx, d0 - B, d1 - B, c, sd, sq};
}

// HBM -> VGPR in two steps, so a caller can issue the next segment's loads before it
// reduces the current one.  issue_loads: the segment p[0:n) into v (64*PL slots, see
// lean_core) with 16-byte buffer loads from the 16-B aligned base below p; the descriptor
// is built from wave-uniform (readfirstlane'd) inputs so the loads issue back to back (no
// waterfall); lanes past the segment fall outside the descriptor's range (the hardware
// returns 0).  finish_loads (after the loads landed): m0 = p's offset in its 16-B vector
// (in samples), x0 = sample 0 (lane 0's slot m0: no extra memory access); !FULL sets the
// slots outside the segment to x0 (a sample: neutral for MIN/MAX).
template <int PL>
__device__ __forceinline__ void issue_loads(const uint32_t* p, int n, unsigned (&v)[PL]) {
    constexpr int NV = PL / 4;
    const int lane = lane_id();
    const uintptr_t pa = (uintptr_t)p & ~(uintptr_t)15;
    const int m0 = (int)(((uintptr_t)p & 15) >> 2);
    const int nvec = (n + m0 + 3) >> 2;
    const unsigned pa_lo = __builtin_amdgcn_readfirstlane((unsigned)pa);
    const unsigned pa_hi = __builtin_amdgcn_readfirstlane((unsigned)(pa >> 32));
    const int nbytes = __builtin_amdgcn_readfirstlane(nvec * 16);
    void* const pbase = (void*)(((uint64_t)pa_hi << 32) | pa_lo);
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(pbase, 0, nbytes, 0x00020000);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 16, j * 1024, LOAD_AUX);
        v[4 * j + 0] = q.x;
        v[4 * j + 1] = q.y;
        v[4 * j + 2] = q.z;
        v[4 * j + 3] = q.w;
    }
}

template <int PL, bool FULL>
__device__ __forceinline__ void first_sample(const uint32_t* p, const unsigned (&v)[PL], int& m0,
                                             unsigned& x0) {
    m0 = FULL ? 0 : (int)(((uintptr_t)p & 15) >> 2);
    const unsigned e0 = m0 == 0 ? v[0] : m0 == 1 ? v[1] : m0 == 2 ? v[2] : v[3];
    x0 = __builtin_amdgcn_readlane(e0, 0);
}
// the slots outside the segment take x (a sample)
template <int PL, bool FULL>
__device__ __forceinline__ void fill_outside(int n, unsigned (&v)[PL], int m0, unsigned x) {
    const int lane = lane_id();
    // a masked-class segment that happens to fill the wave exactly (configs[3]: every ring at
    // cap = 8192) needs no masking (wave-uniform test)
    if (!FULL && (n != 64 * PL || m0 != 0)) {
#pragma unroll
        for (int i = 0; i < PL; ++i) {
            const unsigned e = (unsigned)(((i >> 2) * 64 + lane) * 4 + (i & 3) - m0);
            v[i] = (e < (unsigned)n) ? v[i] : x;
        }
    }
}

template <int PL, bool FULL>
__device__ __forceinline__ void finish_loads(const uint32_t* p, int n, unsigned (&v)[PL], int& m0,
                                             unsigned& x0) {
    first_sample<PL, FULL>(p, v, m0, x0);
    fill_outside<PL, FULL>(n, v, m0, x0);
}

template <int PL, bool FULL>
__device__ __forceinline__ void load_segment(const uint32_t* p, int n, unsigned (&v)[PL], int& m0,
                                             unsigned& x0) {
    issue_loads<PL>(p, n, v);
    finish_loads<PL, FULL>(p, n, v, m0, x0);
}

// The masked bodies' pivot (lean_core's x0 there: the centre of the f32 squares and the padding
// value): the median of the three probes p[0], p[n / 2], p[n - 1] (lean_core, above).  Lane 0 /
// the other lanes load p[n / 2] / p[n - 1] with one more vector load issued behind the segment's
// own, so it lands with them (n >= 1: both inside the segment); the unmasked bodies find the
// probes in known registers (lean_core) and load nothing more.
__device__ __forceinline__ unsigned issue_probes(const uint32_t* p, int n) {
    return p[lane_id() == 0 ? n >> 1 : n - 1];
}
template <int PL>
__device__ __forceinline__ void finish_loads_pivot(const uint32_t* p, int n, unsigned (&v)[PL],
                                                   unsigned probes, int& m0, unsigned& x0) {
    first_sample<PL, false>(p, v, m0, x0);
    x0 = median3(x0, __builtin_amdgcn_readlane(probes, 0), __builtin_amdgcn_readlane(probes, 1));
    fill_outside<PL, false>(n, v, m0, x0);
}
template <int PL>
__device__ __forceinline__ void load_segment_pivot(const uint32_t* p, int n, unsigned (&v)[PL],
                                                   int& m0, unsigned& x0) {
    issue_loads<PL>(p, n, v);
    const unsigned probes = issue_probes(p, n);
    finish_loads_pivot<PL>(p, n, v, probes, m0, x0);
}

}  // namespace nvrx
