// segment_quantiles.hip -- per-kernel duration quantiles (tail order statistics) on gfx950.
//
// No reference counterpart: computeStats (CuptiProfiler.cpp:44-74) keeps MIN / MAX / MED only.
// A quantile is asked for as an integer permille pm in [0, 1000]; for a segment of n >= 1
// retained samples the answer is the order statistic of 0-based rank
//     k = (pm * (n - 1)) / 1000        (integer division, 64-bit)
// over the duration keys sorted ascending, converted like every other sample (ns_to_us): always
// one of the samples, never an interpolation, so pm = 0 has MIN's bits, pm = 1000 MAX's and
// pm = 500 of an odd n MED's.  Up to NVRX_MAX_QUANTILES ranks per segment come out of one launch
// (the permilles travel by value in the kernel arguments); out is quantile-major [nq][nseg].
//
// Register path (retained length + misalignment <= 8192), one wave per segment: the samples
// are loaded once with load_segment (segment_wave.h: the PL ladder, 16-byte buffer loads) and
// selected MSB-first on d = x - MIN with a wave-private LDS histogram of Bins<PL>::NB bins.  The
// state of rank q (its window [lo, lo + 2^sh), the count below it, the count inside it) lives in
// lane q; ranks whose windows coincide form a group that is resolved once:
//     sh == 0             the window is one value: done;
//     <= 64 samples       compacted into LDS and ranked by compare, every rank of the group read off;
//     otherwise           one more histogram level over the window, every rank of the group located.
// The first level's window is the whole range, so its histogram serves every rank.
//
// Streaming path (longer segments, up to NVRX_MAX_SEGMENT), one 1024-thread workgroup per
// segment: four passes over the segment in memory, an 8-bit digit of the key per pass from the
// top; every rank advances in each pass, ranks with equal prefixes share one of the nq x 256 LDS
// bins' histograms.  No scratch, no allocation.
//
// Every launch covers all segments; a segment is taken by the one kernel whose class holds its own
// retained length (plus its offset in the first 16-byte vector).  seg_len < 0: untouched; empty:
// NaN and num 0 (as nvrx_segment_stats_ragged).  Segments of a few samples still take a whole wave
// (a lane-per-segment class is not built).

#include "segment_wave.h"

namespace nvrx {
namespace {

struct QuantArgs {
    int32_t pm[NVRX_MAX_QUANTILES];
    int32_t nq;
};

// a.pm[lane] for lane < NVRX_MAX_QUANTILES without a runtime-indexed array
__device__ __forceinline__ unsigned pm_of(const QuantArgs& a, int lane) {
    int r = a.pm[0];
#pragma unroll
    for (int j = 1; j < NVRX_MAX_QUANTILES; ++j) r = lane == j ? a.pm[j] : r;
    return (unsigned)r;
}

// One read of a wave's histogram (lane L: bins [L * BPL, (L + 1) * BPL)) and its inclusive
// prefix over the lanes; hist_find then locates any number of ranks without touching LDS again.
template <int BPL>
struct HistScan {
    unsigned h[BPL], local, incl;
    __device__ __forceinline__ void read(const unsigned* hist) {
        const int lane = lane_id();
        local = 0;
#pragma unroll
        for (int j = 0; j < BPL; ++j) {
            h[j] = hist[lane * BPL + j];
            local += h[j];
        }
        incl = wave_incl_scan_u32(local);
    }
    // the bin holding relative rank ta (wave-uniform, below the histogram's total): its index,
    // the elements in lower bins, its count
    __device__ __forceinline__ void find(unsigned ta, unsigned& b, unsigned& below, unsigned& cnt) const {
        const int La = min((int)__popcll(__ballot(incl <= ta)), 63);
        unsigned run = rl(incl, La) - rl(local, La);
        b = (unsigned)(La * BPL + BPL - 1);
        below = run;
        cnt = 0;
        bool found = false;
#pragma unroll
        for (int j = 0; j < BPL; ++j) {
            const unsigned hs = rl(h[j], La);
            const unsigned nxt = run + hs;
            if (!found && nxt > ta) {
                found = true;
                b = (unsigned)(La * BPL + j);
                below = run;
                cnt = hs;
            }
            run = nxt;
        }
    }
};

constexpr int QCAND = 64;  // candidates a group ranks by compare (one per lane)

// The selection of the register path.  v: the segment as load_segment<PL, false> left it (slots
// outside the segment hold x0, sample 0); tq: this lane's rank (lanes < nq).  Returns MIN in mn
// and, in lane q < nq, the key of rank q minus MIN.  The pad = 64 * PL - n copies of x0 are
// taken out where they count, as lean_core does: -pad as the initial count of x0's bin at every
// histogram level whose window holds it, and a masked compaction of a window that holds it.
template <int PL>
__device__ __forceinline__ unsigned quant_core(unsigned (&v)[PL], int n, int m0, unsigned x0,
                                               unsigned* hist, unsigned* cand, unsigned tq, int nq,
                                               unsigned& mn_out) {
    constexpr int NB = Bins<PL>::NB;
    constexpr int LOG = Bins<PL>::LOG;
    constexpr int BPL = Bins<PL>::BPL;
    const int lane = lane_id();
    const unsigned pad = (unsigned)(64 * PL - n);
    const int eb = 4 * lane - m0;  // slot of register i: eb + 256 (i >> 2) + (i & 3)
    const auto real = [&](int i) { return (unsigned)(eb + 256 * (i >> 2) + (i & 3)) < (unsigned)n; };

    unsigned lmn = v[0], lmx = v[0];
#pragma unroll
    for (int i = 1; i < PL; ++i) {
        lmn = min(lmn, v[i]);
        lmx = max(lmx, v[i]);
    }
    const unsigned mn = wave_min_b(lmn);
    const unsigned mx = wave_max_b(lmx);
#pragma unroll
    for (int i = 0; i < PL; ++i) v[i] -= mn;
    const unsigned cp = x0 - mn;  // the padding's d
    const int bits = 32 - __clz((int)(mx - mn));
    mn_out = mn;

    // rank q's window and counts, in lane q
    unsigned s_lo = 0u, s_sh = (unsigned)bits, s_below = 0u, s_cnt = (unsigned)n, res = 0u;
    unsigned todo = (1u << nq) - 1u;  // wave-uniform: ranks not resolved yet
    // every visit resolves a group or narrows its window by LOG bits (sh reaches 0, an exit, after
    // ceil(32 / LOG) <= 6 levels): at most 7 visits per rank.  The bound makes that explicit, so
    // no wave can spin here.
    constexpr int MAXIT = 7 * NVRX_MAX_QUANTILES;
#pragma unroll 1
    for (int it = 0; it < MAXIT && todo; ++it) {
        const int q = __builtin_ffs((int)todo) - 1;
        const unsigned lo = rl(s_lo, q), below = rl(s_below, q), cnt = rl(s_cnt, q);
        const int sh = (int)rl(s_sh, q);
        // the ranks sharing q's window (equal lo and sh: the same window, so the same counts)
        const unsigned grp = (unsigned)__ballot(lane < nq && s_lo == lo && s_sh == (unsigned)sh) & todo;
        if (sh == 0) {  // one value
            if (lane < NVRX_MAX_QUANTILES && ((grp >> lane) & 1u)) res = lo;
            todo &= ~grp;
            continue;
        }
        const unsigned wm1 = sh >= 32 ? 0xFFFFFFFFu : (1u << sh) - 1u;  // d in window: d - lo <= wm1
        const bool padin = pad != 0u && cp - lo <= wm1;                // the padding is in the window
        if (cnt <= (unsigned)QCAND) {
            // compact the window's samples into LDS (a wave-uniform branch skips the registers
            // that hold none), rank them by compare, read every rank of the group off
            unsigned base = 0;
            if (padin) {
#pragma unroll
                for (int i = 0; i < PL; ++i) {
                    const bool in = v[i] - lo <= wm1 && real(i);
                    const uint64_t bm = __ballot(in);
                    if (bm) {
                        const unsigned idx = base + mbcnt(bm);
                        if (in && idx < (unsigned)QCAND) cand[idx] = v[i];
                        base += (unsigned)__popcll(bm);
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < PL; ++i) {
                    const bool in = v[i] - lo <= wm1;
                    const uint64_t bm = __ballot(in);
                    if (bm) {
                        const unsigned idx = base + mbcnt(bm);
                        if (in && idx < (unsigned)QCAND) cand[idx] = v[i];
                        base += (unsigned)__popcll(bm);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            const unsigned ci = (lane < (int)cnt) ? cand[lane] : 0xFFFFFFFFu;
            unsigned rank = 0;
            if (sh <= 26) {
                // unique keys (candidate - lo, lane) in one word: rank = keys below mine; lanes
                // >= cnt hold the maximum and never count
                const unsigned key = (lane < (int)cnt) ? ((ci - lo) << 6) | (unsigned)lane : 0xFFFFFFFFu;
                for (int j = 0; j < (int)cnt; j += 4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) rank += (rl(key, (j + u) & 63) < key) ? 1u : 0u;
                }
            } else {
                for (int j = 0; j < (int)cnt; ++j) {
                    const unsigned cj = rl(ci, j);
                    rank += (cj < ci || (cj == ci && j < lane)) ? 1u : 0u;
                }
            }
            for (unsigned g = grp; g; g &= g - 1u) {
                const int q2 = __builtin_ffs((int)g) - 1;
                const unsigned r = rl(tq, q2) - below;
                const int L = (__builtin_ffsll((long long)__ballot(lane < (int)cnt && rank == r)) - 1) & 63;
                const unsigned val = rl(ci, L);
                if (lane == q2) res = val;
            }
            todo &= ~grp;
            __builtin_amdgcn_wave_barrier();  // cand is rewritten by the next group
            continue;
        }
        // one more histogram level over the window: bin (d - lo) >> s2
        const int s2 = sh > LOG ? sh - LOG : 0;
        const unsigned pb = padin ? (cp - lo) >> s2 : 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < BPL; ++j) hist[lane * BPL + j] = (unsigned)(lane * BPL + j) == pb ? 0u - pad : 0u;
        __builtin_amdgcn_wave_barrier();
        if (sh == bits) {  // the first level: the window is the whole range, shared by every rank
#pragma unroll
            for (int i = 0; i < PL; ++i) atomicAdd(&hist[v[i] >> s2], 1u);
        } else {
#pragma unroll
            for (int i = 0; i < PL; ++i) {
                const unsigned d = v[i] - lo;
                if (d <= wm1) atomicAdd(&hist[d >> s2], 1u);
            }
        }
        __builtin_amdgcn_wave_barrier();
        HistScan<BPL> hs;
        hs.read(hist);
        for (unsigned g = grp; g; g &= g - 1u) {
            const int q2 = __builtin_ffs((int)g) - 1;
            unsigned b, bl, c;
            hs.find(rl(tq, q2) - below, b, bl, c);
            if (lane == q2) {
                s_lo = lo + (b << s2);
                s_sh = (unsigned)s2;
                s_below = below + bl;
                s_cnt = c;
            }
        }
        __builtin_amdgcn_wave_barrier();  // the bins are cleared by the next level
    }
    static_assert(NB >= 64 && (1 << LOG) == NB, "bins");
    return res;
}

constexpr int QUANT_WAVE_MAX = 64 * 128;  // the longest need of the register path

// Register path, class PL: segments of 32 * PL < need <= 64 * PL (PL = 4: every need <= 256,
// the empty segments among them).
template <int PL, class Segs>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Occ<PL>::W)))
void seg_quantiles_wave_kernel(Segs segs, int64_t nseg, QuantArgs qa, float* out, int32_t* num) {
    constexpr int WL = Bins<PL>::NB + QCAND;  // LDS words per wave: histogram, candidates
    __shared__ __attribute__((aligned(16))) unsigned lds[4 * WL];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t s = (int64_t)blockIdx.x * 4 + wave;
    if (s >= nseg) return;  // wave-uniform; the kernel has no workgroup barrier
    const uint32_t* p;
    int n;
    segs.get(s, p, n);
    if (n < 0) return;  // skipped: outputs untouched
    const int need = seg_need(p, n);
    if (need > 64 * PL || (PL > 4 && need <= 32 * PL)) return;  // another class's segment
    const int nq = qa.nq;
    if (n == 0) {
        if (lane < nq) out[(int64_t)lane * nseg + s] = __builtin_nanf("");
        if (lane == 0 && num) num[s] = 0;
        return;
    }
    unsigned* hist = lds + wave * WL;
    unsigned v[PL];
    int m0;
    unsigned x0;
    load_segment<PL, false>(p, n, v, m0, x0);
    // n <= 8192 and pm <= 1000: the product fits 32 bits
    const unsigned tq = lane < nq ? (pm_of(qa, lane) * (unsigned)(n - 1)) / 1000u : 0u;
    unsigned mn;
    const unsigned res = quant_core<PL>(v, n, m0, x0, hist, hist + Bins<PL>::NB, tq, nq, mn);
    if (lane < nq) out[(int64_t)lane * nseg + s] = ns_to_us(mn + res);
    if (lane == 0 && num) num[s] = n;
}

// Streaming path: need > QUANT_WAVE_MAX.  Pass j takes bits [24 - 8j, 32 - 8j) of the keys whose
// higher bits equal a rank's prefix; after four passes a rank's prefix is its key.  Ranks with
// equal prefixes share a histogram (s_h: rank -> histogram, s_pf: histogram -> prefix).
constexpr int QS_THREADS = 1024;
template <class Segs>
__global__ __launch_bounds__(QS_THREADS)
void seg_quantiles_stream_kernel(Segs segs, int64_t nseg, QuantArgs qa, float* out, int32_t* num) {
    constexpr int NQ = NVRX_MAX_QUANTILES;
    __shared__ unsigned bins[NQ * 256];
    __shared__ unsigned s_pf[NQ], s_key[NQ], s_t[NQ], s_h[NQ], s_nh;
    const int64_t s = blockIdx.x;
    if (s >= nseg) return;
    const uint32_t* p;
    int n;
    segs.get(s, p, n);
    if (n <= 0 || seg_need(p, n) <= QUANT_WAVE_MAX) return;  // block-uniform
    const int tid = threadIdx.x, lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nq = qa.nq;
    if (tid < NQ) {
        s_t[tid] = tid < nq ? (unsigned)(((uint64_t)pm_of(qa, tid) * (uint64_t)(n - 1)) / 1000u) : 0u;
        s_key[tid] = 0u;
        s_h[tid] = 0u;
        s_pf[tid] = tid == 0 ? 0u : 0xFFFFFFFFu;  // no key's high bits: never matched
        if (tid == 0) s_nh = 1u;
    }
    // the segment as scalar head (up to the first 16-byte boundary), 16-byte vectors, scalar tail
    const int head = min((int)((0u - (unsigned)(((uintptr_t)p & 15) >> 2)) & 3u), n);
    const int nv = (n - head) >> 2;
    const int tail0 = head + 4 * nv;
    const u32x4* pv = (const u32x4*)(p + head);
    __syncthreads();
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        unsigned pf[NQ];
#pragma unroll
        for (int l = 0; l < NQ; ++l) pf[l] = s_pf[l];
        const int nh = (int)s_nh;
        for (int i = tid; i < NQ * 256; i += QS_THREADS) bins[i] = 0u;
        __syncthreads();
        const auto add = [&](unsigned x) {
            const unsigned hi = pass == 0 ? 0u : x >> ((shift + 8) & 31);
            const unsigned dg = (x >> shift) & 255u;
#pragma unroll
            for (int l = 0; l < NQ; ++l)
                if (l < nh && hi == pf[l]) atomicAdd(&bins[l * 256 + (int)dg], 1u);
        };
        if (tid < head) add(p[tid]);
        for (int j = tid; j < nv; j += QS_THREADS) {
            const u32x4 x = pv[j];
            add(x.x);
            add(x.y);
            add(x.z);
            add(x.w);
        }
        if (tail0 + tid < n) add(p[tail0 + tid]);  // fewer than 4 samples
        __syncthreads();
        if (wave < nq) {  // wave q locates rank q in its prefix's histogram
            HistScan<4> hs;
            hs.read(bins + s_h[wave] * 256);
            unsigned b, bl, c;
            const unsigned ta = __builtin_amdgcn_readfirstlane(s_t[wave]);
            hs.find(ta, b, bl, c);
            if (lane == 0) {
                s_t[wave] = ta - bl;
                s_key[wave] = (s_key[wave] << 8) | b;
            }
        }
        __syncthreads();
        if (tid == 0 && pass < 3) {  // histograms of the next pass: one per distinct prefix
            unsigned m = 0;
            for (int q = 0; q < nq; ++q) {
                unsigned f = m;
                for (unsigned l = 0; l < m; ++l)
                    if (s_pf[l] == s_key[q]) f = min(f, l);
                if (f == m) s_pf[m++] = s_key[q];
                s_h[q] = f;
            }
            s_nh = m;
        }
        __syncthreads();
    }
    if (tid < nq) out[(int64_t)tid * nseg + s] = ns_to_us(s_key[tid]);
    if (tid == 0 && num) num[s] = n;
}

template <int PL, class Segs>
void launch_wave_class(const Segs& segs, int64_t nseg, int64_t need_lo, int64_t need_hi,
                       const QuantArgs& qa, float* out, int32_t* num, hipStream_t st) {
    // the class holds needs in (32 * PL, 64 * PL], from 0 for PL = 4
    if (need_lo > 64 * PL || (PL > 4 && need_hi <= 32 * PL)) return;
    hipLaunchKernelGGL((seg_quantiles_wave_kernel<PL, Segs>), dim3((unsigned)((nseg + 3) / 4)), dim3(256),
                       0, st, segs, nseg, qa, out, num);
}

// every class that a need in [need_lo, need_hi] can fall in, each over all segments
template <class Segs>
hipError_t launch_quantiles(const Segs& segs, int64_t nseg, int64_t need_lo, int64_t need_hi,
                            const int32_t* permille, int nq, float* out, int32_t* num, hipStream_t st) {
    QuantArgs qa{};
    qa.nq = nq;
    for (int j = 0; j < nq; ++j) qa.pm[j] = permille[j];
    launch_wave_class<4>(segs, nseg, need_lo, need_hi, qa, out, num, st);
    launch_wave_class<8>(segs, nseg, need_lo, need_hi, qa, out, num, st);
    launch_wave_class<16>(segs, nseg, need_lo, need_hi, qa, out, num, st);
    launch_wave_class<32>(segs, nseg, need_lo, need_hi, qa, out, num, st);
    launch_wave_class<64>(segs, nseg, need_lo, need_hi, qa, out, num, st);
    launch_wave_class<128>(segs, nseg, need_lo, need_hi, qa, out, num, st);
    if (need_hi > QUANT_WAVE_MAX)
        hipLaunchKernelGGL((seg_quantiles_stream_kernel<Segs>), dim3((unsigned)nseg), dim3(QS_THREADS), 0, st,
                           segs, nseg, qa, out, num);
    return hipGetLastError();
}

}  // namespace

// Shape checks happen in abi.cpp (check_strided / check_ragged) before these run.
hipError_t segment_quantiles_strided(const uint32_t* ns, int64_t nseg, int64_t seg_stride,
                                     int64_t seg_begin, int64_t seg_len, int64_t cap,
                                     const int32_t* permille, int nq, float* out, int32_t* num,
                                     hipStream_t st) {
    if (nseg <= 0) return hipSuccess;
    StridedSegs segs{ns, seg_stride, seg_begin, seg_len, cap};
    const SegRange r = seg_range(segs);
    return launch_quantiles(segs, nseg, r.need_lo, r.need_hi, permille, nq, out, num, st);
}

hipError_t segment_quantiles_ragged(const uint32_t* ns, const int64_t* seg_off, const int32_t* seg_len,
                                    int64_t nseg, int64_t max_len, int64_t cap, bool aligned16,
                                    const int32_t* permille, int nq, float* out, int32_t* num,
                                    hipStream_t st) {
    if (nseg <= 0) return hipSuccess;
    RaggedSegs segs{ns, seg_off, seg_len, cap};
    const SegRange r = seg_range(segs, max_len, aligned16);
    return launch_quantiles(segs, nseg, r.need_lo, r.need_hi, permille, nq, out, num, st);
}

}  // namespace nvrx
