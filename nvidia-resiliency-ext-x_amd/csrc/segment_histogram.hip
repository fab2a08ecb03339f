// segment_histogram.hip -- per-kernel duration histograms with fixed buckets, on gfx950.
//
// No reference counterpart (computeStats keeps five numbers per kernel).  The buckets are the
// same for every segment, rank and report, so counts add: over ranks to a fleet-wide
// distribution, over reports to a whole run's.  Log-linear over the u32 duration key x with 3
// mantissa bits, NVRX_HIST_BINS = 240 buckets, each at most 12.5 % wide:
//     bucket(x) = x                                 x < 8
//               = 8 (e - 2) + ((x >> (e - 3)) & 7)  otherwise, e = 31 - clz(x)   (3..31)
//     edge(b)   = b                                 b < 8          (lower edge, a key)
//               = (8 + b % 8) << (b / 8 - 1)        otherwise;     edge(240) := 2^32
//   * bucket is monotone in the key, hence in the duration;
//   * edge(bucket(x)) <= x < edge(bucket(x) + 1);
//   * edge(238) == NVRX_KEY_WIDE: buckets 238 and 239 hold exactly the wide keys (durations of
//     3.76 s and more), every bucket below holds plain nanoseconds;
//   * an edge in us is its key converted like every sample (key_to_f32(edge) / 1000.0f).
// With sh = 28 - clz(x | 8) (0 for x < 16) both branches are bucket(x) = 8 sh + (x >> sh).
//
// A segment is read exactly once, whatever its length, in 16-byte nt vectors from the 16-byte
// boundary at or below its first retained sample; slots of the first and last vector outside
// the retained run count into a spare bin past the 240 (no branch per sample).
//   wave kernel    retained length + offset in the first vector <= HIST_WAVE_MAX: one wave per
//                  segment, a wave-private LDS histogram, 4 vectors per lane per trip, the next
//                  trip's loads issued before the current one is counted;
//   block kernel   longer segments (up to NVRX_MAX_SEGMENT): one 1024-thread workgroup per
//                  segment, a private LDS histogram per wave, combined once at the end.
// Every launch covers all segments; a segment is taken by the kernel whose class holds it.
// Every loop is bounded by the segment's length.
//
// Counting.  A real kernel's durations fall in one to three buckets, so a plain LDS add per lane
// puts most of a wave on one address.  The wave therefore keeps two buckets and their counts in
// scalar registers: per register of 64 samples one ballot per kept bucket and a population count;
// only the lanes matching neither bucket add to LDS, and when 16 or more of them miss, the kept
// bucket with fewer hits is flushed and replaced by a missing lane's bucket.  Clustered input
// costs no LDS traffic at all, spread input one LDS add per lane as the plain scheme plus the
// scalar bookkeeping.  Measured on configs[1]'s shape against the statistics kernel (0.654 ms):
// plain LDS adds 2.688 ms clustered / 0.683 ms spread, this scheme 0.782 / 0.967 ms.
//
// counts is segment-major [nseg][240] u32 (960 B per segment, 16-byte stores by the segment's one
// owner: no global atomics).  accumulate == 0 writes all 240 bins of every segment taken (no
// memset needed), otherwise the counts are added to what is there.  seg_len < 0: untouched;
// empty: zero bins (nothing added) and num 0.  Segments of a few samples still take a whole wave.

#include "histogram_wave.h"
#include "segment_wave.h"

namespace nvrx {
namespace {

constexpr int HW = 256;                  // LDS words per wave: 240 bins, the spare bin, padding
constexpr unsigned SPARE = HB;           // where slots outside the segment count
constexpr unsigned SPARE2 = HB + 1;      // a bucket no slot ever has
constexpr int HIST_WAVE_MAX = 16384;     // the longest need (length + offset) of the wave kernel
constexpr int HIST_REPLACE = 16;         // misses in one register that replace a kept bucket
static_assert(HB % 4 == 0 && HB + 2 <= HW, "bins");

// the two buckets a wave keeps in scalar registers, with their counts
struct Kept {
    unsigned b0 = SPARE, c0 = 0, b1 = SPARE2, c1 = 0;  // b0 != b1 always
};

// one register: bucket b per lane (SPARE for a slot outside the segment)
__device__ __forceinline__ void count_reg(unsigned b, unsigned* h, Kept& k) {
    const uint64_t m0 = __ballot(b == k.b0), m1 = __ballot(b == k.b1);
    const unsigned p0 = (unsigned)__popcll(m0), p1 = (unsigned)__popcll(m1);
    k.c0 += p0;
    k.c1 += p1;
    const uint64_t rest = ~(m0 | m1);
    if (rest) {  // wave-uniform
        if (b != k.b0 && b != k.b1) atomicAdd(&h[b], 1u);
        if (__popcll(rest) >= HIST_REPLACE) {
            // (the missing lanes have been counted above; the new bucket starts at 0)
            const unsigned nb = rl(b, __builtin_ffsll((long long)rest) - 1);
            if (p0 <= p1) {
                if (k.c0 && lane_id() == 0) atomicAdd(&h[k.b0], k.c0);
                k.b0 = nb;
                k.c0 = 0;
            } else {
                if (k.c1 && lane_id() == 0) atomicAdd(&h[k.b1], k.c1);
                k.b1 = nb;
                k.c1 = 0;
            }
        }
    }
}

// one 16-byte vector per lane; e0: the segment slot of q.x (negative or >= n outside the run)
template <bool MASK>
__device__ __forceinline__ void count_vec(const u32x4& q, int e0, int n, unsigned* h, Kept& k) {
    unsigned b[4] = {bucket_of(q.x), bucket_of(q.y), bucket_of(q.z), bucket_of(q.w)};
    if (MASK) {
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = (unsigned)(e0 + c) < (unsigned)n ? b[c] : SPARE;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) count_reg(b[c], h, k);
}

__device__ __forceinline__ void flush_kept(unsigned* h, const Kept& k) {
    if (lane_id() == 0) {
        if (k.c0) atomicAdd(&h[k.b0], k.c0);
        if (k.c1) atomicAdd(&h[k.b1], k.c1);
    }
}

__device__ __forceinline__ void clear_hist(unsigned* h) {
    *(u32x4*)(h + 4 * lane_id()) = (u32x4){0u, 0u, 0u, 0u};
}

// bins [4 t, 4 t + 4) of segment s, t < HB / 4
__device__ __forceinline__ void store_bins(uint32_t* counts, int64_t s, int t, u32x4 c, int accumulate) {
    u32x4* o = (u32x4*)(counts + s * HB) + t;
    if (accumulate) c += *o;
    *o = c;
}

constexpr int WV = 4;  // vectors per lane per trip

template <class Segs>
__global__ __launch_bounds__(256)
void seg_histogram_wave_kernel(Segs segs, int64_t nseg, int accumulate, uint32_t* counts, int32_t* num) {
    __shared__ __attribute__((aligned(16))) unsigned lds[4 * HW];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t s = (int64_t)blockIdx.x * 4 + wave;
    if (s >= nseg) return;  // wave-uniform; the kernel has no workgroup barrier
    const uint32_t* p;
    int n;
    segs.get(s, p, n);
    if (n < 0 || seg_need(p, n) > HIST_WAVE_MAX) return;  // skipped, or the block kernel's
    unsigned* h = lds + wave * HW;
    clear_hist(h);
    __builtin_amdgcn_wave_barrier();
    if (n > 0) {
        // the descriptor of issue_loads (segment_wave.h): lanes past the last vector read 0
        const uintptr_t pa = (uintptr_t)p & ~(uintptr_t)15;
        const int m0 = (int)(((uintptr_t)p & 15) >> 2);
        const int nvec = (n + m0 + 3) >> 2;
        const unsigned pa_lo = __builtin_amdgcn_readfirstlane((unsigned)pa);
        const unsigned pa_hi = __builtin_amdgcn_readfirstlane((unsigned)(pa >> 32));
        const int nbytes = __builtin_amdgcn_readfirstlane(nvec * 16);
        void* const pbase = (void*)(((uint64_t)pa_hi << 32) | pa_lo);
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(pbase, 0, nbytes, 0x00020000);
        const int trips = __builtin_amdgcn_readfirstlane((nvec + 64 * WV - 1) / (64 * WV));
        const auto load = [&](u32x4 (&q)[WV], int trip) {
#pragma unroll
            for (int u = 0; u < WV; ++u)
                q[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 16, (trip * WV + u) * 1024, LOAD_AUX);
        };
        Kept k;
        u32x4 cur[WV], nxt[WV];
        load(cur, 0);
#pragma unroll 1
        for (int trip = 0; trip < trips; ++trip) {
            if (trip + 1 < trips) load(nxt, trip + 1);
            const int e0 = (trip * WV * 64 + lane) * 4 - m0;  // slot of cur[0].x; cur[u]: + 256 u
            // a trip whose 256 WV slots all lie inside the run needs no mask (wave-uniform)
            const int t0 = trip * WV * 256 - m0;
            if (t0 >= 0 && t0 + WV * 256 <= n) {
#pragma unroll
                for (int u = 0; u < WV; ++u) count_vec<false>(cur[u], e0 + 256 * u, n, h, k);
            } else {
#pragma unroll
                for (int u = 0; u < WV; ++u) count_vec<true>(cur[u], e0 + 256 * u, n, h, k);
            }
#pragma unroll
            for (int u = 0; u < WV; ++u) cur[u] = nxt[u];
        }
        flush_kept(h, k);
        __builtin_amdgcn_wave_barrier();
    }
    if (lane < HB / 4) store_bins(counts, s, lane, *(const u32x4*)(h + 4 * lane), accumulate);
    if (lane == 0 && num) num[s] = n;
}

constexpr int HS_THREADS = 1024;
constexpr int HS_WAVES = HS_THREADS / 64;

template <class Segs>
__global__ __launch_bounds__(HS_THREADS)
void seg_histogram_block_kernel(Segs segs, int64_t nseg, int accumulate, uint32_t* counts, int32_t* num) {
    __shared__ __attribute__((aligned(16))) unsigned lds[HS_WAVES * HW];
    const int64_t s = blockIdx.x;
    if (s >= nseg) return;
    const uint32_t* p;
    int n;
    segs.get(s, p, n);
    if (n <= 0 || seg_need(p, n) <= HIST_WAVE_MAX) return;  // block-uniform
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned* h = lds + wave * HW;
    clear_hist(h);
    __builtin_amdgcn_wave_barrier();
    const int m0 = (int)(((uintptr_t)p & 15) >> 2);
    const u32x4* pv = (const u32x4*)(p - m0);  // the 16-byte boundary at or below p
    const int nvec = (int)(((int64_t)n + m0 + 3) >> 2);  // <= 2^28 + 1
    constexpr int TV = HS_THREADS * WV;                  // vectors per trip
    const int trips = (nvec + TV - 1) / TV;
    // past the last vector a lane re-reads it; its slots are then >= n and count into the spare bin
    const auto load = [&](u32x4 (&q)[WV], int trip) {
#pragma unroll
        for (int u = 0; u < WV; ++u)
            q[u] = __builtin_nontemporal_load(pv + min(trip * TV + u * HS_THREADS + tid, nvec - 1));
    };
    Kept k;
    u32x4 cur[WV], nxt[WV];
    load(cur, 0);
#pragma unroll 1
    for (int trip = 0; trip < trips; ++trip) {
        if (trip + 1 < trips) load(nxt, trip + 1);
        const int64_t t0 = (int64_t)trip * TV * 4 - m0;  // first slot of the trip
        const int e0 = (int)(t0 + 4 * tid);              // < 2^30 + 2^14: an int
        if (t0 >= 0 && t0 + TV * 4 <= n) {
#pragma unroll
            for (int u = 0; u < WV; ++u) count_vec<false>(cur[u], e0 + 4 * HS_THREADS * u, n, h, k);
        } else {
#pragma unroll
            for (int u = 0; u < WV; ++u) count_vec<true>(cur[u], e0 + 4 * HS_THREADS * u, n, h, k);
        }
#pragma unroll
        for (int u = 0; u < WV; ++u) cur[u] = nxt[u];
    }
    flush_kept(h, k);
    __syncthreads();
    if (tid < HB / 4) {
        u32x4 c = *(const u32x4*)(lds + 4 * tid);
#pragma unroll
        for (int w = 1; w < HS_WAVES; ++w) c += *(const u32x4*)(lds + w * HW + 4 * tid);
        store_bins(counts, s, tid, c, accumulate);
    }
    if (tid == 0 && num) num[s] = n;
}

// need_hi: the largest need any segment can have
template <class Segs>
hipError_t launch_histogram(const Segs& segs, int64_t nseg, int64_t need_lo, int64_t need_hi,
                            int accumulate, uint32_t* counts, int32_t* num, hipStream_t st) {
    if (need_lo <= HIST_WAVE_MAX)
        hipLaunchKernelGGL((seg_histogram_wave_kernel<Segs>), dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0,
                           st, segs, nseg, accumulate, counts, num);
    if (need_hi > HIST_WAVE_MAX)
        hipLaunchKernelGGL((seg_histogram_block_kernel<Segs>), dim3((unsigned)nseg), dim3(HS_THREADS), 0, st,
                           segs, nseg, accumulate, counts, num);
    return hipGetLastError();
}

}  // namespace

// Shape checks happen in abi.cpp (check_strided / check_ragged) before these run.
hipError_t segment_histogram_strided(const uint32_t* ns, int64_t nseg, int64_t seg_stride,
                                     int64_t seg_begin, int64_t seg_len, int64_t cap, int accumulate,
                                     uint32_t* counts, int32_t* num, hipStream_t st) {
    if (nseg <= 0) return hipSuccess;
    StridedSegs segs{ns, seg_stride, seg_begin, seg_len, cap};
    const SegRange r = seg_range(segs);
    return launch_histogram(segs, nseg, r.need_lo, r.need_hi, accumulate, counts, num, st);
}

hipError_t segment_histogram_ragged(const uint32_t* ns, const int64_t* seg_off, const int32_t* seg_len,
                                    int64_t nseg, int64_t max_len, int64_t cap, bool aligned16,
                                    int accumulate, uint32_t* counts, int32_t* num, hipStream_t st) {
    if (nseg <= 0) return hipSuccess;
    RaggedSegs segs{ns, seg_off, seg_len, cap};
    const SegRange r = seg_range(segs, max_len, aligned16);
    return launch_histogram(segs, nseg, r.need_lo, r.need_hi, accumulate, counts, num, st);
}

}  // namespace nvrx
