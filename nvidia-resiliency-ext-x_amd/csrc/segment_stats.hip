// segment_stats.hip -- per-kernel duration statistics on gfx950 (MI355X).
//
// Replaces the reference's CPU computeStats (straggler/cupti_src/CuptiProfiler.cpp:44-74,
// reached from CuptiProfiler::getStats :136-146) for a whole batch of segments at once.
// A segment is one (rank, kernel) ring: the last `cap` integer-ns durations
// (CircularBuffer.h:53-69 keeps the last statsMaxLenPerKernel pushes).
//
// FAST mode (the batch/bench path), one 64-lane wave per segment:
//   * the segment (<= 64*PL samples) is streamed HBM -> VGPRs with 16-B loads, once;
//   * MIN/MAX: wave min/max of the u32 keys;
//   * AVG/STD: exact u64 sum of (x - min) and an f64 sum of squares (no sort needed);
//   * MED: radix select on (x - min) with a wave-private LDS histogram (NB bins);
//     the target bucket is then resolved by candidate extraction (<= 64 values,
//     ballot/mbcnt compaction + rank-by-compare) or another histogram level.
//   MIN/MAX/MED are selected on the integer keys and converted exactly as
//   CuptiProfiler.cpp:187 converts one duration; ns -> us is monotone, so the
//   k-th smallest key converts to the k-th smallest float: NUM/MIN/MAX/MED are
//   bit-exact with the reference.  AVG/STD are the exact mean/population std of
//   the retained samples rounded once to f32 (within ~1e-6 of the reference's
//   sequential-f32 values; see DESIGN.md, "AVG/STD modes").
//
// EXACT mode (live path, small batches): one 256-thread workgroup per segment,
//   samples converted to f32 us, bitonic-sorted in LDS, then AVG = sequential f32
//   sum over the sorted samples and STD = sqrtf(sequential sum of squares / n),
//   exactly as CuptiProfiler.cpp:63-69 -- every field bit-exact.

#include <algorithm>

#include "segment_emit.h"
#include "segment_sorted.h"

namespace nvrx {

// FULL: the host guarantees every segment holds exactly 64*PL samples starting on a
// 16-byte boundary, so no lane needs masking.  !FULL: per-element masks (branch-free).
template <int PL, bool FULL, class Segs>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(OccV<PL, FULL>::W)))
void seg_stats_fast_kernel(Segs segs, int64_t nseg, nvrx_stats_soa out, ColRef cr) {
    constexpr int NB = Bins<PL>::NB;
    __shared__ __attribute__((aligned(16))) unsigned lds_hist[4 * NB];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t s = (int64_t)blockIdx.x * 4 + wave;
    if (s >= nseg) return;  // wave-uniform; the kernel has no workgroup barrier
    unsigned* hist = lds_hist + wave * NB;

    const uint32_t* p;
    int n;
    segs.get(s, p, n);
    if (n <= 0) {  // n < 0: segment reduced elsewhere (records_stats), outputs untouched
        if (n == 0 && lane == 0) {
            write_empty(out, s);
            cr.miss(s);
        }
        return;
    }

    unsigned v[PL];
    int m0;
    unsigned x0;
    if constexpr (FULL)
        load_segment<PL, true>(p, n, v, m0, x0);
    else
        load_segment_pivot<PL>(p, n, v, m0, x0);
    const LeanOut<PL> r = lean_core<PL, FULL>(v, n, m0, x0, hist);
    emit_stats(out, s, n, r.mn, r.mx, r.d0, r.d1, (double)r.sd, r.sq, r.c, cr);
    // keys of >= 3.76 s take the decoded moments (rare, wave-uniform)
    if (r.mx >= NVRX_KEY_WIDE) wide_moments(p, n, s, out);
}

// FULL segments (configs[1] / configs[2]): each wave reduces `group` consecutive segments one
// after another and keeps what lean_core returns for segment s0 + j in lane j (one compare and
// nine selects), so the epilogue -- the unit conversions, the f64 quotients and the root, the
// stores -- runs once per group, lane-parallel with coalesced stores, instead of once per
// segment on one busy lane (~55 VALU, half of them f64).  Same arithmetic as emit_stats, so the
// same bits.  Groups of up to 8 (lean_group): the sweep on configs[2] in DESIGN.md section 3.1.
constexpr int GROUP_WAVES = 4;  // waves per workgroup of the group kernel
template <int PL, class Segs>
__global__ __launch_bounds__(64 * GROUP_WAVES) __attribute__((amdgpu_waves_per_eu(Occ<PL>::W)))
void seg_stats_lean_group_kernel(Segs segs, int64_t nseg, int group, nvrx_stats_soa out, ColRef cr) {
    constexpr int NB = Bins<PL>::NB;
    __shared__ __attribute__((aligned(16))) unsigned lds_hist[GROUP_WAVES * NB];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int64_t s0 = ((int64_t)blockIdx.x * GROUP_WAVES + wave) * group;
    if (s0 >= nseg) return;
    const int cnt = (int)(nseg - s0 < group ? nseg - s0 : group);
    unsigned* hist = lds_hist + wave * NB;
    LaneResults<PL, uint64_t> res{};
    int n = 0;
    for (int j = 0; j < cnt; ++j) {
        const uint32_t* p;
        segs.get(s0 + j, p, n);
        unsigned v[PL];
        int m0;
        unsigned x0;
        load_segment<PL, true>(p, n, v, m0, x0);
        res.keep(j, lean_core<PL>(v, n, 0, x0, hist));
    }
    if (lane < cnt) res.emit(out, s0 + lane, n, cr);
    res.each_wide([&](int j) {  // keys of >= 3.76 s: the decoded moments (rare)
        const uint32_t* p;
        segs.get(s0 + j, p, n);
        wide_moments(p, n, s0 + j, out);
    });
}

template <int NMAX, class Segs>
__global__ __launch_bounds__(256) void seg_stats_exact_kernel(Segs segs, int64_t nseg,
                                                              nvrx_stats_soa out, ColRef cr) {
    __shared__ __attribute__((aligned(16))) float sbuf[NMAX];
    const int64_t s = blockIdx.x;
    if (s >= nseg) return;
    const uint32_t* p;
    int n;
    segs.get(s, p, n);
    if (n <= 0) {  // n < 0: reduced elsewhere
        if (n == 0 && threadIdx.x == 0) {
            write_empty(out, s);
            cr.miss(s);
        }
        return;
    }
    exact_body<NMAX>(p, n, s, sbuf, out, cr);
}

// segments s0 + blockIdx.x (a chunk of the batch: the scratch holds one slice per block)
template <class Segs>
__global__ __launch_bounds__(XG_THREADS) void seg_stats_exact_global_kernel(
    Segs segs, int64_t s0, int64_t nseg, float* work, int64_t np2, nvrx_stats_soa out, ColRef cr) {
    __shared__ __attribute__((aligned(16))) float lds[XG_CHUNK];
    const int64_t s = s0 + blockIdx.x;
    if (s >= nseg) return;
    const uint32_t* p;
    int n;
    segs.get(s, p, n);
    if (n <= 0) {
        if (n == 0 && threadIdx.x == 0) {
            write_empty(out, s);
            cr.miss(s);
        }
        return;
    }
    exact_global_body(p, n, s, work + (int64_t)blockIdx.x * np2, lds, out, cr);
}

// ---------------------------------------------------------------- launchers
// col_ref: [min med bits | missing] per column, initialised to (+inf, 0) on `st` by one
// kernel (a launch that HIP graph capture records like any other)
__global__ void colref_init_kernel(uint32_t* col_ref, int64_t ncols) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * ncols) col_ref[i] = i < ncols ? 0x7F800000u : 0u;
}
static inline hipError_t make_colref(uint32_t* col_ref, int64_t ncols, hipStream_t st, ColRef& cr,
                                     bool ready = false) {
    cr = ColRef::none();
    if (!col_ref || ncols <= 0) return hipSuccess;
    cr = ColRef{col_ref, col_ref + ncols, ncols, 1.0 / (double)ncols};
    if (ready) return hipSuccess;  // NVRX_STATS_COLREF_READY: initialised by the caller
    hipLaunchKernelGGL(colref_init_kernel, dim3((unsigned)((2 * ncols + 255) / 256)), dim3(256), 0,
                       st, col_ref, ncols);
    return hipGetLastError();
}

// Segments per wave of the group kernel: up to LEAN_GROUP_MAX while the grid keeps at least
// LEAN_GROUP_WAVES waves.  configs[2] statistics interleaved on one box
// (profiles/r03/group_size/): 4 / 6 / 8 / 12 / 32 / 64 per wave 5.70 / 5.87 / 5.57 / 5.78 / 6.04
// / 5.87 ms (round-start library 6.00 ms); a prefetch of the next segment's loads (80 VGPRs,
// 6 waves / SIMD) 5.90-5.94 at 64.
constexpr int LEAN_GROUP_MAX = 8;
// one segment's results per lane, wide-key flags in a 64-bit mask
static_assert(LEAN_GROUP_MAX >= 1 && LEAN_GROUP_MAX <= 64, "LEAN_GROUP_MAX in [1, 64]");
constexpr int LEAN_GROUP_WAVES = 32768;  // the fewest waves a grouped grid keeps
static inline int lean_group(int64_t nseg) {
    const int64_t g = nseg / LEAN_GROUP_WAVES;
    return g < 1 ? 1 : g > LEAN_GROUP_MAX ? LEAN_GROUP_MAX : (int)g;
}

template <int PL, class Segs>
static void launch_pl(const Segs& segs, int64_t nseg, bool full, const nvrx_stats_soa& out,
                      const ColRef& cr, hipStream_t st) {
    // FULL: unmasked lean_core with the group epilogue; otherwise the masked lean_core
    if (full) {
        const int g = lean_group(nseg);
        const int64_t waves = (nseg + g - 1) / g;
        hipLaunchKernelGGL((seg_stats_lean_group_kernel<PL, Segs>),
                           dim3((unsigned)((waves + GROUP_WAVES - 1) / GROUP_WAVES)),
                           dim3(64 * GROUP_WAVES), 0, st, segs, nseg, g, out, cr);
    } else {
        const dim3 grid((unsigned)((nseg + 3) / 4)), block(256);
        hipLaunchKernelGGL((seg_stats_fast_kernel<PL, false, Segs>), grid, block, 0, st, segs, nseg, out, cr);
    }
}

// need = samples + alignment slack a wave must hold; picks the smallest PL.  `full`
// (every segment exactly 64*PL samples, 16-B aligned) selects the unmasked variant.
template <class Segs>
static hipError_t launch_fast(const Segs& segs, int64_t nseg, int64_t need, int64_t exact_len,
                              const nvrx_stats_soa& out, const ColRef& cr, hipStream_t st) {
    if (need <= 64 * 4)
        launch_pl<4>(segs, nseg, exact_len == 64 * 4, out, cr, st);
    else if (need <= 64 * 8)
        launch_pl<8>(segs, nseg, exact_len == 64 * 8, out, cr, st);
    else if (need <= 64 * 16)
        launch_pl<16>(segs, nseg, exact_len == 64 * 16, out, cr, st);
    else if (need <= 64 * 32)
        launch_pl<32>(segs, nseg, exact_len == 64 * 32, out, cr, st);
    else if (need <= 64 * 64)
        launch_pl<64>(segs, nseg, exact_len == 64 * 64, out, cr, st);
    else if (need <= 64 * 128)
        launch_pl<128>(segs, nseg, exact_len == 64 * 128, out, cr, st);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

template <class Segs>
static hipError_t launch_exact(const Segs& segs, int64_t nseg, int64_t max_len,
                               const nvrx_stats_soa& out, const ColRef& cr, hipStream_t st) {
    const dim3 grid((unsigned)nseg), block(256);
    if (max_len <= 1024)
        hipLaunchKernelGGL((seg_stats_exact_kernel<1024, Segs>), grid, block, 0, st, segs, nseg, out, cr);
    else if (max_len <= 8192)
        hipLaunchKernelGGL((seg_stats_exact_kernel<8192, Segs>), grid, block, 0, st, segs, nseg, out, cr);
    else if (max_len <= NVRX_LDS_SEGMENT)
        hipLaunchKernelGGL((seg_stats_exact_kernel<NVRX_LDS_SEGMENT, Segs>), grid, block, 0, st, segs, nseg, out, cr);
    else if (max_len <= NVRX_MAX_SEGMENT) {
        // longer rings: device scratch, the batch in chunks of blocks (one slice each)
        const int64_t np2 = exact_global_np2(max_len), chunk = exact_global_blocks(np2, nseg);
        void* work = nullptr;
        hipError_t e = scratch_alloc(&work, (size_t)(chunk * np2) * sizeof(float), st);
        if (e != hipSuccess) return e;
        for (int64_t s0 = 0; s0 < nseg && e == hipSuccess; s0 += chunk) {
            hipLaunchKernelGGL((seg_stats_exact_global_kernel<Segs>), dim3((unsigned)std::min(chunk, nseg - s0)),
                               dim3(XG_THREADS), 0, st, segs, s0, nseg, (float*)work, np2, out, cr);
            e = hipGetLastError();
        }
        const hipError_t f = hipFreeAsync(work, st);  // on the error path too
        return e != hipSuccess ? e : f;
    } else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// Shape checks happen here, on the host, before any launch: a fast-mode wave
// holds at most 64*128 samples (+ up to 3 slots of 16-B misalignment); longer
// or misaligned-and-full segments go to the EXACT kernel (bit-exact, slower).
hipError_t segment_stats_strided(const uint32_t* ns, int64_t nseg, int64_t seg_stride,
                                 int64_t seg_begin, int64_t seg_len, int64_t cap, int mode,
                                 const nvrx_stats_soa& out, uint32_t* col_ref, int64_t ncols,
                                 hipStream_t st) {
    const bool ready = (mode & NVRX_STATS_COLREF_READY) != 0;
    mode &= ~NVRX_STATS_COLREF_READY;
    ColRef cr;
    if (hipError_t e = make_colref(col_ref, ncols, st, cr, ready); e != hipSuccess) return e;
    if (nseg <= 0) return hipSuccess;
    StridedSegs segs{ns, seg_stride, seg_begin, seg_len, cap};
    const SegRange r = seg_range(segs);
    if (r.keep > NVRX_MAX_SEGMENT) return hipErrorInvalidValue;
    if (mode == NVRX_STATS_EXACT || r.need_hi > 64 * 128) return launch_exact(segs, nseg, r.keep, out, cr, st);
    // every strided segment has the same length and (aligned) phase
    return launch_fast(segs, nseg, r.need_hi, r.aligned ? r.keep : -1, out, cr, st);
}

// raw u32 ns (durations below 2^32 ns, never encoded) -> duration keys, in place: values from
// NVRX_KEY_WIDE (3.76 s) up become 0xE0000000 + bits(f32(ns)) - bits(f32(0xE0000000)), as
// nvrx_duration_key encodes the same u64 (v_cvt_f32_u32 rounds to nearest even, like the u64
// conversion of CuptiProfiler.cpp:187).  One coalesced read-modify-write pass.
__global__ __launch_bounds__(256) void encode_ns_u32_kernel(uint32_t* ns, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint32_t v = ns[i];
        if (v >= NVRX_KEY_WIDE) ns[i] = NVRX_KEY_WIDE + (__float_as_uint((float)v) - NVRX_KEY_WIDE_F32BITS);
    }
}

hipError_t encode_ns_u32(uint32_t* ns, int64_t n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(encode_ns_u32_kernel, dim3((unsigned)blocks), dim3(256), 0, st, ns, n);
    return hipGetLastError();
}

}  // namespace nvrx
