// segment_ragged.hip -- statistics of ragged segments (gfx950): length classes.
//
// Ragged inputs (the per-(rank, kernel) buckets of record streams, the profiler's
// per-kernel rings) mix a few long segments with very many short ones: under a Zipf
// kernel-frequency law most kernels fire a handful of times per report interval
// (SURVEY.md 8(d), C4).  One wave per segment sized for the longest one would spend
// 64*PL lanes-slots on a 3-sample segment, so segments are first sorted into length
// classes and each class runs the kernel shaped for it:
//
//   n == 0            classifier writes the empty KernelStats (num 0, NaN) itself
//   n <= 8..128       one LANE per segment: the samples in registers, a sorting
//                     sorting network, then CuptiProfiler.cpp:53-71 statement by
//                     statement (sequential f32 sums) -- every field bit-exact
//   n <= 64*PL        one WAVE per segment (lean_core, segment_wave.h), PL 4..128
//   longer / EXACT    one WORKGROUP per segment (exact_body, segment_sorted.h)
//
// Classification is three small launches over the segment lengths (count per block,
// scan, scatter) into one id list ordered by class; every class kernel is persistent
// (grid = CUs x occupancy) and reads its [start, count) from device memory, so the
// host never waits for the class sizes.
#include <mutex>

#include "segment_ragged_kernels.h"

namespace nvrx {
namespace ragged {

// ---------------------------------------------------------------- the classifier
// Wave-aggregated class counting: one LDS atomic per distinct class present in the
// wave (leader = lowest lane); returns this lane's rank among same-class lanes plus the
// class's previous count.  cls < 0: lane does not take part.
__device__ __forceinline__ uint32_t wave_class_add(uint32_t* lcnt, int cls) {
    uint64_t pending = __ballot(cls >= 0);
    uint32_t mine = 0;
    while (pending) {
        const int leader = __builtin_ffsll(pending) - 1;
        const int c = __builtin_amdgcn_readlane(cls, leader);
        const uint64_t grp = __ballot(cls == c) & pending;
        uint32_t base = 0;
        if (lane_id() == leader) base = atomicAdd(&lcnt[c], (uint32_t)__popcll(grp));
        base = __builtin_amdgcn_readlane(base, leader);
        if (cls == c) mine = base + mbcnt(grp);
        pending &= ~grp;
    }
    return mine;
}

constexpr int CLS_THREADS = 1024;
constexpr int CLS_MAX_BLOCKS = 1024;
// segment lengths loaded per thread before any is classified: a block's chunk is tens of
// thousands of segments, and one dependent load per 1024 of them left both passes
// latency-bound (configs[3]: 153 + 118 us for 33.5 M segments)
constexpr int CLS_BATCH = 8;
static_assert(CLS_BATCH >= 1 && CLS_BATCH < 16 && 4 * NCLASS <= 64, "4-bit packed class counts per batch");

// pass 1: per-block class counts (bcnt[b][c]); empty segments are written here
__global__ __launch_bounds__(CLS_THREADS) void classify_count_kernel(
    RaggedSegs segs, int64_t nseg, int64_t chunk, int aligned16, int exact, int full_n, uint32_t* bcnt,
    nvrx_stats_soa out) {
    const ColRef cr = ColRef::none();  // column references: kernel_ref afterwards
    __shared__ uint32_t lcnt[NCLASS];
    if (threadIdx.x < NCLASS) lcnt[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(nseg, lo + chunk);
    // per-lane class counters in registers (no LDS traffic per segment), one wave reduction
    // and one LDS add per class at the end
    unsigned mine[NCLASS];
#pragma unroll
    for (int c = 0; c < NCLASS; ++c) mine[c] = 0u;
    for (int64_t b = lo; b < hi; b += CLS_THREADS * CLS_BATCH) {
        int n[CLS_BATCH];
#pragma unroll
        for (int j = 0; j < CLS_BATCH; ++j) {
            const int64_t s = b + j * CLS_THREADS + threadIdx.x;
            n[j] = s < hi ? segs.kept_len(s) : -1;
        }
        // the batch's class counts packed 4 bits per class in one 64-bit word (one shift and
        // add per segment instead of a compare and add per class), unpacked once per batch
        uint64_t pk = 0;
#pragma unroll
        for (int j = 0; j < CLS_BATCH; ++j) {
            const int64_t s = b + j * CLS_THREADS + threadIdx.x;
            if (n[j] == 0) {
                write_empty(out, s);
                cr.miss(s);
            } else if (n[j] > 0) {  // n < 0: reduced elsewhere (or past the chunk)
                pk += 1ull << (4 * seg_class(n[j], aligned16 != 0, exact != 0, full_n));
            }
        }
#pragma unroll
        for (int c = 0; c < NCLASS; ++c) mine[c] += (uint32_t)(pk >> (4 * c)) & 15u;
    }
#pragma unroll
    for (int c = 0; c < NCLASS; ++c) {
        const unsigned w = wave_sum_u32(mine[c]);
        if (lane_id() == 0 && w) atomicAdd(&lcnt[c], w);
    }
    __syncthreads();
    if (threadIdx.x < NCLASS) bcnt[(int64_t)blockIdx.x * NCLASS + threadIdx.x] = lcnt[threadIdx.x];
}

// pass 2 (one block): boff[b][c] = start of class c + blocks before b; cls[c] = {start, count}
__global__ __launch_bounds__(CLS_MAX_BLOCKS) void classify_scan_kernel(uint32_t* bcnt, int nblocks,
                                                                       uint32_t* cls) {
    __shared__ uint32_t wsum[CLS_MAX_BLOCKS / 64];
    const int b = threadIdx.x;
    const int w = b >> 6;
    uint32_t start = 0;
    for (int c = 0; c < NCLASS; ++c) {
        const uint32_t v = b < nblocks ? bcnt[(int64_t)b * NCLASS + c] : 0u;
        const uint32_t incl = wave_incl_scan_u32(v);
        if (lane_id() == 63) wsum[w] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int j = 0; j < CLS_MAX_BLOCKS / 64; ++j) {
            before += j < w ? wsum[j] : 0u;
            all += wsum[j];
        }
        if (b < nblocks) bcnt[(int64_t)b * NCLASS + c] = start + before + incl - v;
        if (b == 0) {
            cls[2 * c] = start;
            cls[2 * c + 1] = all;
        }
        start += all;
        __syncthreads();
    }
}

// pass 3: scatter segment ids into the class-ordered list
__global__ __launch_bounds__(CLS_THREADS) void classify_scatter_kernel(
    RaggedSegs segs, int64_t nseg, int64_t chunk, int aligned16, int exact, int full_n, const uint32_t* boff,
    uint32_t* list) {
    __shared__ uint32_t lcnt[NCLASS];
    __shared__ uint32_t lbase[NCLASS];
    if (threadIdx.x < NCLASS) {
        lcnt[threadIdx.x] = 0u;
        lbase[threadIdx.x] = boff[(int64_t)blockIdx.x * NCLASS + threadIdx.x];
    }
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(nseg, lo + chunk);
    for (int64_t b = lo; b < hi; b += CLS_THREADS * CLS_BATCH) {
        int n[CLS_BATCH];
#pragma unroll
        for (int j = 0; j < CLS_BATCH; ++j) {
            const int64_t s = b + j * CLS_THREADS + threadIdx.x;
            n[j] = s < hi ? segs.kept_len(s) : -1;
        }
#pragma unroll
        for (int j = 0; j < CLS_BATCH; ++j) {  // the same order as the counting pass
            const int64_t s = b + j * CLS_THREADS + threadIdx.x;
            const int cls = n[j] > 0 ? seg_class(n[j], aligned16 != 0, exact != 0, full_n) : -1;
            const uint32_t r = wave_class_add(lcnt, cls);
            if (cls >= 0) list[lbase[cls] + r] = (uint32_t)s;
        }
    }
}

// CUs of the current device (the class kernels' grids), asked once per device
int cu_count() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            n <= 0)
            n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

}  // namespace ragged

using namespace ragged;

// The class kernels are dealt over the caller's stream and one side stream per device
// (configs[3]: 4.28 -> 4.15 ms; 3 / 4 streams were no faster).
constexpr int RAGGED_STREAMS = 2;
struct Fork {
    hipStream_t s[RAGGED_STREAMS];  // s[0] unused: slot 0 is the caller's stream
    hipEvent_t fork, join[RAGGED_STREAMS];
};
// One caller at a time per process from fork to join (the caller holds `fork_mutex()`): the
// fork / join events and side streams are shared, and another thread's event record between
// this caller's record and wait would hand it the wrong dependency.
static std::mutex& fork_mutex() {
    static std::mutex mu;
    return mu;
}
// out = nullptr (every class on `st`) unless the side stream of st's device can take work:
// st must belong to the current device (the side stream is created there) and the side
// stream must not be inside a graph capture -- once forked into a capture it stays part of
// it until that capture ends, and another caller's eager work on it would be recorded into
// that graph.  A capturing `st` forks as usual (the capture follows the events), also into
// a side stream already joined to that same capture.
static hipError_t ragged_fork(hipStream_t st, Fork*& out) {
    out = nullptr;
    static Fork* forks[64] = {nullptr};
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipSuccess;
    if (st != nullptr) {
        hipDevice_t sdev = 0;
        if (hipError_t e = hipStreamGetDevice(st, &sdev); e != hipSuccess) return e;
        if ((int)sdev != dev) return hipSuccess;
    }
    if (!forks[dev]) {
        Fork* f = new Fork{};
        hipError_t e = hipEventCreateWithFlags(&f->fork, hipEventDisableTiming);
        for (int i = 1; i < RAGGED_STREAMS && e == hipSuccess; ++i) {
            e = hipStreamCreateWithFlags(&f->s[i], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&f->join[i], hipEventDisableTiming);
        }
        if (e != hipSuccess) return e;  // leaked on failure: a one-time setup
        forks[dev] = f;
    }
    Fork* f = forks[dev];
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    unsigned long long id_st = 0;
    if (hipError_t e = hipStreamGetCaptureInfo(st, &cst, &id_st); e != hipSuccess) return e;
    for (int i = 1; i < RAGGED_STREAMS; ++i) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        unsigned long long id = 0;
        if (hipError_t e = hipStreamGetCaptureInfo(f->s[i], &cs, &id); e != hipSuccess) return e;
        // busy in a capture other than st's own
        if (cs != hipStreamCaptureStatusNone && !(cst == hipStreamCaptureStatusActive && id == id_st))
            return hipSuccess;
    }
    if (hipError_t e = hipEventRecord(f->fork, st); e != hipSuccess) return e;
    for (int i = 1; i < RAGGED_STREAMS; ++i)
        if (hipError_t e = hipStreamWaitEvent(f->s[i], f->fork, 0); e != hipSuccess) return e;
    out = f;
    return hipSuccess;
}
static hipError_t ragged_join(hipStream_t st, Fork* f) {
    for (int i = 1; i < RAGGED_STREAMS; ++i) {
        if (hipError_t e = hipEventRecord(f->join[i], f->s[i]); e != hipSuccess) return e;
        if (hipError_t e = hipStreamWaitEvent(st, f->join[i], 0); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The class kernels over the class-ordered segment list: keep = the longest retained segment;
// classes it rules out are not launched.
static hipError_t ragged_launch_classes(const RaggedSegs& segs, const uint32_t* cls_list,
                                        const uint32_t* cls, const SegRange& r, bool exact,
                                        const nvrx_stats_soa& out, hipStream_t st) {
    const uint32_t* list = cls_list;
    const int64_t keep = r.keep, need = r.need_hi;
    const bool aligned16 = r.aligned;
    // class kernels; classes that max_len rules out are not launched.  With side streams the
    // classes are dealt round robin over them in launch order (fork / join by events, which HIP
    // graph capture follows), so one class's tail and latency-bound waves overlap the next class.
    std::lock_guard<std::mutex> lock(fork_mutex());
    Fork* fk = nullptr;
    if (hipError_t e = ragged_fork(st, fk); e != hipSuccess) return e;
    int k = 0;
    const auto S = [&]() {
        const int i = fk ? k++ % RAGGED_STREAMS : 0;
        return i ? fk->s[i] : st;
    };
    const uint32_t* c = cls;
    // order: the long-segment classes first, then the wave classes, then the lane classes (a FULL
    // kernel last ran alone behind the others; DESIGN 3.2, profiles/r05/class_order_ab.log)
    hipError_t e = hipSuccess;
    if (!exact)
        if (const int fn = full_len(keep, aligned16, exact))  // the FULL class
            ragged_launch_full(fn / 64, segs, list, c + 2 * C_F, out, S());
    if (exact ? keep > 128 : need > 64 * 128)  // the workgroup class
        e = ragged_launch_exact(segs, list, c + 2 * C_X, keep, out, S());
    if (e == hipSuccess) {
        if (!exact) {  // the wave classes, ascending PL: C_W4, C_W8 .. C_W128
            if (keep > 128) ragged_launch_list(4, segs, list, c + 2 * C_W4, out, S());
            for (int pl = 8, cl = C_W8; pl <= 128; pl *= 2, ++cl)
                if (need > 64 * (pl / 2)) ragged_launch_list(pl, segs, list, c + 2 * cl, out, S());
        }
        for (int n = 8, cl = C_T8; n <= 128; n *= 2, ++cl)  // the lane classes, ascending N
            if (n == 8 || keep > n / 2) ragged_launch_lane(n, segs, list, c + 2 * cl, aligned16, out, S());
        e = hipGetLastError();
    }
    // joined on every path: a side stream left forked would leave a graph capture unjoined
    if (fk) {
        const hipError_t j = ragged_join(st, fk);
        if (e == hipSuccess) e = j;
    }
    return e;
}

hipError_t segment_stats_ragged(const uint32_t* ns, const int64_t* seg_off, const int32_t* seg_len,
                                int64_t nseg, int64_t max_len, int64_t cap, int mode,
                                bool aligned16, const nvrx_stats_soa& out, uint32_t* col_ref,
                                int64_t ncols, hipStream_t st) {
    // the column reference (MIN over rows of MED, missing flags) is a column reduction over the
    // finished statistics (kernel_ref), not per-segment atomics in the class kernels: the class
    // kernels then carry no column-reference state (fewer SGPRs, fewer spills)
    const auto colref = [&]() -> hipError_t {
        if (!col_ref || ncols <= 0) return hipSuccess;
        return kernel_ref(out.num, out.med, nseg > 0 ? nseg / ncols : 0, ncols, nullptr, col_ref, st);
    };
    if (nseg <= 0) return colref();
    RaggedSegs segs{ns, seg_off, seg_len, cap};
    const SegRange r = seg_range(segs, max_len, aligned16);
    const int64_t keep = r.keep;
    if (keep > NVRX_MAX_SEGMENT) return hipErrorInvalidValue;
    const bool exact = mode == NVRX_STATS_EXACT;
    if (nseg >= ((int64_t)1 << 32) - ((int64_t)1 << 26)) return hipErrorInvalidValue;  // 32-bit lists

    const int64_t nblocks = std::min<int64_t>(CLS_MAX_BLOCKS, (nseg + CLS_THREADS - 1) / CLS_THREADS);
    const int64_t chunk = (nseg + nblocks - 1) / nblocks;
    // scratch: list [nseg] | bcnt [nblocks][NCLASS] | cls [NCLASS][2]
    const size_t bytes = (size_t)(nseg + nblocks * NCLASS + 2 * NCLASS) * sizeof(uint32_t);
    void* ws = nullptr;
    if (hipError_t e = scratch_alloc(&ws, bytes, st); e != hipSuccess) return e;
    uint32_t* list = (uint32_t*)ws;
    uint32_t* bcnt = list + nseg;
    uint32_t* cls = bcnt + nblocks * NCLASS;

    // (a one-pass variant -- per-block totals reserving each class's range with global atomics,
    // lists of nseg entries per class -- measured 4.17 / 4.37 ms with 1024 / 256-thread blocks
    // against 4.13 for these three launches on configs[3]: the reservations contend on one
    // address per class)
    hipLaunchKernelGGL(classify_count_kernel, dim3((unsigned)nblocks), dim3(CLS_THREADS), 0, st, segs,
                       nseg, chunk, aligned16 ? 1 : 0, exact ? 1 : 0, full_len(keep, aligned16, exact), bcnt, out);
    hipLaunchKernelGGL(classify_scan_kernel, dim3(1), dim3(CLS_MAX_BLOCKS), 0, st, bcnt, (int)nblocks,
                       cls);
    hipLaunchKernelGGL(classify_scatter_kernel, dim3((unsigned)nblocks), dim3(CLS_THREADS), 0, st,
                       segs, nseg, chunk, aligned16 ? 1 : 0, exact ? 1 : 0, full_len(keep, aligned16, exact), bcnt, list);
    const hipError_t e = ragged_launch_classes(segs, list, cls, r, exact, out, st);
    const hipError_t f = hipFreeAsync(ws, st);  // on the error path too
    if (e != hipSuccess) return e;
    if (f != hipSuccess) return f;
    return colref();
}

}  // namespace nvrx
