// segment_ragged_kernels.h -- the length classes of segment_ragged.hip and their template
// kernels, shared by the translation units that instantiate them (segment_ragged*.hip: split
// so that the heavy instantiations -- 128-sample sorting networks, PL = 64/128 wave bodies --
// compile in parallel; each instantiation lives in exactly one of them).  The kernels that are
// no templates are defined where they are launched: the classifier in segment_ragged.hip, the
// long-ring EXACT kernel in segment_ragged_big.hip.  See segment_ragged.hip for the algorithm.
#pragma once
#include "segment_emit.h"
#include "segment_sorted.h"

namespace nvrx {

// ---------------------------------------------------------------------------
// Length classes of ragged segments.  Class lists: cls[2c] = first list entry of class c,
// cls[2c+1] = its count.
// ---------------------------------------------------------------------------
namespace ragged {
enum : int {
    C_T8 = 0, C_T16, C_T32, C_T64, C_T128,    // lane classes
    C_W4, C_W8, C_W16, C_W32, C_W64, C_W128,  // wave classes (PL)
    C_X,                                      // workgroup (EXACT kernel)
    C_F,                                      // FAST, exactly full_n = 64 * PL samples, 16-B aligned
    NCLASS
};

// need = retained samples + misalignment slack a wave would have to hold.  Every class is a
// power-of-two length range, so the class is ceil(log2) of the length, offset: lane classes
// 1..8 / 9..16 / ... / 65..128, then wave classes of need 129..256 (PL 4) ... 4097..8192 (PL 128).
// full_n (0: none) -- the longest retained length when it is 64 * PL samples for a PL of 16..128
// and the segments start on 16-B boundaries (FAST): segments of exactly that length, the rings
// that overflowed (the hot kernels of a live report, configs[3]'s hottest slot), are the FULL
// class -- no lane masks, and the grouped lane-parallel epilogue (seg_stats_list_full_kernel).
__device__ __forceinline__ int seg_class(int n, bool aligned16, bool exact, int full_n) {
    if (n <= 128) {
        const int l = 32 - __clz(n - 1);  // ceil(log2 n); 0 for n = 1
        return l <= 3 ? C_T8 : l - 3;     // 4..7 -> C_T16..C_T128
    }
    if (exact) return C_X;
    if (n == full_n) return C_F;
    const int need = aligned16 ? n : n + 3;
    const int l = 32 - __clz(need - 1);  // 8..13 -> C_W4..C_W128
    return l <= 13 ? l - 3 : C_X;
}
static_assert(C_T16 == 1 && C_T128 == 4 && C_W4 == 5 && C_W128 == 10 && C_X == 11 && C_F == 12,
              "class order");
// the FULL length of a launch (seg_class): keep if it is 64 * PL for PL in 16..128, else 0
inline int full_len(int64_t keep, bool aligned16, bool exact) {
    return (!exact && aligned16 && (keep == 1024 || keep == 2048 || keep == 4096 || keep == 8192)) ? (int)keep : 0;
}

int cu_count();  // CUs of the current device (segment_ragged.hip)

// ---------------------------------------------------------------- lane classes
template <int N>
struct LaneOcc {
    static constexpr int W = N >= 128 ? 2 : N >= 64 ? 4 : N >= 32 ? 6 : 8;
};

// The shortest segment of a lane class (seg_class): n <= 8, then (N/2, N].
template <int N>
struct LaneMin {
    static constexpr int n = N >= 16 ? N / 2 + 1 : 1;
};

// Segments per lane per step: each takes a chain of three dependent loads (list entry,
// descriptor, samples), so the shortest class runs B chains side by side.
template <int N>
struct LaneBatch {
    static constexpr int B = N <= 8 ? 4 : N <= 16 ? 2 : 1;  // 2 for N = 32: 189 -> 214 us (configs[3])
};

// One lane per segment of 1..N samples.  u32 -> f32 us is monotone, so sorting the
// integer ns sorts the floats computeStats sorts; then CuptiProfiler.cpp:53-71.
template <int N>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LaneOcc<N>::W)))
void seg_stats_lane_kernel(RaggedSegs segs, const uint32_t* list, const uint32_t* cls,
                           int aligned16, nvrx_stats_soa out) {
    const ColRef cr = ColRef::none();  // column references: kernel_ref afterwards
    constexpr int B = LaneBatch<N>::B;
    // 32-bit list indices (a 64-bit loop cost lane<8> 315 -> 372 us); the host keeps the
    // segment count below 2^32 - 2^26, so i + B * G never wraps
    const uint32_t start = cls[0], cnt = cls[1];
    const uint32_t G = gridDim.x * 256u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < cnt; i += B * G) {
        int64_t s[B];
        const uint32_t* p[B];
        int n[B];
#pragma unroll
        for (int b = 0; b < B; ++b) s[b] = i + b * G < cnt ? (int64_t)list[start + i + b * G] : -1;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            n[b] = 0;
            p[b] = nullptr;
            if (s[b] >= 0) segs.get(s[b], p[b], n[b]);  // 1 <= n <= N
        }
        unsigned v[B][N];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (aligned16) {
                const u32x4* q = (const u32x4*)p[b];
#pragma unroll
                for (int j = 0; j < N / 4; ++j) {
                    u32x4 w = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
                    if (4 * j < n[b]) w = q[j];
                    v[b][4 * j + 0] = w.x;
                    v[b][4 * j + 1] = w.y;
                    v[b][4 * j + 2] = w.z;
                    v[b][4 * j + 3] = w.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < N; ++j) v[b][j] = j < n[b] ? p[b][j] : 0xFFFFFFFFu;
            }
        }
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (s[b] >= 0) lane_stats<N, LaneMin<N>::n>(v[b], n[b], s[b], out, cr);
    }
}

template <int N>
void launch_lane(const RaggedSegs& segs, const uint32_t* list, const uint32_t* cls, bool aligned16,
                 const nvrx_stats_soa& out, hipStream_t st) {
    const unsigned blocks = (unsigned)(cu_count() * 2 * LaneOcc<N>::W);
    hipLaunchKernelGGL((seg_stats_lane_kernel<N>), dim3(blocks), dim3(256), 0, st, segs, list, cls,
                       aligned16 ? 1 : 0, out);
}

// ---------------------------------------------------------------- wave / workgroup classes
// One wave per segment over a class list.  Waves take chunks of CH consecutive list
// entries (static round robin; CH shrinks when the class is small so every wave gets
// work); lanes 0..CH-1 fetch the chunk's segment descriptors in one coalesced access, so
// per segment the only dependent memory access is the data itself -- and for PL <= 16
// (short segments, few registers) the next segment's loads are issued before the
// current one is reduced.
template <int PL>
struct ListPrefetch {
    static constexpr bool on = PL <= 16;
};
template <int PL>
struct ListKeepBin {  // level-0 bins in registers while they fit beside the prefetch buffer
    static constexpr bool on = PL <= 8;
};
template <int PL>
struct ListGroup {  // one epilogue per chunk (emit_lane): the short classes, whose chunks are long
    static constexpr bool on = PL <= 8;
};
constexpr int LIST4_OCC = 8, LIST8_OCC = 7;  // waves per SIMD of list<4> / list<8>
template <int PL>
struct ListOcc {  // the prefetch buffer costs PL more VGPRs, the chunk's results nine
    static constexpr int W = PL == 16 ? 6 : PL == 8 ? LIST8_OCC : PL == 4 ? LIST4_OCC : OccV<PL, false>::W;
};
constexpr int LIST_CHUNK = 16;
// results are held one per lane and the wide-key flags in a 32-bit mask
static_assert(LIST_CHUNK >= 1 && LIST_CHUNK <= 32, "LIST_CHUNK must be in [1, 32]");

template <int PL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ListOcc<PL>::W)))
void seg_stats_list_kernel(RaggedSegs segs, const uint32_t* list, const uint32_t* cls,
                           nvrx_stats_soa out) {
    const ColRef cr = ColRef::none();  // column references: kernel_ref afterwards
    constexpr int NB = Bins<PL>::NB;
    __shared__ __attribute__((aligned(16))) unsigned lds_hist[4 * NB];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    unsigned* hist = lds_hist + wave * NB;
    const uint32_t start = cls[0], cnt = cls[1];
    const uint32_t G = gridDim.x * 4u;
    const uint32_t CH = max(1u, min((uint32_t)LIST_CHUNK, cnt / (4u * G)));
    for (uint32_t c0 = (blockIdx.x * 4u + wave) * CH; c0 < cnt; c0 += G * CH) {
        const int m = (int)min(CH, cnt - c0);
        uint32_t sid = 0, plo = 0, phi = 0;
        int nn = 0;
        if (lane < m) {
            sid = list[start + c0 + lane];
            const uint32_t* p;
            segs.get(sid, p, nn);
            plo = (uint32_t)(uintptr_t)p;
            phi = (uint32_t)((uintptr_t)p >> 32);
        }
        auto desc = [&](int j, int64_t& s, const uint32_t*& p, int& n) {
            s = (uint32_t)__builtin_amdgcn_readlane((int)sid, j);
            p = (const uint32_t*)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)phi, j) << 32) |
                                  (uint32_t)__builtin_amdgcn_readlane((int)plo, j));
            n = __builtin_amdgcn_readlane(nn, j);
        };
        int64_t s;
        const uint32_t* p;
        int n;
        desc(0, s, p, n);
        // the chunk's results, segment j in lane j (lane j already holds its id and length):
        // one epilogue per chunk, lane-parallel, instead of one per segment
        LaneResults<PL, uint32_t> res{};
        unsigned v[PL];
        if (ListPrefetch<PL>::on) {
            issue_loads<PL>(p, n, v);
            unsigned probes = issue_probes(p, n);
            for (int j = 0; j < m; ++j) {
                // unconditional prefetch (the last one re-reads the current segment): a load
                // under a branch would make the waitcnt at the join cover it
                int64_t s2;
                const uint32_t* p2;
                int n2;
                desc(j + 1 < m ? j + 1 : j, s2, p2, n2);
                unsigned w[PL];
                issue_loads<PL>(p2, n2, w);
                const unsigned probes2 = issue_probes(p2, n2);
                int m0;
                unsigned x0;
                finish_loads_pivot<PL>(p, n, v, probes, m0, x0);
                const LeanOut<PL> r = lean_core<PL, false, ListKeepBin<PL>::on>(v, n, m0, x0, hist);
                if (ListGroup<PL>::on) {
                    res.keep(j, r);
                } else {
                    emit_stats(out, s, n, r.mn, r.mx, r.d0, r.d1, (double)r.sd, r.sq, r.c, cr);
                    if (r.mx >= NVRX_KEY_WIDE) wide_moments(p, n, s, out);
                }
#pragma unroll
                for (int i = 0; i < PL; ++i) v[i] = w[i];
                probes = probes2;
                s = s2;
                p = p2;
                n = n2;
            }
        } else {
            for (int j = 0; j < m; ++j) {
                if (j) desc(j, s, p, n);
                int m0;
                unsigned x0;
                load_segment_pivot<PL>(p, n, v, m0, x0);
                const LeanOut<PL> r = lean_core<PL, false, ListKeepBin<PL>::on>(v, n, m0, x0, hist);
                if (ListGroup<PL>::on) {
                    res.keep(j, r);
                } else {
                    emit_stats(out, s, n, r.mn, r.mx, r.d0, r.d1, (double)r.sd, r.sq, r.c, cr);
                    if (r.mx >= NVRX_KEY_WIDE) wide_moments(p, n, s, out);
                }
            }
        }
        if (ListGroup<PL>::on && lane < m) res.emit(out, (int64_t)sid, nn, cr);
        res.each_wide([&](int j) {  // keys of >= 3.76 s: the decoded moments (rare)
            desc(j, s, p, n);
            wide_moments(p, n, s, out);
        });
    }
}

template <int PL>
void launch_list(const RaggedSegs& segs, const uint32_t* list, const uint32_t* cls,
                 const nvrx_stats_soa& out, hipStream_t st) {
    const unsigned blocks = (unsigned)(cu_count() * ListOcc<PL>::W);
    hipLaunchKernelGGL((seg_stats_list_kernel<PL>), dim3(blocks), dim3(256), 0, st, segs, list, cls,
                       out);
}

// The FULL class (seg_class C_F: exactly 64 * PL samples, PL 16..128, 16-B aligned, FAST): the
// configs[1] group kernel's body over a class list -- each wave takes LIST_FULL_GROUP consecutive
// list entries, lanes 0..m-1 fetch their ids in one access, every segment runs the unmasked
// lean_core, and segment j's results wait in lane j for one lane-parallel epilogue.
constexpr uint32_t LIST_FULL_GROUP = 4;
template <int PL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Occ<PL>::W)))
void seg_stats_list_full_kernel(RaggedSegs segs, const uint32_t* list, const uint32_t* cls,
                                nvrx_stats_soa out) {
    const ColRef cr = ColRef::none();  // column references: kernel_ref afterwards
    constexpr int NB = Bins<PL>::NB;
    constexpr uint32_t G = LIST_FULL_GROUP;
    __shared__ __attribute__((aligned(16))) unsigned lds_hist[4 * NB];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    unsigned* hist = lds_hist + wave * NB;
    const uint32_t start = cls[0], cnt = cls[1];
    const uint32_t W = gridDim.x * 4u;
    for (uint32_t c0 = (blockIdx.x * 4u + wave) * G; c0 < cnt; c0 += W * G) {
        const int m = (int)min(G, cnt - c0);
        const uint32_t sid = lane < m ? list[start + c0 + lane] : 0u;
        LaneResults<PL, uint32_t> res{};
        int n = 0;
        for (int j = 0; j < m; ++j) {
            const int64_t s = (uint32_t)__builtin_amdgcn_readlane((int)sid, j);
            const uint32_t* p;
            segs.get(s, p, n);  // n == 64 * PL (the class)
            unsigned v[PL];
            int m0;
            unsigned x0;
            load_segment<PL, true>(p, n, v, m0, x0);
            res.keep(j, lean_core<PL>(v, n, 0, x0, hist));
        }
        if (lane < m) res.emit(out, (int64_t)sid, n, cr);
        res.each_wide([&](int j) {  // keys of >= 3.76 s: the decoded moments (rare)
            const int64_t s = (uint32_t)__builtin_amdgcn_readlane((int)sid, j);
            const uint32_t* p;
            segs.get(s, p, n);
            wide_moments(p, n, s, out);
        });
    }
}

template <int PL>
void launch_list_full(const RaggedSegs& segs, const uint32_t* list, const uint32_t* cls,
                      const nvrx_stats_soa& out, hipStream_t st) {
    const unsigned blocks = (unsigned)(cu_count() * Occ<PL>::W);
    hipLaunchKernelGGL((seg_stats_list_full_kernel<PL>), dim3(blocks), dim3(256), 0, st, segs, list, cls, out);
}

template <int NMAX>
__global__ __launch_bounds__(256) void seg_stats_exact_list_kernel(RaggedSegs segs,
                                                                   const uint32_t* list,
                                                                   const uint32_t* cls,
                                                                   nvrx_stats_soa out) {
    const ColRef cr = ColRef::none();  // column references: kernel_ref afterwards
    __shared__ __attribute__((aligned(16))) float sbuf[NMAX];
    const uint32_t start = cls[0], cnt = cls[1];
    for (uint32_t i = blockIdx.x; i < cnt; i += gridDim.x) {
        const int64_t s = list[start + i];
        const uint32_t* p;
        int n;
        segs.get(s, p, n);
        exact_body<NMAX>(p, n, s, sbuf, out, cr);
    }
}

}  // namespace ragged

// per-class launches, each defined in the translation unit that instantiates its kernel
void ragged_launch_lane(int n, const RaggedSegs& segs, const uint32_t* list, const uint32_t* cls,
                        bool aligned16, const nvrx_stats_soa& out, hipStream_t st);
void ragged_launch_list(int pl, const RaggedSegs& segs, const uint32_t* list, const uint32_t* cls,
                        const nvrx_stats_soa& out, hipStream_t st);
void ragged_launch_full(int pl, const RaggedSegs& segs, const uint32_t* list, const uint32_t* cls,
                        const nvrx_stats_soa& out, hipStream_t st);
hipError_t ragged_launch_exact(const RaggedSegs& segs, const uint32_t* list, const uint32_t* cls,
                               int64_t max_len, const nvrx_stats_soa& out,
                               hipStream_t st);

}  // namespace nvrx
