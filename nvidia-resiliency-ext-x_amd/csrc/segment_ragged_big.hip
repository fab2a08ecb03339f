// segment_ragged_big.hip -- the wave-per-segment class kernels of PL 64 / 128 and the
// workgroup-per-segment (EXACT) kernels of segment_ragged.hip, in their own translation unit
// (parallel build).
#include "segment_ragged_kernels.h"

namespace nvrx {
namespace ragged {

// rings longer than NVRX_LDS_SEGMENT: exact_global_body over a per-block slice of device scratch
__global__ __launch_bounds__(XG_THREADS) void seg_stats_exact_list_global_kernel(
    RaggedSegs segs, const uint32_t* list, const uint32_t* cls, float* work, int64_t np2,
    nvrx_stats_soa out) {
    const ColRef cr = ColRef::none();
    __shared__ __attribute__((aligned(16))) float lds[XG_CHUNK];
    const uint32_t start = cls[0], cnt = cls[1];
    for (uint32_t i = blockIdx.x; i < cnt; i += gridDim.x) {
        const int64_t s = list[start + i];
        const uint32_t* p;
        int n;
        segs.get(s, p, n);
        exact_global_body(p, n, s, work + (int64_t)blockIdx.x * np2, lds, out, cr);
    }
}

}  // namespace ragged

hipError_t ragged_launch_exact(const RaggedSegs& segs, const uint32_t* list, const uint32_t* cls,
                               int64_t max_len, const nvrx_stats_soa& out, hipStream_t st) {
    using namespace ragged;
    const unsigned cus = (unsigned)cu_count();
    if (max_len <= 1024)
        hipLaunchKernelGGL((seg_stats_exact_list_kernel<1024>), dim3(cus * 8), dim3(256), 0, st, segs,
                           list, cls, out);
    else if (max_len <= 8192)
        hipLaunchKernelGGL((seg_stats_exact_list_kernel<8192>), dim3(cus * 4), dim3(256), 0, st, segs,
                           list, cls, out);
    else if (max_len <= NVRX_LDS_SEGMENT)
        hipLaunchKernelGGL((seg_stats_exact_list_kernel<NVRX_LDS_SEGMENT>), dim3(cus), dim3(256), 0,
                           st, segs, list, cls, out);
    else if (max_len <= NVRX_MAX_SEGMENT) {
        const int64_t np2 = exact_global_np2(max_len), blocks = exact_global_blocks(np2, cus);
        void* work = nullptr;
        hipError_t e = scratch_alloc(&work, (size_t)(blocks * np2) * sizeof(float), st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(seg_stats_exact_list_global_kernel, dim3((unsigned)blocks), dim3(XG_THREADS),
                           0, st, segs, list, cls, (float*)work, np2, out);
        e = hipGetLastError();
        const hipError_t f = hipFreeAsync(work, st);
        return e != hipSuccess ? e : f;
    } else
        return hipErrorInvalidValue;
    return hipSuccess;
}

void ragged_launch_list_big(int pl, const RaggedSegs& segs, const uint32_t* list, const uint32_t* cls,
                            const nvrx_stats_soa& out, hipStream_t st) {
    using namespace ragged;
    if (pl == 64)
        launch_list<64>(segs, list, cls, out, st);
    else
        launch_list<128>(segs, list, cls, out, st);
}

}  // namespace nvrx
