// Test-only code object (not product code): the product's length-class rule
// (nvrx::ragged::seg_class, segment_ragged_kernels.h -- what the classifier of
// segment_ragged.hip sorts every ragged segment by) tabulated for tests/_ragged_model.py:
// table[((aligned16 * 2 + exact) * NFULL + f) * nmax + (n - 1)] = seg_class(n, aligned16, exact,
// full_n[f]) for n = 1..nmax.
#include "segment_ragged_kernels.h"

extern "C" __global__ void nvrx_ragged_class_probe(unsigned char* table, int nmax) {
    constexpr int NFULL = 5;
    const int full_n[NFULL] = {0, 1024, 2048, 4096, 8192};
    const long long total = 4ll * NFULL * nmax;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int n = (int)(i % nmax) + 1;
        const int f = (int)(i / nmax % NFULL);
        const int ae = (int)(i / nmax / NFULL);
        table[i] = (unsigned char)nvrx::ragged::seg_class(n, (ae >> 1) != 0, (ae & 1) != 0, full_n[f]);
    }
}
