// score_element.h -- one element's terms of the median scores, shared by the two attributions that
// explain them: attribution.hip (per rank, the kernels behind its score) and
// score_rank_attribution.hip (per kernel, the ranks that lose on it).  One copy, so that both
// compute the same bits: f64, every operation rounded separately (-ffp-contract=off).
#pragma once
#include <cstdint>

namespace nvrx {
namespace {

// One element's terms; false when the element is not taken (absent, filtered, no base, MED == 0,
// NaN loss).  zero_med reports an eligible element with MED == 0.
template <typename T>
__device__ __forceinline__ bool element_terms(bool eligible, int32_t nm, T mt, T av, double base,
                                              double& w, double& s, double& loss, bool& zero_med) {
    const double m = (double)mt;
    w = (double)nm * (double)av;
    s = base / m;
    loss = w * (1.0 - s);
    zero_med = eligible && m == 0.0;
    return eligible && m != 0.0 && loss == loss;
}

}  // namespace
}  // namespace nvrx
