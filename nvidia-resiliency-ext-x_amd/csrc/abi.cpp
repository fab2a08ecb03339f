// abi.cpp -- the stateless part of the extern "C" boundary of libnvrx_hip.so (declared in
// include/nvrx_straggler.h): statistics, quantiles, histograms, scoring, sections, records.
//
// Thin host glue: argument/shape checks on the host before any launch, HIP error -> status
// code + thread-local message.  The profiler handle that replaces the reference's
// nvrx_cupti_module.CuptiProfiler lives in profiler.cpp.  All arithmetic runs in the HIP
// kernels of segment_stats.hip, scores.hip, attribution.hip, segment_histogram.hip,
// histogram_scores.hip, histogram_history.hip, histogram_attribution.hip, segment_tail.hip,
// segment_tail_attribution.hip, segment_history.hip, segment_history_attribution.hip,
// segment_history_compact.hip, segment_history_compact_attribution.hip, history_age.hip,
// histogram_history_compact.hip and records.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "abi_util.h"
#include "history_age.h"

namespace {
thread_local std::string g_last_error;
}  // namespace

namespace nvrx {

void set_error(const std::string& msg) { g_last_error = msg; }

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
int hip_status(hipError_t e, const char* where) {
    if (e == hipSuccess) return NVRX_OK;
    return fail(e == hipErrorInvalidValue ? NVRX_ERR_INVALID : NVRX_ERR_HIP,
                std::string(where) + ": " + hipGetErrorString(e));
}

int check_permille(const char* fn, const int32_t* permille, int32_t nq) {
    if (nq < 1 || nq > NVRX_MAX_QUANTILES)
        return fail(NVRX_ERR_INVALID, std::string(fn) + ": nq must be in [1, NVRX_MAX_QUANTILES = 8]");
    if (!permille) return fail(NVRX_ERR_INVALID, std::string(fn) + ": null permille");
    for (int32_t j = 0; j < nq; ++j)
        if (permille[j] < 0 || permille[j] > 1000)
            return fail(NVRX_ERR_INVALID, std::string(fn) + ": permille[" + std::to_string(j) +
                                              "] outside [0, 1000]");
    return NVRX_OK;
}

}  // namespace nvrx

using nvrx::check_permille;
using nvrx::fail;
using nvrx::hip_status;
using nvrx::S;

namespace {

// The geometry of the six nvrx_segment_* entries, checked once per addressing: one message per
// argument, naming it, prefixed with the entry's name.  nseg_limit (a power of two) is the
// entry's own: nseg must be below it.  The retained length is what `cap` leaves of a segment.
int check_retained(const std::string& fn, const char* what, int64_t len, int64_t cap) {
    const int64_t keep = (cap > 0 && len > cap) ? cap : len;
    NVRX_CHECK_ARG(keep <= NVRX_MAX_SEGMENT,
                   fn + ": retained " + what + " longer than NVRX_MAX_SEGMENT (2^30)");
    return NVRX_OK;
}
std::string below_limit(int64_t nseg_limit) {
    return ": nseg must be below 2^" + std::to_string(63 - __builtin_clzll((uint64_t)nseg_limit));
}

int check_strided(const char* entry, const uint32_t* ns, int64_t nseg, int64_t nseg_limit,
                  int64_t seg_stride, int64_t seg_begin, int64_t seg_len, int64_t cap) {
    const std::string fn(entry);
    NVRX_CHECK_ARG(nseg >= 0, fn + ": negative nseg");
    NVRX_CHECK_ARG(seg_len >= 0, fn + ": negative seg_len");
    NVRX_CHECK_ARG(seg_begin >= 0, fn + ": negative seg_begin");
    NVRX_CHECK_ARG(seg_stride >= 0, fn + ": negative seg_stride");
    NVRX_CHECK_ARG(nseg < nseg_limit, fn + below_limit(nseg_limit));
    NVRX_CHECK_ARG(nseg == 0 || seg_len == 0 || ns, fn + ": null ns");
    NVRX_CHECK_ARG(nseg <= 1 || seg_stride >= seg_begin + seg_len,
                   fn + ": segments overlap (seg_stride < seg_begin + seg_len)");
    return check_retained(fn, "seg_len", seg_len, cap);
}

int check_ragged(const char* entry, const uint32_t* ns, const int64_t* seg_off, int64_t nseg,
                 int64_t nseg_limit, int64_t max_len, int64_t cap) {
    const std::string fn(entry);
    NVRX_CHECK_ARG(nseg >= 0, fn + ": negative nseg");
    NVRX_CHECK_ARG(max_len >= 0, fn + ": negative max_len");
    NVRX_CHECK_ARG(nseg < nseg_limit, fn + below_limit(nseg_limit));
    NVRX_CHECK_ARG(nseg == 0 || seg_off, fn + ": null seg_off");
    NVRX_CHECK_ARG(nseg == 0 || max_len == 0 || ns, fn + ": null ns");
    return check_retained(fn, "max_len", max_len, cap);
}

// R rows x K kernels of the three nvrx_histogram_* tail-score entries
int check_tail_shape(const char* entry, int64_t R, int64_t K) {
    const std::string fn(entry);
    const int64_t lim = ((int64_t)1 << 31) - 1;
    NVRX_CHECK_ARG(R >= 0, fn + ": negative R");
    NVRX_CHECK_ARG(K >= 0, fn + ": negative K");
    NVRX_CHECK_ARG(K <= lim / NVRX_HIST_BINS, fn + ": K * 240 must be below 2^31");
    NVRX_CHECK_ARG(R == 0 || K <= lim / R, fn + ": R * K must be below 2^31");
    return NVRX_OK;
}

// What the tail-score entries share beyond their shape, as templates over the entry's args
// struct.  Each holds the checks it replaces in their order and with their text; an entry calls
// them where those checks stood, between the checks that are its own.

// permille and hist_stride of an entry with a history
template <typename A>
int check_history_slots(const std::string& fn, const A* a) {
    NVRX_CHECK_ARG(a->permille >= 0 && a->permille <= 1000, fn + ": permille outside [0, 1000]");
    NVRX_CHECK_ARG(a->hist_stride >= 0, fn + ": negative hist_stride");
    NVRX_CHECK_ARG(a->hist_stride == 0 || a->hist_index || a->hist_stride >= a->K,
                   fn + ": hist_stride below K without hist_index");
    return NVRX_OK;
}
// mode, then the above: the request of an individual score
template <typename A>
int check_history_request(const std::string& fn, const A* a) {
    NVRX_CHECK_ARG(a->mode != 0 && !(a->mode & ~(NVRX_HTAIL_SCORE | NVRX_HTAIL_UPDATE)),
                   fn + ": mode must be NVRX_HTAIL_SCORE, NVRX_HTAIL_UPDATE or both");
    return check_history_slots(fn, a);
}
// the outputs of an individual score, non-empty shape: the five of SCORE present
template <typename A>
int check_history_outputs_set(const std::string& fn, const A* a) {
    if (!(a->mode & NVRX_HTAIL_SCORE)) return NVRX_OK;
    NVRX_CHECK_ARG(a->tail_ns, fn + ": null tail_ns");
    NVRX_CHECK_ARG(a->total_ns, fn + ": null total_ns");
    NVRX_CHECK_ARG(a->base_tail_ns, fn + ": null base_tail_ns");
    NVRX_CHECK_ARG(a->base_total_ns, fn + ": null base_total_ns");
    NVRX_CHECK_ARG(a->score, fn + ": null score");
    return NVRX_OK;
}
// ... and, against a compact history, UPDATE's folded present and no alias of those five
template <typename A>
int check_folded_set(const std::string& fn, const A* a) {
    if (!(a->mode & NVRX_HTAIL_UPDATE)) return NVRX_OK;
    NVRX_CHECK_ARG(a->folded, fn + ": null folded");
    if (a->mode & NVRX_HTAIL_SCORE) {
        const void* const outs[] = {a->tail_ns, a->total_ns, a->base_tail_ns, a->base_total_ns, a->score};
        for (const void* o : outs)
            NVRX_CHECK_ARG(o != (const void*)a->folded, fn + ": folded aliases another output");
    }
    return NVRX_OK;
}
// the alignment of the five (any shape)
template <typename A>
int check_history_outputs_aligned(const std::string& fn, const A* a) {
    if (!(a->mode & NVRX_HTAIL_SCORE)) return NVRX_OK;
    NVRX_CHECK_ARG(((uintptr_t)a->tail_ns & 7) == 0, fn + ": tail_ns not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->total_ns & 7) == 0, fn + ": total_ns not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->base_tail_ns & 7) == 0, fn + ": base_tail_ns not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->base_total_ns & 7) == 0, fn + ": base_total_ns not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->score & 7) == 0, fn + ": score not 8-byte aligned");
    return NVRX_OK;
}

// the outputs of a tail attribution: `top` first of all, the eight present for a non-empty shape,
// the alignment of the five 8-byte ones
template <typename A>
int check_attribution_top(const std::string& fn, const A* a) {
    NVRX_CHECK_ARG(a->top >= 1 && a->top <= NVRX_MAX_ATTRIBUTION,
                   fn + ": top must be in [1, NVRX_MAX_ATTRIBUTION = 16]");
    return NVRX_OK;
}
template <typename A>
int check_attribution_outputs_set(const std::string& fn, const A* a) {
    NVRX_CHECK_ARG(a->idx, fn + ": null idx");
    NVRX_CHECK_ARG(a->loss, fn + ": null loss");
    NVRX_CHECK_ARG(a->tail_ns, fn + ": null tail_ns");
    NVRX_CHECK_ARG(a->total_ns, fn + ": null total_ns");
    NVRX_CHECK_ARG(a->tail_calls, fn + ": null tail_calls");
    NVRX_CHECK_ARG(a->thr_bucket, fn + ": null thr_bucket");
    NVRX_CHECK_ARG(a->base_share, fn + ": null base_share");
    NVRX_CHECK_ARG(a->loss_all, fn + ": null loss_all");
    return NVRX_OK;
}
template <typename A>
int check_attribution_outputs_aligned(const std::string& fn, const A* a) {
    NVRX_CHECK_ARG(((uintptr_t)a->loss & 7) == 0, fn + ": loss not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->tail_ns & 7) == 0, fn + ": tail_ns not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->total_ns & 7) == 0, fn + ": total_ns not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->base_share & 7) == 0, fn + ": base_share not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->loss_all & 7) == 0, fn + ": loss_all not 8-byte aligned");
    return NVRX_OK;
}

// R rows x stride slots of a history on its own (aging, conversion); dense: 240 bins per slot
int check_slots_shape(const std::string& fn, int64_t R, int64_t stride, bool dense) {
    const int64_t lim = ((int64_t)1 << 31) - 1;
    NVRX_CHECK_ARG(R >= 0, fn + ": negative R");
    NVRX_CHECK_ARG(stride >= 0, fn + ": negative stride");
    if (dense) NVRX_CHECK_ARG(stride <= lim / NVRX_HIST_BINS, fn + ": stride * 240 must be below 2^31");
    NVRX_CHECK_ARG(R == 0 || stride <= lim / R, fn + ": R * stride must be below 2^31");
    return NVRX_OK;
}

bool all_columns(const nvrx_stats_soa* out) {
    return out && out->num && out->min && out->max && out->med && out->avg && out->std;
}

}  // namespace

extern "C" {

const char* nvrx_last_error(void) { return g_last_error.c_str(); }

uint32_t nvrx_duration_key(uint64_t ns) {
    if (ns < NVRX_KEY_WIDE) return (uint32_t)ns;
    const float f = (float)ns;  // u64 -> f32, round to nearest: CuptiProfiler.cpp:187's conversion
    uint32_t b;
    std::memcpy(&b, &f, sizeof b);
    return NVRX_KEY_WIDE + (b - NVRX_KEY_WIDE_F32BITS);
}
int nvrx_abi_version(void) { return NVRX_ABI_VERSION; }

int nvrx_encode_ns_u32(uint32_t* ns, int64_t n, void* stream) {
    NVRX_CHECK_ARG(n >= 0 && (n == 0 || ns), "nvrx_encode_ns_u32: bad args");
    return hip_status(nvrx::encode_ns_u32(ns, n, S(stream)), "nvrx_encode_ns_u32");
}

int nvrx_device_count(int* count) {
    NVRX_CHECK_ARG(count, "nvrx_device_count: null count");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e == hipErrorNoDevice) c = 0, e = hipSuccess;
    *count = c;
    return hip_status(e, "hipGetDeviceCount");
}

int nvrx_sync(void* stream) { return hip_status(hipStreamSynchronize(S(stream)), "nvrx_sync"); }

// ------------------------------------------------------------------ statistics
int nvrx_segment_stats_strided(const uint32_t* ns, int64_t nseg, int64_t seg_stride,
                               int64_t seg_begin, int64_t seg_len, int64_t cap, int32_t mode,
                               const nvrx_stats_soa* out, uint32_t* col_ref, int64_t ncols,
                               void* stream) {
    if (int rc = check_strided("nvrx_segment_stats_strided", ns, nseg, (int64_t)1 << 33, seg_stride,
                               seg_begin, seg_len, cap))
        return rc;
    NVRX_CHECK_ARG(all_columns(out), "nvrx_segment_stats_strided: null output array");
    NVRX_CHECK_ARG((mode & ~NVRX_STATS_COLREF_READY) == NVRX_STATS_FAST ||
                       (mode & ~NVRX_STATS_COLREF_READY) == NVRX_STATS_EXACT,
                   "nvrx_segment_stats_strided: unknown mode");
    NVRX_CHECK_ARG(!col_ref || (ncols > 0 && nseg % ncols == 0),
                   "nvrx_segment_stats_strided: col_ref needs ncols > 0 dividing nseg");
    return hip_status(nvrx::segment_stats_strided(ns, nseg, seg_stride, seg_begin, seg_len, cap,
                                                  mode, *out, col_ref, ncols, S(stream)),
                      "nvrx_segment_stats_strided");
}

int nvrx_segment_stats_ragged(const uint32_t* ns, const int64_t* seg_off, const int32_t* seg_len,
                              int64_t nseg, int64_t max_len, int64_t cap, int32_t mode,
                              int32_t aligned16, const nvrx_stats_soa* out, uint32_t* col_ref,
                              int64_t ncols, void* stream) {
    if (int rc = check_ragged("nvrx_segment_stats_ragged", ns, seg_off, nseg, (int64_t)1 << 31,
                              max_len, cap))
        return rc;
    // this entry has always wanted ns for any segment, also when max_len == 0
    NVRX_CHECK_ARG(nseg == 0 || ns, "nvrx_segment_stats_ragged: null ns");
    NVRX_CHECK_ARG(all_columns(out), "nvrx_segment_stats_ragged: null output array");
    NVRX_CHECK_ARG(mode == NVRX_STATS_FAST || mode == NVRX_STATS_EXACT,
                   "nvrx_segment_stats_ragged: unknown mode");
    NVRX_CHECK_ARG(!col_ref || (ncols > 0 && nseg % ncols == 0),
                   "nvrx_segment_stats_ragged: col_ref needs ncols > 0 dividing nseg");
    return hip_status(nvrx::segment_stats_ragged(ns, seg_off, seg_len, nseg, max_len, cap, mode,
                                                 aligned16 != 0, *out, col_ref, ncols, S(stream)),
                      "nvrx_segment_stats_ragged");
}

// ------------------------------------------------------------------ quantiles
int nvrx_segment_quantiles_strided(const uint32_t* ns, int64_t nseg, int64_t seg_stride,
                                   int64_t seg_begin, int64_t seg_len, int64_t cap,
                                   const int32_t* permille, int32_t nq, float* out, int32_t* num,
                                   void* stream) {
    if (int rc = check_permille("nvrx_segment_quantiles_strided", permille, nq)) return rc;
    if (int rc = check_strided("nvrx_segment_quantiles_strided", ns, nseg, (int64_t)1 << 31,
                               seg_stride, seg_begin, seg_len, cap))
        return rc;
    NVRX_CHECK_ARG(nseg == 0 || out, "nvrx_segment_quantiles_strided: null out");
    if (nseg == 0) return NVRX_OK;
    return hip_status(nvrx::segment_quantiles_strided(ns, nseg, seg_stride, seg_begin, seg_len, cap,
                                                      permille, nq, out, num, S(stream)),
                      "nvrx_segment_quantiles_strided");
}

int nvrx_segment_quantiles_ragged(const uint32_t* ns, const int64_t* seg_off,
                                  const int32_t* seg_len, int64_t nseg, int64_t max_len,
                                  int64_t cap, int32_t aligned16, const int32_t* permille,
                                  int32_t nq, float* out, int32_t* num, void* stream) {
    if (int rc = check_permille("nvrx_segment_quantiles_ragged", permille, nq)) return rc;
    if (int rc = check_ragged("nvrx_segment_quantiles_ragged", ns, seg_off, nseg, (int64_t)1 << 31,
                              max_len, cap))
        return rc;
    NVRX_CHECK_ARG(nseg == 0 || out, "nvrx_segment_quantiles_ragged: null out");
    if (nseg == 0) return NVRX_OK;
    return hip_status(nvrx::segment_quantiles_ragged(ns, seg_off, seg_len, nseg, max_len, cap,
                                                     aligned16 != 0, permille, nq, out, num, S(stream)),
                      "nvrx_segment_quantiles_ragged");
}

// ------------------------------------------------------------------ histograms
uint32_t nvrx_histogram_bucket(uint32_t key) {
    if (key < 8) return key;
    const int e = 31 - __builtin_clz(key);
    return (uint32_t)(8 * (e - 2)) + ((key >> (e - 3)) & 7u);
}

uint64_t nvrx_histogram_edge(int32_t bucket) {
    if (bucket < 0 || bucket > NVRX_HIST_BINS) return UINT64_MAX;
    if (bucket < 8) return (uint64_t)bucket;
    return (uint64_t)(8 + bucket % 8) << (bucket / 8 - 1);
}

int nvrx_segment_histogram_strided(const uint32_t* ns, int64_t nseg, int64_t seg_stride,
                                   int64_t seg_begin, int64_t seg_len, int64_t cap,
                                   int32_t accumulate, uint32_t* counts, int32_t* num, void* stream) {
    if (int rc = check_strided("nvrx_segment_histogram_strided", ns, nseg, (int64_t)1 << 31,
                               seg_stride, seg_begin, seg_len, cap))
        return rc;
    NVRX_CHECK_ARG(nseg == 0 || counts, "nvrx_segment_histogram_strided: null counts");
    NVRX_CHECK_ARG(((uintptr_t)counts & 15) == 0, "nvrx_segment_histogram_strided: counts not 16-byte aligned");
    if (nseg == 0) return NVRX_OK;
    return hip_status(nvrx::segment_histogram_strided(ns, nseg, seg_stride, seg_begin, seg_len, cap,
                                                      accumulate != 0, counts, num, S(stream)),
                      "nvrx_segment_histogram_strided");
}

int nvrx_segment_histogram_ragged(const uint32_t* ns, const int64_t* seg_off,
                                  const int32_t* seg_len, int64_t nseg, int64_t max_len,
                                  int64_t cap, int32_t aligned16, int32_t accumulate,
                                  uint32_t* counts, int32_t* num, void* stream) {
    if (int rc = check_ragged("nvrx_segment_histogram_ragged", ns, seg_off, nseg, (int64_t)1 << 31,
                              max_len, cap))
        return rc;
    NVRX_CHECK_ARG(nseg == 0 || counts, "nvrx_segment_histogram_ragged: null counts");
    NVRX_CHECK_ARG(((uintptr_t)counts & 15) == 0, "nvrx_segment_histogram_ragged: counts not 16-byte aligned");
    if (nseg == 0) return NVRX_OK;
    return hip_status(nvrx::segment_histogram_ragged(ns, seg_off, seg_len, nseg, max_len, cap,
                                                     aligned16 != 0, accumulate != 0, counts, num,
                                                     S(stream)),
                      "nvrx_segment_histogram_ragged");
}

// ------------------------------------------------------------------ tail scores
int nvrx_histogram_sum(const uint32_t* counts, int64_t R, int64_t K, int32_t accumulate,
                       uint64_t* fleet, void* stream) {
    if (int rc = check_tail_shape("nvrx_histogram_sum", R, K)) return rc;
    if (R > 0 && K > 0) {
        NVRX_CHECK_ARG(counts, "nvrx_histogram_sum: null counts");
        NVRX_CHECK_ARG(fleet, "nvrx_histogram_sum: null fleet");
    }
    NVRX_CHECK_ARG(((uintptr_t)counts & 15) == 0, "nvrx_histogram_sum: counts not 16-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)fleet & 15) == 0, "nvrx_histogram_sum: fleet not 16-byte aligned");
    return hip_status(nvrx::histogram_sum(counts, R, K, accumulate != 0, fleet, S(stream)),
                      "nvrx_histogram_sum");
}

int nvrx_histogram_tail_threshold(const uint64_t* fleet, int64_t K, int32_t permille,
                                  const uint8_t* col_valid, int32_t* thr, uint64_t* fleet_sums,
                                  void* stream) {
    if (int rc = check_tail_shape("nvrx_histogram_tail_threshold", 0, K)) return rc;
    NVRX_CHECK_ARG(permille >= 0 && permille <= 1000,
                   "nvrx_histogram_tail_threshold: permille outside [0, 1000]");
    if (K > 0) {
        NVRX_CHECK_ARG(fleet, "nvrx_histogram_tail_threshold: null fleet");
        NVRX_CHECK_ARG(thr, "nvrx_histogram_tail_threshold: null thr");
        NVRX_CHECK_ARG(fleet_sums, "nvrx_histogram_tail_threshold: null fleet_sums");
    }
    NVRX_CHECK_ARG(((uintptr_t)fleet & 15) == 0,
                   "nvrx_histogram_tail_threshold: fleet not 16-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)fleet_sums & 7) == 0,
                   "nvrx_histogram_tail_threshold: fleet_sums not 8-byte aligned");
    return hip_status(nvrx::histogram_tail_threshold(fleet, K, permille, col_valid, thr, fleet_sums,
                                                     S(stream)),
                      "nvrx_histogram_tail_threshold");
}

int nvrx_histogram_tail_scores(const nvrx_tail_args* a, void* stream) {
    NVRX_CHECK_ARG(a, "nvrx_histogram_tail_scores: null args");
    if (int rc = check_tail_shape("nvrx_histogram_tail_scores", a->R, a->K)) return rc;
    if (a->R > 0 && a->K > 0) {
        NVRX_CHECK_ARG(a->counts, "nvrx_histogram_tail_scores: null counts");
        NVRX_CHECK_ARG(a->thr, "nvrx_histogram_tail_scores: null thr");
        NVRX_CHECK_ARG(a->fleet_sums, "nvrx_histogram_tail_scores: null fleet_sums");
        NVRX_CHECK_ARG(a->tail_ns, "nvrx_histogram_tail_scores: null tail_ns");
        NVRX_CHECK_ARG(a->total_ns, "nvrx_histogram_tail_scores: null total_ns");
        NVRX_CHECK_ARG(a->score, "nvrx_histogram_tail_scores: null score");
    }
    NVRX_CHECK_ARG(((uintptr_t)a->counts & 15) == 0,
                   "nvrx_histogram_tail_scores: counts not 16-byte aligned");
    return hip_status(nvrx::histogram_tail_scores(*a, S(stream)), "nvrx_histogram_tail_scores");
}

int nvrx_histogram_history_scores(const nvrx_histtail_args* a, void* stream) {
    const std::string fn("nvrx_histogram_history_scores");
    NVRX_CHECK_ARG(a, fn + ": null args");
    if (int rc = check_tail_shape(fn.c_str(), a->R, a->K)) return rc;
    if (int rc = check_history_request(fn, a)) return rc;
    if (a->R > 0 && a->K > 0) {
        NVRX_CHECK_ARG(a->counts, fn + ": null counts");
        NVRX_CHECK_ARG(a->hist, fn + ": null hist");
        if (int rc = check_history_outputs_set(fn, a)) return rc;
    }
    NVRX_CHECK_ARG(((uintptr_t)a->counts & 15) == 0, fn + ": counts not 16-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->hist & 15) == 0, fn + ": hist not 16-byte aligned");
    if (a->mode & NVRX_HTAIL_SCORE)
        NVRX_CHECK_ARG((((uintptr_t)a->tail_ns | (uintptr_t)a->total_ns | (uintptr_t)a->base_tail_ns |
                         (uintptr_t)a->base_total_ns) & 7) == 0,
                       fn + ": the u64 outputs are not 8-byte aligned");
    return hip_status(nvrx::histogram_history_scores(*a, S(stream)), fn.c_str());
}

int nvrx_histogram_tail_base(const uint64_t* fleet, int64_t K, const int32_t* thr, uint64_t* base,
                             void* stream) {
    if (int rc = check_tail_shape("nvrx_histogram_tail_base", 0, K)) return rc;
    if (K > 0) {
        NVRX_CHECK_ARG(fleet, "nvrx_histogram_tail_base: null fleet");
        NVRX_CHECK_ARG(thr, "nvrx_histogram_tail_base: null thr");
        NVRX_CHECK_ARG(base, "nvrx_histogram_tail_base: null base");
    }
    NVRX_CHECK_ARG(((uintptr_t)fleet & 15) == 0, "nvrx_histogram_tail_base: fleet not 16-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)base & 15) == 0, "nvrx_histogram_tail_base: base not 16-byte aligned");
    return hip_status(nvrx::histogram_tail_base(fleet, K, thr, base, S(stream)),
                      "nvrx_histogram_tail_base");
}

int nvrx_histogram_tail_attribution(const nvrx_tailattr_args* a, void* stream) {
    const std::string fn("nvrx_histogram_tail_attribution");
    NVRX_CHECK_ARG(a, fn + ": null args");
    if (int rc = check_attribution_top(fn, a)) return rc;
    NVRX_CHECK_ARG(a->kind == NVRX_ATTR_RELATIVE || a->kind == NVRX_ATTR_INDIVIDUAL,
                   fn + ": unknown kind (NVRX_ATTR_RELATIVE or NVRX_ATTR_INDIVIDUAL)");
    if (int rc = check_tail_shape(fn.c_str(), a->R, a->K)) return rc;
    const bool ind = a->kind == NVRX_ATTR_INDIVIDUAL;
    if (ind) {
        if (int rc = check_history_slots(fn, a)) return rc;
    }
    if (a->R > 0 && a->K > 0) {
        NVRX_CHECK_ARG(a->counts, fn + ": null counts");
        NVRX_CHECK_ARG(ind || a->thr, fn + ": the relative kind needs thr");
        NVRX_CHECK_ARG(ind || a->base, fn + ": the relative kind needs base");
        NVRX_CHECK_ARG(!ind || a->hist, fn + ": the individual kind needs hist");
        if (int rc = check_attribution_outputs_set(fn, a)) return rc;
    }
    NVRX_CHECK_ARG(((uintptr_t)a->counts & 15) == 0, fn + ": counts not 16-byte aligned");
    NVRX_CHECK_ARG(!ind || ((uintptr_t)a->hist & 15) == 0, fn + ": hist not 16-byte aligned");
    NVRX_CHECK_ARG(ind || ((uintptr_t)a->base & 7) == 0, fn + ": base not 8-byte aligned");
    NVRX_CHECK_ARG((((uintptr_t)a->loss | (uintptr_t)a->tail_ns | (uintptr_t)a->total_ns |
                     (uintptr_t)a->base_share | (uintptr_t)a->loss_all) & 7) == 0,
                   fn + ": the 8-byte outputs are not 8-byte aligned");
    return hip_status(nvrx::histogram_tail_attribution(*a, S(stream)), fn.c_str());
}

// tail scores straight from ragged segments (segment_tail.hip).  aligned16 is part of the
// addressing the entries share with nvrx_segment_histogram_ragged; these kernels read by sample
// and are correct for either value.
int nvrx_segment_fleet_histogram_ragged(const uint32_t* ns, const int64_t* seg_off,
                                        const int32_t* seg_len, int64_t R, int64_t K,
                                        int64_t max_len, int64_t cap, int32_t aligned16,
                                        int32_t accumulate, uint64_t* fleet, void* stream) {
    const char* fn = "nvrx_segment_fleet_histogram_ragged";
    (void)aligned16;
    if (int rc = check_tail_shape(fn, R, K)) return rc;
    if (int rc = check_ragged(fn, ns, seg_off, R * K, (int64_t)1 << 31, max_len, cap)) return rc;
    NVRX_CHECK_ARG(R == 0 || K == 0 || fleet, std::string(fn) + ": null fleet");
    NVRX_CHECK_ARG(((uintptr_t)seg_off & 7) == 0, std::string(fn) + ": seg_off not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)fleet & 15) == 0, std::string(fn) + ": fleet not 16-byte aligned");
    return hip_status(nvrx::segment_fleet_histogram_ragged(ns, seg_off, seg_len, R, K, max_len, cap,
                                                           accumulate != 0, fleet, S(stream)),
                      fn);
}

int nvrx_segment_tail_scores_ragged(const nvrx_segtail_args* a, void* stream) {
    const std::string fn("nvrx_segment_tail_scores_ragged");
    NVRX_CHECK_ARG(a, fn + ": null args");
    if (int rc = check_tail_shape(fn.c_str(), a->R, a->K)) return rc;
    if (int rc = check_ragged(fn.c_str(), a->ns, a->seg_off, a->R * a->K, (int64_t)1 << 31,
                              a->max_len, a->cap))
        return rc;
    if (a->R > 0 && a->K > 0) {
        NVRX_CHECK_ARG(a->thr, fn + ": null thr");
        NVRX_CHECK_ARG(a->fleet_sums, fn + ": null fleet_sums");
        NVRX_CHECK_ARG(a->tail_ns, fn + ": null tail_ns");
        NVRX_CHECK_ARG(a->total_ns, fn + ": null total_ns");
        NVRX_CHECK_ARG(a->score, fn + ": null score");
    }
    NVRX_CHECK_ARG(((uintptr_t)a->seg_off & 7) == 0, fn + ": seg_off not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->fleet_sums & 7) == 0, fn + ": fleet_sums not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->tail_ns & 7) == 0, fn + ": tail_ns not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->total_ns & 7) == 0, fn + ": total_ns not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->score & 7) == 0, fn + ": score not 8-byte aligned");
    return hip_status(nvrx::segment_tail_scores_ragged(*a, S(stream)), fn.c_str());
}

// the relative tail score attribution straight from those segments (segment_tail_attribution.hip)
int nvrx_segment_tail_attribution_ragged(const nvrx_segtailattr_args* a, void* stream) {
    const std::string fn("nvrx_segment_tail_attribution_ragged");
    NVRX_CHECK_ARG(a, fn + ": null args");
    if (int rc = check_attribution_top(fn, a)) return rc;
    if (int rc = check_tail_shape(fn.c_str(), a->R, a->K)) return rc;
    if (int rc = check_ragged(fn.c_str(), a->ns, a->seg_off, a->R * a->K, (int64_t)1 << 31,
                              a->max_len, a->cap))
        return rc;
    if (a->R > 0 && a->K > 0) {
        NVRX_CHECK_ARG(a->thr, fn + ": null thr");
        NVRX_CHECK_ARG(a->base, fn + ": null base");
        if (int rc = check_attribution_outputs_set(fn, a)) return rc;
    }
    NVRX_CHECK_ARG(((uintptr_t)a->seg_off & 7) == 0, fn + ": seg_off not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->base & 7) == 0, fn + ": base not 8-byte aligned");
    if (int rc = check_attribution_outputs_aligned(fn, a)) return rc;
    return hip_status(nvrx::segment_tail_attribution_ragged(*a, S(stream)), fn.c_str());
}

// the individual tail scores straight from those segments (segment_history.hip)
int nvrx_segment_history_scores_ragged(const nvrx_seghist_args* a, void* stream) {
    const std::string fn("nvrx_segment_history_scores_ragged");
    NVRX_CHECK_ARG(a, fn + ": null args");
    if (int rc = check_tail_shape(fn.c_str(), a->R, a->K)) return rc;
    if (int rc = check_ragged(fn.c_str(), a->ns, a->seg_off, a->R * a->K, (int64_t)1 << 31,
                              a->max_len, a->cap))
        return rc;
    if (int rc = check_history_request(fn, a)) return rc;
    const bool score = a->mode & NVRX_HTAIL_SCORE;
    if (a->R > 0 && a->K > 0) {
        NVRX_CHECK_ARG(a->hist, fn + ": null hist");
        if (int rc = check_history_outputs_set(fn, a)) return rc;
    }
    NVRX_CHECK_ARG(((uintptr_t)a->seg_off & 7) == 0, fn + ": seg_off not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->hist & 15) == 0, fn + ": hist not 16-byte aligned");
    if (int rc = check_history_outputs_aligned(fn, a)) return rc;
    nvrx_seghist_args b = *a;
    if (!score) b.tail_calls = nullptr;  // ignored without SCORE
    return hip_status(nvrx::segment_history_scores_ragged(b, S(stream)), fn.c_str());
}

// the same scores against a compact history of 64 B per element (segment_history_compact.hip)
int nvrx_segment_history_scores_compact_ragged(const nvrx_segchist_args* a, void* stream) {
    const std::string fn("nvrx_segment_history_scores_compact_ragged");
    NVRX_CHECK_ARG(a, fn + ": null args");
    if (int rc = check_tail_shape(fn.c_str(), a->R, a->K)) return rc;
    if (int rc = check_ragged(fn.c_str(), a->ns, a->seg_off, a->R * a->K, (int64_t)1 << 31,
                              a->max_len, a->cap))
        return rc;
    if (int rc = check_history_request(fn, a)) return rc;
    const bool score = a->mode & NVRX_HTAIL_SCORE, update = a->mode & NVRX_HTAIL_UPDATE;
    if (a->R > 0 && a->K > 0) {
        NVRX_CHECK_ARG(a->chist, fn + ": null chist");
        if (int rc = check_history_outputs_set(fn, a)) return rc;
        if (int rc = check_folded_set(fn, a)) return rc;
    }
    NVRX_CHECK_ARG(((uintptr_t)a->seg_off & 7) == 0, fn + ": seg_off not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->chist & 15) == 0, fn + ": chist not 16-byte aligned");
    if (int rc = check_history_outputs_aligned(fn, a)) return rc;
    if (update) NVRX_CHECK_ARG(((uintptr_t)a->folded & 7) == 0, fn + ": folded not 8-byte aligned");
    nvrx_segchist_args b = *a;
    if (!score) b.tail_calls = nullptr;  // ignored without SCORE
    if (!update) b.folded = nullptr;     // not written without UPDATE
    return hip_status(nvrx::segment_history_scores_compact_ragged(b, S(stream)), fn.c_str());
}

// the individual tail score attribution straight from those segments
// (segment_history_attribution.hip)
int nvrx_segment_history_attribution_ragged(const nvrx_seghistattr_args* a, void* stream) {
    const std::string fn("nvrx_segment_history_attribution_ragged");
    NVRX_CHECK_ARG(a, fn + ": null args");
    if (int rc = check_attribution_top(fn, a)) return rc;
    if (int rc = check_tail_shape(fn.c_str(), a->R, a->K)) return rc;
    if (int rc = check_ragged(fn.c_str(), a->ns, a->seg_off, a->R * a->K, (int64_t)1 << 31,
                              a->max_len, a->cap))
        return rc;
    if (int rc = check_history_slots(fn, a)) return rc;
    if (a->R > 0 && a->K > 0) {
        NVRX_CHECK_ARG(a->hist, fn + ": null hist");
        if (int rc = check_attribution_outputs_set(fn, a)) return rc;
    }
    NVRX_CHECK_ARG(((uintptr_t)a->seg_off & 7) == 0, fn + ": seg_off not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->hist & 15) == 0, fn + ": hist not 16-byte aligned");
    if (int rc = check_attribution_outputs_aligned(fn, a)) return rc;
    return hip_status(nvrx::segment_history_attribution_ragged(*a, S(stream)), fn.c_str());
}

// the same attribution against the compact history (segment_history_compact_attribution.hip):
// the checks above without the K * 240 limit, which belongs to the dense history
int nvrx_segment_history_attribution_compact_ragged(const nvrx_segchistattr_args* a, void* stream) {
    const std::string fn("nvrx_segment_history_attribution_compact_ragged");
    NVRX_CHECK_ARG(a, fn + ": null args");
    if (int rc = check_attribution_top(fn, a)) return rc;
    NVRX_CHECK_ARG(a->R >= 0, fn + ": negative R");
    NVRX_CHECK_ARG(a->K >= 0, fn + ": negative K");
    NVRX_CHECK_ARG(a->R == 0 || a->K <= (((int64_t)1 << 31) - 1) / a->R,
                   fn + ": R * K must be below 2^31");
    if (int rc = check_ragged(fn.c_str(), a->ns, a->seg_off, a->R * a->K, (int64_t)1 << 31,
                              a->max_len, a->cap))
        return rc;
    if (int rc = check_history_slots(fn, a)) return rc;
    if (a->R > 0 && a->K > 0) {
        NVRX_CHECK_ARG(a->chist, fn + ": null chist");
        if (int rc = check_attribution_outputs_set(fn, a)) return rc;
    }
    NVRX_CHECK_ARG(((uintptr_t)a->seg_off & 7) == 0, fn + ": seg_off not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->chist & 15) == 0, fn + ": chist not 16-byte aligned");
    if (int rc = check_attribution_outputs_aligned(fn, a)) return rc;
    return hip_status(nvrx::segment_history_attribution_compact_ragged(*a, S(stream)), fn.c_str());
}

// aging of the tail histories (history_age.hip): slots, not columns
int nvrx_compact_history_age(void* chist, int64_t R, int64_t stride, int32_t shift,
                             uint64_t* evicted, uint64_t* full, void* stream) {
    const std::string fn("nvrx_compact_history_age");
    if (int rc = check_slots_shape(fn, R, stride, false)) return rc;
    NVRX_CHECK_ARG(shift >= 1 && shift <= 31, fn + ": shift outside [1, 31]");
    if (R > 0 && stride > 0) NVRX_CHECK_ARG(chist, fn + ": null chist");
    NVRX_CHECK_ARG(((uintptr_t)chist & 15) == 0, fn + ": chist not 16-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)evicted & 7) == 0, fn + ": evicted not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)full & 7) == 0, fn + ": full not 8-byte aligned");
    NVRX_CHECK_ARG(!evicted || evicted != full, fn + ": full aliases evicted");
    return hip_status(nvrx::compact_history_age(chist, R, stride, shift, evicted, full, S(stream)),
                      fn.c_str());
}

int nvrx_histogram_history_age(uint32_t* hist, int64_t R, int64_t stride, int32_t shift, void* stream) {
    const std::string fn("nvrx_histogram_history_age");
    const int64_t lim = ((int64_t)1 << 31) - 1;
    if (int rc = check_slots_shape(fn, R, stride, true)) return rc;
    // the pass indexes 16-byte vectors, 60 per histogram
    NVRX_CHECK_ARG(R == 0 || stride == 0 || R * stride <= lim / (NVRX_HIST_BINS / 4),
                   fn + ": R * stride * 240 must be below 2^31 vectors of four words");
    NVRX_CHECK_ARG(shift >= 1 && shift <= 31, fn + ": shift outside [1, 31]");
    if (R > 0 && stride > 0) NVRX_CHECK_ARG(hist, fn + ": null hist");
    NVRX_CHECK_ARG(((uintptr_t)hist & 15) == 0, fn + ": hist not 16-byte aligned");
    return hip_status(nvrx::histogram_history_age(hist, R, stride, shift, S(stream)), fn.c_str());
}

// individual tail scores from counts against the compact history (histogram_history_compact.hip):
// the checks of nvrx_histogram_history_scores and of nvrx_segment_history_scores_compact_ragged
int nvrx_histogram_history_scores_compact(const nvrx_histchist_args* a, void* stream) {
    const std::string fn("nvrx_histogram_history_scores_compact");
    NVRX_CHECK_ARG(a, fn + ": null args");
    if (int rc = check_tail_shape(fn.c_str(), a->R, a->K)) return rc;
    if (int rc = check_history_request(fn, a)) return rc;
    const bool score = a->mode & NVRX_HTAIL_SCORE, update = a->mode & NVRX_HTAIL_UPDATE;
    if (a->R > 0 && a->K > 0) {
        NVRX_CHECK_ARG(a->counts, fn + ": null counts");
        NVRX_CHECK_ARG(a->chist, fn + ": null chist");
        if (int rc = check_history_outputs_set(fn, a)) return rc;
        if (int rc = check_folded_set(fn, a)) return rc;
    }
    NVRX_CHECK_ARG(((uintptr_t)a->counts & 15) == 0, fn + ": counts not 16-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->chist & 15) == 0, fn + ": chist not 16-byte aligned");
    if (int rc = check_history_outputs_aligned(fn, a)) return rc;
    if (update) NVRX_CHECK_ARG(((uintptr_t)a->folded & 7) == 0, fn + ": folded not 8-byte aligned");
    nvrx_histchist_args b = *a;
    if (!score) b.tail_calls = nullptr;  // ignored without SCORE
    if (!update) b.folded = nullptr;     // not written without UPDATE
    return hip_status(nvrx::histogram_history_scores_compact(b, S(stream)), fn.c_str());
}

// the attribution of counts against the compact history (histogram_history_compact_attribution.hip):
// the checks of the individual kind of nvrx_histogram_tail_attribution, with chist for hist
int nvrx_histogram_history_attribution_compact(const nvrx_histchistattr_args* a, void* stream) {
    const std::string fn("nvrx_histogram_history_attribution_compact");
    NVRX_CHECK_ARG(a, fn + ": null args");
    if (int rc = check_attribution_top(fn, a)) return rc;
    if (int rc = check_tail_shape(fn.c_str(), a->R, a->K)) return rc;
    if (int rc = check_history_slots(fn, a)) return rc;
    if (a->R > 0 && a->K > 0) {
        NVRX_CHECK_ARG(a->counts, fn + ": null counts");
        NVRX_CHECK_ARG(a->chist, fn + ": null chist");
        if (int rc = check_attribution_outputs_set(fn, a)) return rc;
    }
    NVRX_CHECK_ARG(((uintptr_t)a->counts & 15) == 0, fn + ": counts not 16-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->chist & 15) == 0, fn + ": chist not 16-byte aligned");
    if (int rc = check_attribution_outputs_aligned(fn, a)) return rc;
    return hip_status(nvrx::histogram_history_attribution_compact(*a, S(stream)), fn.c_str());
}

// the ranks behind a kernel's tail loss (rank_attribution.hip): the plan is pure host code
static int check_rank_request(const std::string& fn, int64_t R, int64_t K, int32_t top) {
    NVRX_CHECK_ARG(R >= 0, fn + ": negative R");
    NVRX_CHECK_ARG(K >= 0, fn + ": negative K");
    NVRX_CHECK_ARG(top >= 1 && top <= NVRX_MAX_ATTRIBUTION,
                   fn + ": top must be in [1, NVRX_MAX_ATTRIBUTION = 16]");
    return NVRX_OK;
}

int nvrx_rank_attribution_plan(int64_t R, int64_t K, int32_t top, int64_t* tiles, int64_t* splits,
                               int64_t* work_bytes) {
    if (int rc = check_rank_request("nvrx_rank_attribution_plan", R, K, top)) return rc;
    nvrx::rank_attribution_plan(R, K, top, tiles, splits, work_bytes);
    return NVRX_OK;
}

int nvrx_rank_attribution(const nvrx_rankattr_args* a, void* stream) {
    const std::string fn("nvrx_rank_attribution");
    const int64_t lim = ((int64_t)1 << 31) - 1;
    NVRX_CHECK_ARG(a, fn + ": null args");
    if (int rc = check_rank_request(fn, a->R, a->K, a->top)) return rc;
    NVRX_CHECK_ARG(a->ld == 0 || a->ld >= a->K, fn + ": ld below K");
    const int64_t ld = a->ld ? a->ld : a->K;
    NVRX_CHECK_ARG(a->R == 0 || ld <= lim / a->R, fn + ": R * ld must be below 2^31");
    if (a->R > 0 && a->K > 0) {
        int64_t work_bytes = 0;
        nvrx::rank_attribution_plan(a->R, a->K, a->top, nullptr, nullptr, &work_bytes);
        NVRX_CHECK_ARG(a->loss, fn + ": null loss");
        NVRX_CHECK_ARG(a->idx, fn + ": null idx");
        NVRX_CHECK_ARG(a->loss_out, fn + ": null loss_out");
        NVRX_CHECK_ARG(a->taken, fn + ": null taken");
        NVRX_CHECK_ARG(a->positive, fn + ": null positive");
        NVRX_CHECK_ARG(work_bytes == 0 || a->work, fn + ": null work (the plan needs work_bytes)");
    }
    NVRX_CHECK_ARG(((uintptr_t)a->loss & 7) == 0, fn + ": loss not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->loss_out & 7) == 0, fn + ": loss_out not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->work & 7) == 0, fn + ": work not 8-byte aligned");
    return hip_status(nvrx::rank_attribution(*a, S(stream)), fn.c_str());
}

// the conversion between the two histories (histogram_history_compact.hip): slots, not columns
static int check_convert(const std::string& fn, const void* hist, const void* chist, int64_t R,
                         int64_t stride) {
    if (int rc = check_slots_shape(fn, R, stride, true)) return rc;
    if (R > 0 && stride > 0) {
        NVRX_CHECK_ARG(hist, fn + ": null hist");
        NVRX_CHECK_ARG(chist, fn + ": null chist");
    }
    NVRX_CHECK_ARG(((uintptr_t)hist & 15) == 0, fn + ": hist not 16-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)chist & 15) == 0, fn + ": chist not 16-byte aligned");
    return NVRX_OK;
}

int nvrx_compact_history_from_dense(const uint32_t* hist, void* chist, int64_t R, int64_t stride,
                                    uint64_t* folded, void* stream) {
    const std::string fn("nvrx_compact_history_from_dense");
    if (int rc = check_convert(fn, hist, chist, R, stride)) return rc;
    NVRX_CHECK_ARG(((uintptr_t)folded & 7) == 0, fn + ": folded not 8-byte aligned");
    return hip_status(nvrx::compact_history_from_dense(hist, chist, R, stride, folded, S(stream)),
                      fn.c_str());
}

int nvrx_compact_history_to_dense(const void* chist, uint32_t* hist, int64_t R, int64_t stride,
                                  void* stream) {
    const std::string fn("nvrx_compact_history_to_dense");
    if (int rc = check_convert(fn, hist, chist, R, stride)) return rc;
    return hip_status(nvrx::compact_history_to_dense(chist, hist, R, stride, S(stream)), fn.c_str());
}

// ------------------------------------------------------------------ scoring
int nvrx_kernel_ref(const int32_t* num, const float* med, int64_t R, int64_t K, float* ref,
                    uint32_t* scratch, void* stream) {
    NVRX_CHECK_ARG(R >= 0 && K >= 0, "nvrx_kernel_ref: negative size");
    NVRX_CHECK_ARG(K == 0 || (ref && scratch), "nvrx_kernel_ref: null ref/scratch");
    NVRX_CHECK_ARG(R == 0 || K == 0 || (num && med), "nvrx_kernel_ref: null num/med");
    NVRX_CHECK_ARG(R <= NVRX_KREF_MAX_R, "nvrx_kernel_ref: too many rows");
    return hip_status(nvrx::kernel_ref(num, med, R, K, ref, scratch, S(stream)), "nvrx_kernel_ref");
}

int nvrx_pack_min_times(const double* med, const int32_t* ids, int64_t n, float* times,
                        int64_t total, void* stream) {
    NVRX_CHECK_ARG(n >= 0 && total >= 0, "nvrx_pack_min_times: negative size");
    NVRX_CHECK_ARG(total == 0 || times, "nvrx_pack_min_times: null times");
    NVRX_CHECK_ARG(n == 0 || (med && ids), "nvrx_pack_min_times: null inputs");
    NVRX_CHECK_ARG(n <= total, "nvrx_pack_min_times: n > total (more entries than the tensor holds)");
    return hip_status(nvrx::pack_min_times(med, ids, n, times, total, S(stream)),
                      "nvrx_pack_min_times");
}

int nvrx_scores(const nvrx_score_args* a, void* stream) {
    NVRX_CHECK_ARG(a, "nvrx_scores: null args");
    NVRX_CHECK_ARG(a->R >= 0 && a->K >= 0, "nvrx_scores: negative size");
    NVRX_CHECK_ARG(a->R == 0 || a->partials || a->gpu_rel || a->gpu_ind || a->strag_rel ||
                       a->strag_ind,
                   "nvrx_scores: no output (partials or finalized scores)");
    NVRX_CHECK_ARG(a->R == 0 || a->K == 0 || (a->num && a->med && a->avg),
                   "nvrx_scores: null num/med/avg");
    NVRX_CHECK_ARG(!a->hist_index || a->hist_stride > 0,
                   "nvrx_scores: hist_index requires hist_stride");
    NVRX_CHECK_ARG(a->value_f64 == 0 || a->value_f64 == 1, "nvrx_scores: bad value_f64");
    NVRX_CHECK_ARG(a->reset_ncols >= 0 && (a->reset_ncols == 0 || (a->reset_col_ref && a->done)),
                   "nvrx_scores: reset_col_ref needs done and reset_ncols >= 0");
    return hip_status(nvrx::scores(*a, S(stream)), "nvrx_scores");
}

int nvrx_score_attribution(const nvrx_attribution_args* a, void* stream) {
    NVRX_CHECK_ARG(a, "nvrx_score_attribution: null args");
    NVRX_CHECK_ARG(a->top >= 1 && a->top <= NVRX_MAX_ATTRIBUTION,
                   "nvrx_score_attribution: top must be in [1, NVRX_MAX_ATTRIBUTION = 16]");
    NVRX_CHECK_ARG(a->kind == NVRX_ATTR_RELATIVE || a->kind == NVRX_ATTR_INDIVIDUAL,
                   "nvrx_score_attribution: unknown kind (NVRX_ATTR_RELATIVE or NVRX_ATTR_INDIVIDUAL)");
    NVRX_CHECK_ARG(a->R >= 0, "nvrx_score_attribution: negative R");
    NVRX_CHECK_ARG(a->K >= 0, "nvrx_score_attribution: negative K");
    NVRX_CHECK_ARG(a->R < (int64_t)1 << 31, "nvrx_score_attribution: R must be below 2^31");
    NVRX_CHECK_ARG(a->K < (int64_t)1 << 31, "nvrx_score_attribution: K must be below 2^31");
    NVRX_CHECK_ARG(a->value_f64 == 0 || a->value_f64 == 1, "nvrx_score_attribution: bad value_f64");
    NVRX_CHECK_ARG(!a->hist_index || a->hist_stride > 0,
                   "nvrx_score_attribution: hist_index requires hist_stride");
    if (a->R > 0 && a->K > 0) {
        NVRX_CHECK_ARG(a->num, "nvrx_score_attribution: null num");
        NVRX_CHECK_ARG(a->med, "nvrx_score_attribution: null med");
        NVRX_CHECK_ARG(a->avg, "nvrx_score_attribution: null avg");
        NVRX_CHECK_ARG(a->idx, "nvrx_score_attribution: null idx");
        NVRX_CHECK_ARG(a->loss, "nvrx_score_attribution: null loss");
        NVRX_CHECK_ARG(a->score, "nvrx_score_attribution: null score");
        NVRX_CHECK_ARG(a->kind != NVRX_ATTR_RELATIVE || a->ref,
                       "nvrx_score_attribution: the relative kind needs ref");
        NVRX_CHECK_ARG(a->kind != NVRX_ATTR_INDIVIDUAL || a->hist,
                       "nvrx_score_attribution: the individual kind needs hist");
    }
    return hip_status(nvrx::score_attribution(*a, S(stream)), "nvrx_score_attribution");
}

// the ranks behind a kernel's score loss (score_rank_attribution.hip): nvrx_score_attribution's
// input checks, nvrx_rank_attribution's request, outputs and work
int nvrx_score_rank_attribution(const nvrx_scorerank_args* a, void* stream) {
    const std::string fn("nvrx_score_rank_attribution");
    NVRX_CHECK_ARG(a, fn + ": null args");
    if (int rc = check_rank_request(fn, a->R, a->K, a->top)) return rc;
    NVRX_CHECK_ARG(a->kind == NVRX_ATTR_RELATIVE || a->kind == NVRX_ATTR_INDIVIDUAL,
                   fn + ": unknown kind (NVRX_ATTR_RELATIVE or NVRX_ATTR_INDIVIDUAL)");
    NVRX_CHECK_ARG(a->R < (int64_t)1 << 31, fn + ": R must be below 2^31");
    NVRX_CHECK_ARG(a->K < (int64_t)1 << 31, fn + ": K must be below 2^31");
    NVRX_CHECK_ARG(a->value_f64 == 0 || a->value_f64 == 1, fn + ": bad value_f64");
    NVRX_CHECK_ARG(!a->hist_index || a->hist_stride > 0, fn + ": hist_index requires hist_stride");
    if (a->R > 0 && a->K > 0) {
        int64_t work_bytes = 0;
        nvrx::rank_attribution_plan(a->R, a->K, a->top, nullptr, nullptr, &work_bytes);
        NVRX_CHECK_ARG(a->num, fn + ": null num");
        NVRX_CHECK_ARG(a->med, fn + ": null med");
        NVRX_CHECK_ARG(a->avg, fn + ": null avg");
        NVRX_CHECK_ARG(a->idx, fn + ": null idx");
        NVRX_CHECK_ARG(a->loss, fn + ": null loss");
        NVRX_CHECK_ARG(a->score, fn + ": null score");
        NVRX_CHECK_ARG(a->taken, fn + ": null taken");
        NVRX_CHECK_ARG(a->positive, fn + ": null positive");
        NVRX_CHECK_ARG(a->kind != NVRX_ATTR_RELATIVE || a->ref, fn + ": the relative kind needs ref");
        NVRX_CHECK_ARG(a->kind != NVRX_ATTR_INDIVIDUAL || a->hist,
                       fn + ": the individual kind needs hist");
        NVRX_CHECK_ARG(work_bytes == 0 || a->work, fn + ": null work (the plan needs work_bytes)");
    }
    NVRX_CHECK_ARG(((uintptr_t)a->loss & 7) == 0, fn + ": loss not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->score & 7) == 0, fn + ": score not 8-byte aligned");
    NVRX_CHECK_ARG(((uintptr_t)a->work & 7) == 0, fn + ": work not 8-byte aligned");
    return hip_status(nvrx::score_rank_attribution(*a, S(stream)), fn.c_str());
}

int nvrx_finalize_scores(const double* partials, int64_t R, int64_t nshards, int32_t round_f32,
                         double thr_rel, double thr_ind, double* gpu_rel, double* gpu_ind,
                         uint8_t* strag_rel, uint8_t* strag_ind, int32_t* err, void* stream) {
    NVRX_CHECK_ARG(R >= 0, "nvrx_finalize_scores: negative R");
    NVRX_CHECK_ARG(nshards >= 1, "nvrx_finalize_scores: nshards must be at least 1");
    NVRX_CHECK_ARG(R == 0 || partials, "nvrx_finalize_scores: null partials");
    return hip_status(nvrx::finalize_scores(partials, R, nshards, round_f32, thr_rel, thr_ind,
                                            gpu_rel, gpu_ind, strag_rel, strag_ind, err, S(stream)),
                      "nvrx_finalize_scores");
}

int nvrx_section_scores(const double* med, const uint8_t* present, int64_t R, int64_t S_,
                        const float* ref_in, const int32_t* ref_index, float* ref_work,
                        double* hist, int32_t round_f32, double* out_rel, double* out_ind,
                        int32_t* err, void* stream) {
    NVRX_CHECK_ARG(R >= 0 && S_ >= 0, "nvrx_section_scores: negative size");
    NVRX_CHECK_ARG(R == 0 || S_ == 0 || (med && present), "nvrx_section_scores: null med/present");
    NVRX_CHECK_ARG(!out_ind || hist, "nvrx_section_scores: individual scores need hist");
    NVRX_CHECK_ARG(!out_rel || ref_in || ref_work, "nvrx_section_scores: need ref_in or ref_work");
    return hip_status(nvrx::section_scores(med, present, R, S_, ref_in, ref_index, ref_work, hist,
                                           round_f32, out_rel, out_ind, err, S(stream)),
                      "nvrx_section_scores");
}

int nvrx_section_stats(const double* vals, const int64_t* off, int64_t nsec, int64_t max_len,
                       int32_t* num, double* mn, double* mx, double* med, double* avg,
                       double* sd, void* stream) {
    NVRX_CHECK_ARG(nsec >= 0 && max_len >= 0, "nvrx_section_stats: negative size");
    NVRX_CHECK_ARG(nsec == 0 || (vals && off && num && mn && mx && med && avg && sd),
                   "nvrx_section_stats: null array");
    return hip_status(nvrx::section_stats(vals, off, nsec, max_len, num, mn, mx, med, avg, sd,
                                          S(stream)),
                      "nvrx_section_stats");
}

int nvrx_stragglers(const double* score, int64_t n, double thr, uint8_t* mask, void* stream) {
    NVRX_CHECK_ARG(n >= 0, "nvrx_stragglers: negative n");
    NVRX_CHECK_ARG(n == 0 || (score && mask), "nvrx_stragglers: null score/mask");
    return hip_status(nvrx::stragglers(score, n, thr, mask, S(stream)), "nvrx_stragglers");
}

// ------------------------------------------------------------------ record streams
int64_t nvrx_records_bucket_capacity(int64_t n, int64_t nstreams, int64_t nslots) {
    return nvrx::records_bucket_capacity(n, nstreams, nslots);
}
int nvrx_records_stats(const nvrx_record* recs, const int64_t* rec_off, int64_t nstreams,
                       int64_t nslots, int64_t cap, int32_t mode, int64_t max_len, int64_t* seg_off,
                       int32_t* seg_len, uint32_t* out_ns, int32_t* counts,
                       const nvrx_stats_soa* out, uint32_t* col_ref, void* stream) {
    NVRX_CHECK_ARG(nstreams >= 0 && nslots >= 0 && max_len >= 0, "nvrx_records_stats: negative size");
    NVRX_CHECK_ARG(all_columns(out), "nvrx_records_stats: null output array");
    NVRX_CHECK_ARG(nstreams == 0 || nslots == 0 || (recs && rec_off && seg_off && seg_len && out_ns),
                   "nvrx_records_stats: null array");  // counts may be NULL (not written)
    NVRX_CHECK_ARG(mode == NVRX_STATS_FAST || mode == NVRX_STATS_EXACT,
                   "nvrx_records_stats: unknown mode");
    NVRX_CHECK_ARG(nstreams * nslots < (int64_t)1 << 31, "nvrx_records_stats: too many segments");
    NVRX_CHECK_ARG(((uintptr_t)out_ns & 15) == 0, "nvrx_records_stats: out_ns not 16-byte aligned");
    const int64_t keep = (cap > 0 && max_len > cap) ? cap : max_len;
    NVRX_CHECK_ARG(keep <= NVRX_MAX_SEGMENT, "nvrx_records_stats: retained run longer than NVRX_MAX_SEGMENT (2^30)");
    return hip_status(nvrx::records_stats(recs, rec_off, nstreams, nslots, cap, mode, max_len,
                                          seg_off, seg_len, out_ns, counts, *out, col_ref, S(stream)),
                      "nvrx_records_stats");
}

int64_t nvrx_records_max_slots(void) { return NVRX_RECORDS_MAX_LDS / (3 * sizeof(uint32_t)); }  // W = 1

int nvrx_records_bucket(const nvrx_record* recs, const int64_t* rec_off, int64_t nstreams,
                        int64_t nslots, int64_t cap, int64_t* seg_off, int32_t* seg_len,
                        uint32_t* out_ns, int32_t* counts, void* stream) {
    NVRX_CHECK_ARG(nstreams >= 0 && nslots >= 0, "nvrx_records_bucket: negative size");
    NVRX_CHECK_ARG(nstreams == 0 || nslots == 0 ||
                       (rec_off && seg_off && seg_len && out_ns && counts),
                   "nvrx_records_bucket: null array");
    NVRX_CHECK_ARG(nstreams < (int64_t)1 << 31, "nvrx_records_bucket: too many streams");
    NVRX_CHECK_ARG(((uintptr_t)out_ns & 15) == 0, "nvrx_records_bucket: out_ns not 16-byte aligned");
    return hip_status(nvrx::records_bucket(recs, rec_off, nstreams, nslots, cap, 0, seg_off,
                                           seg_len, out_ns, counts, S(stream)),
                      "nvrx_records_bucket");
}

}  // extern "C"
