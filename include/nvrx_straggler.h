/*
 * nvrx_straggler.h -- C ABI of the MI355X-native straggler-detection scoring path.
 *
 * Implemented by libnvrx_hip.so (hand-written HIP kernels for gfx950).  Every entry
 * point takes plain pointers and sizes; no torch types cross this boundary.  Device
 * pointers are caller-owned (e.g. torch tensors' data_ptr()); `stream` is a
 * hipStream_t (NULL = default stream).  Calls are stream-ordered and asynchronous,
 * except nvrx_sync, the nvrx_profiler_* lifecycle calls and functions documented as
 * "synchronous".  Nothing is retained after return except state owned by a
 * nvrx_profiler handle.
 *
 * Errors: every function returns NVRX_OK (0) or a negative NVRX_ERR_*; the message
 * of the last error on the calling thread is nvrx_last_error().  The Python layer
 * raises RuntimeError with that message, as the reference's CUPTI_CALL -> std::
 * runtime_error -> RuntimeError path does (cupti_src/CuptiProfiler.cpp:30-38).
 *
 * Reference interfaces replaced (paths relative to
 * /root/reference/src/nvidia_resiliency_ext/straggler):
 *   nvrx_segment_stats_*   computeStats + CuptiProfiler::getStats   cupti_src/CuptiProfiler.cpp:44-74, 136-146
 *   nvrx_kernel_ref        ReportGenerator._all_reduce_times (MIN over ranks, -1 => NaN)   reporting.py:255-296
 *   nvrx_pack_min_times    the [K+Nsec] float32 pack of _all_reduce_times                 reporting.py:269-279
 *   nvrx_scores            _update_local_min_times + _compute_gpu_perf_score              reporting.py:298-314, 219-253
 *   nvrx_finalize_scores   score = sum(s*w)/sum(w), NaN if no common kernel; optional
 *                          float32 rounding of _get_tensor_from_scores                    reporting.py:251-253, 338-361
 *   nvrx_section_scores    _compute_sections_perf_scores (+ section MIN reduce, history)  reporting.py:196-217, 255-314
 *   nvrx_stragglers        Report.identify_stragglers (score < threshold, strict)         reporting.py:84-151
 *   nvrx_section_stats     Detector._get_section_summaries (torch f64 stats)             straggler.py:171-197
 *   nvrx_profiler_*        nvrx_cupti_module.CuptiProfiler (ctor, initialize, shutdown,
 *                          start, stop, get_stats, reset)                                 cupti_src/cupti_module_py.cpp:33-54
 *   nvrx_records_*         CuptiProfiler::bufferCompleted record loop + CircularBuffer     cupti_src/CuptiProfiler.cpp:168-203, CircularBuffer.h:53-69
 * Beyond the reference (no counterpart there): nvrx_segment_quantiles_*, nvrx_score_attribution,
 * nvrx_histogram_bucket / _edge, nvrx_segment_histogram_*, nvrx_profiler_get_histograms,
 * nvrx_histogram_sum / _tail_threshold / _tail_scores, nvrx_histogram_history_scores,
 * nvrx_histogram_tail_base / _tail_attribution, nvrx_segment_fleet_histogram_ragged,
 * nvrx_segment_tail_scores_ragged, nvrx_segment_tail_attribution_ragged,
 * nvrx_segment_history_scores_ragged, nvrx_segment_history_attribution_ragged,
 * nvrx_segment_history_scores_compact_ragged, nvrx_segment_history_attribution_compact_ragged,
 * nvrx_compact_history_age, nvrx_histogram_history_age, nvrx_histogram_history_scores_compact,
 * nvrx_compact_history_from_dense, nvrx_compact_history_to_dense,
 * nvrx_histogram_history_attribution_compact, nvrx_rank_attribution / _plan,
 * nvrx_score_rank_attribution.
 */
#ifndef NVRX_STRAGGLER_H
#define NVRX_STRAGGLER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVRX_ABI_VERSION 6

#define NVRX_OK 0
#define NVRX_ERR_INVALID -1   /* bad argument / shape */
#define NVRX_ERR_HIP -2       /* HIP runtime error */
#define NVRX_ERR_STATE -3     /* call not valid in the current state */
#define NVRX_ERR_SINGLETON -4 /* a second profiler instance (CuptiProfiler.cpp:86-87) */
#define NVRX_ERR_NOMEM -5
#define NVRX_ERR_RUNTIME -6 /* rocprofiler-sdk / runtime configuration refused */

/* statistics modes */
#define NVRX_STATS_FAST 0  /* NUM/MIN/MAX/MED bit-exact; AVG/STD exact mean/std rounded once to f32 */
#define NVRX_STATS_EXACT 1 /* every field bit-exact with computeStats (sequential f32 over sorted) */
/* flag OR-ed into the mode of nvrx_segment_stats_strided: col_ref already holds the initial
 * column reference (+inf bits | 0), e.g. re-initialised by the previous report's nvrx_scores
 * (nvrx_score_args.reset_col_ref), so the initialising launch is skipped */
#define NVRX_STATS_COLREF_READY 0x10

/* largest retained segment (statsMaxLenPerKernel) the kernels accept.  The reference's ring takes
 * any capacity (CuptiProfiler.h:49-51); rings of up to 32,768 samples are sorted on chip, longer
 * ones in device scratch (slower, same bits): 4 B per retained sample of every segment in flight,
 * up to 256 MiB per launch and, near 2^30, 4 GiB for one segment's workgroup.  Freed scratch above
 * 256 MiB returns to the driver at the next synchronisation.  Practical rings are <= 2^24 samples
 * (nvrx_profiler_create warns above that). */
#define NVRX_MAX_SEGMENT (1 << 30)

/* SoA output of the statistics kernels: one entry per segment (device pointers).
 * Units are microseconds as float32, like KernelStats (CuptiProfiler.h:39-45). */
typedef struct nvrx_stats_soa {
    int32_t* num;
    float* min;
    float* max;
    float* med;
    float* avg;
    float* std;
} nvrx_stats_soa;

/* Arguments of nvrx_scores: R score rows (ranks) x K kernel columns, row-major.
 * value_f64 selects the element type of med / avg / hist: 0 = float32 (statistics from
 * the segment kernels, exact in f64), 1 = float64 (summaries handed in through the
 * ReportGenerator API, whose MED/AVG are Python floats). */
typedef struct nvrx_score_args {
    int64_t R, K;
    int32_t value_f64;
    const int32_t* num;        /* [R][K] NUM; <= 0 means the kernel is absent on that rank */
    const void* med;           /* [R][K] MED (us), float or double */
    const void* avg;           /* [R][K] AVG (us), float or double */
    const uint8_t* col_valid;  /* [K] 0 = column filtered out ("ncclDev"), NULL = all valid */
    /* relative score reference (NULL = relative scores not computed) */
    const float* ref;          /* ref[ref_index ? ref_index[k] : k]; a value !(>= 0) (NaN, -1) = missing */
    const int32_t* ref_index;  /* [K] or NULL */
    const uint32_t* ref_missing; /* [K] or NULL: nonzero => reference missing (NaN) */
    /* individual score history (NULL = individual scores not computed); updated in place
     * to min(hist, MED) for every present kernel BEFORE scoring (reporting.py:469-474) */
    void* hist;                /* hist[r*hist_stride + (hist_index ? hist_index[k] : k)], float or double */
    const int32_t* hist_index; /* [K] or NULL */
    int64_t hist_stride;       /* per-row stride of hist; 0 => K */
    /* output: partial sums per row, 6 doubles (NULL allowed when finalizing in place):
     * {sum s*w (rel), sum w (rel), n (rel), sum s*w (ind), sum w (ind), n (ind)} */
    double* partials;          /* [R][6] */
    int32_t* err;              /* [1] device flags |= 1 when some MED == 0, |= 2 when a score's
                                  total weight is 0 (ZeroDivisionError) */
    /* optional in-kernel finalize (single shard), as nvrx_finalize_scores: any may be NULL */
    int32_t round_f32;
    double thr_rel, thr_ind;
    double* gpu_rel;
    double* gpu_ind;
    uint8_t* strag_rel;
    uint8_t* strag_ind;
    /* optional self-resetting epilogue, for reports replayed back to back (HIP graphs): with
     * `done` (2 u32 of device memory, zero before the first call) the error bits collect in
     * done[1] and the LAST workgroup to finish stores them to *err (no zeroing of *err needed
     * before the call), re-initialises reset_col_ref[0 : 2*reset_ncols] to the initial column
     * reference for the next report's statistics (NVRX_STATS_COLREF_READY) and zeroes done. */
    uint32_t* done;
    uint32_t* reset_col_ref;
    int64_t reset_ncols;
} nvrx_score_args;

/* ---------------------------------------------------------------- library */
const char* nvrx_last_error(void);
int nvrx_abi_version(void);
int nvrx_device_count(int* count);             /* synchronous */
int nvrx_sync(void* stream);                   /* synchronous: waits for `stream` */

/* ---------------------------------------------------------------- durations */
/* Every duration the library reads is a u32 DURATION KEY.  The reference keeps
 * (end - start) / 1000.0f (CuptiProfiler.cpp:187): the u64 ns difference rounded to f32, then
 * divided.  A key is the integer ns below NVRX_KEY_WIDE (3.76 s) and the f32 bits of f32(ns)
 * above it (0xE0000000 + bits(f32(ns)) - bits(f32(0xE0000000)), at most 0xF0200000), so it
 * keeps exactly what the reference keeps for any u64 duration, and keys order like the
 * durations.  nvrx_duration_key encodes one (host); a tracer feeding nvrx_profiler_ingest or a
 * matrix of durations of 3.76 s and more must encode them.  Below 3.76 s keys are plain ns.
 * Every u32 is read as a key: a RAW u32 ns of 3.76 s or more (never encoded) would be read as
 * the f32 bits of a far larger duration, so nvrx_encode_ns_u32 turns a device array of raw u32
 * ns into keys in place first.  u32 values above NVRX_KEY_MAX come from no u64 duration (they
 * decode beyond 2^64 ns, keeping the order). */
#define NVRX_KEY_WIDE 0xE0000000u
#define NVRX_KEY_WIDE_F32BITS 0x4F600000u /* bits of f32(0xE0000000) */
#define NVRX_KEY_MAX 0xF0200000u          /* key of f32(2^64 - 1) */
uint32_t nvrx_duration_key(uint64_t ns);
int nvrx_encode_ns_u32(uint32_t* ns, int64_t n, void* stream);

/* ---------------------------------------------------------------- statistics */
/* Segment s = ns[s*seg_stride + seg_begin : + seg_len] (uint32 duration keys); the
 * last min(seg_len, cap) samples are retained (cap <= 0: all).  out->* are [nseg].
 * col_ref (optional, [2*ncols] uint32): segments form a [nseg/ncols][ncols] rank x kernel
 * matrix; the call also produces the per-kernel relative reference of _all_reduce_times
 * (reporting.py:255-296): col_ref[c] = float bits of min over rows of MED, col_ref[ncols+c]
 * != 0 when some row has no sample of c (=> NaN).  Feed (float*)col_ref as nvrx_score_args
 * .ref and col_ref + ncols as .ref_missing. */
int nvrx_segment_stats_strided(const uint32_t* ns, int64_t nseg, int64_t seg_stride,
                               int64_t seg_begin, int64_t seg_len, int64_t cap, int32_t mode,
                               const nvrx_stats_soa* out, uint32_t* col_ref, int64_t ncols,
                               void* stream);
/* Segment s = ns[seg_off[s] : seg_off[s] + seg_len[s]] (device arrays; seg_len NULL:
 * seg_off has nseg+1 entries and segment s ends at seg_off[s+1]); max_len bounds every
 * segment length (host-known); aligned16 != 0 promises every retained run starts on a
 * 16-byte boundary; seg_len[s] < 0 skips segment s (outputs untouched).  col_ref / ncols:
 * as for the strided call (segment s is row s / ncols, column s % ncols).  Segments of <= 128 retained samples are bit-exact in every field in
 * both modes (one lane per segment, the reference's sequential f32 sums). */
int nvrx_segment_stats_ragged(const uint32_t* ns, const int64_t* seg_off, const int32_t* seg_len,
                              int64_t nseg, int64_t max_len, int64_t cap, int32_t mode,
                              int32_t aligned16, const nvrx_stats_soa* out, uint32_t* col_ref,
                              int64_t ncols, void* stream);

/* Tail quantiles of the same segments.  No reference counterpart (computeStats keeps MIN, MAX
 * and MED only): the order statistics a straggler that is slow on every n-th call shows up in.
 * A quantile is an integer permille pm in [0, 1000]; for a segment of n >= 1 retained samples
 * (the last min(len, cap), as above) the result is the sample of 0-based rank
 * (pm * (n - 1)) / 1000 (integer division, 64-bit) among the keys sorted ascending, converted to
 * us like every other sample -- no interpolation, so pm = 0 / 1000 have MIN's / MAX's bits and
 * pm = 500 of an odd n has MED's.  permille: HOST array of nq <= NVRX_MAX_QUANTILES entries
 * (copied at the call; any order, repeats allowed); out: [nq][nseg] f32 us, quantile-major, in the
 * order of permille; num: [nseg] retained lengths, or NULL.  An empty segment gives NaN and
 * num 0; in the ragged call seg_len[s] < 0 skips segment s (outputs untouched).  Stream-ordered:
 * kernels on `stream` only, no allocation, no synchronisation (capturable in a graph).
 * Segments are read by their own retained length: up to 8192 samples in one wave's registers
 * (one read of the segment), longer ones by a workgroup in four passes over memory. */
#define NVRX_MAX_QUANTILES 8
int nvrx_segment_quantiles_strided(const uint32_t* ns, int64_t nseg, int64_t seg_stride,
                                   int64_t seg_begin, int64_t seg_len, int64_t cap,
                                   const int32_t* permille, int32_t nq, float* out, int32_t* num,
                                   void* stream);
int nvrx_segment_quantiles_ragged(const uint32_t* ns, const int64_t* seg_off,
                                  const int32_t* seg_len, int64_t nseg, int64_t max_len,
                                  int64_t cap, int32_t aligned16, const int32_t* permille,
                                  int32_t nq, float* out, int32_t* num, void* stream);

/* Duration histograms of the same segments, with FIXED buckets: the same edges for every segment,
 * rank and report, so counts add -- over ranks to a fleet-wide distribution, over reports to a
 * whole run's -- and any quantile is known to within one bucket.  No reference counterpart.
 * Log-linear over the u32 duration key x, 3 mantissa bits, every bucket at most 12.5 % wide:
 *   bucket(x) = x                                  x < 8
 *             = 8*(e-2) + ((x >> (e-3)) & 7)       otherwise, e = 31 - clz(x)   (3..31)
 *   edge(b)   = b                                  b < 8     (lower edge, a key)
 *             = (8 + b%8) << (b/8 - 1)             otherwise; edge(240) := 2^32
 * bucket is monotone in the key (hence in the duration); edge(bucket(x)) <= x < edge(bucket(x)+1);
 * edge(238) == NVRX_KEY_WIDE, so buckets 238 and 239 hold exactly the wide keys (3.76 s and more)
 * and every bucket below holds plain ns; an edge in us is its key converted like every sample.
 * The scheme is part of the ABI.  nvrx_histogram_bucket / _edge are host functions (pure);
 * _edge takes 0..240 (2^32 for 240) and returns UINT64_MAX outside.
 * counts: [nseg][NVRX_HIST_BINS] u32 device memory, segment-major (16-byte aligned); num: [nseg]
 * retained lengths, or NULL.  accumulate == 0: all 240 bins of every segment taken are written
 * (no memset needed); != 0: the counts are added to what is there (one owner per segment, no
 * atomics on device memory).  An empty segment gives zero bins (nothing added) and num 0; in the
 * ragged call seg_len[s] < 0 skips segment s (outputs untouched).  Segments as for the statistics
 * calls, the last min(len, cap) samples retained.  Every segment is read exactly once.
 * Stream-ordered: kernels on `stream` only, no allocation, no synchronisation (capturable). */
#define NVRX_HIST_BINS 240
uint32_t nvrx_histogram_bucket(uint32_t key);
uint64_t nvrx_histogram_edge(int32_t bucket);
int nvrx_segment_histogram_strided(const uint32_t* ns, int64_t nseg, int64_t seg_stride,
                                   int64_t seg_begin, int64_t seg_len, int64_t cap,
                                   int32_t accumulate, uint32_t* counts, int32_t* num, void* stream);
int nvrx_segment_histogram_ragged(const uint32_t* ns, const int64_t* seg_off,
                                  const int32_t* seg_len, int64_t nseg, int64_t max_len,
                                  int64_t cap, int32_t aligned16, int32_t accumulate,
                                  uint32_t* counts, int32_t* num, void* stream);

/* Tail scores from the histograms: one score per row (rank) on the scale of the GPU scores -- about
 * 1 for a healthy rank, lower for a straggler -- that sees what the median hides: a rank slow on
 * every n-th call.  No reference counterpart.  Computed from integer counts, so exact and
 * deterministic.  The definition is part of the ABI; every sum is an exact integer.
 * Inputs: counts C[r][k][b], u32 over the NVRX_HIST_BINS fixed buckets, R rows x K kernels;
 * permille pm, an integer in [0, 1000].
 *   1. fleet histogram   F[k][b] = sum_r C[r][k][b]                                        (u64)
 *   2. threshold bucket  N_k = sum_b F[k][b];  T_k = the bucket that holds the fleet's sample of
 *                        0-based rank (pm * (N_k - 1)) / 1000 (64-bit integer division; the product
 *                        is taken exactly), i.e. the smallest b with sum_{b' <= b} F[k][b'] > rank:
 *                        the rank rule of the quantile calls.  T_k = -1 when N_k == 0 or
 *                        col_valid[k] == 0; such a kernel is skipped everywhere below.
 *   3. weights           w(b) = nvrx_histogram_edge(min(b, 238)) (u64): the bucket's lower edge in ns.
 *                        Buckets 238 and 239 both weigh NVRX_KEY_WIDE: keys there are not ns, and
 *                        3.76 s is still a true lower bound.
 *   4. per row           total_ns[r] = sum_k sum_b         C[r][k][b] * w(b)
 *                        tail_ns[r]  = sum_k sum_{b > T_k} C[r][k][b] * w(b)
 *                        (u64, over the kernels with T >= 0; lower bounds of real time, so they do
 *                        not overflow in a real run, and wrap mod 2^64 otherwise);
 *                        tail_calls[r][k] = sum_{b > T_k} C[r][k][b] (u32; 0 for a skipped kernel)
 *   5. fleet             fleet_total = sum_k sum_b F[k][b] * w(b),  fleet_tail = the same over
 *                        b > T_k, over the kernels with T >= 0
 *   6. score             in f64, each operation rounded separately, each u64 converted to f64
 *                        (round to nearest even) first:
 *                            share_r  = tail_ns[r] / total_ns[r]
 *                            fs       = fleet_tail / fleet_total
 *                            score[r] = (1.0 - share_r) / (1.0 - fs)
 *                        NaN when total_ns[r] == 0, fleet_total == 0 or 1.0 - fs == 0.0;
 *                        strag[r] = score[r] < score_thr (strict; NaN never), as nvrx_stragglers.
 * score is about the time the row would have needed with a fleet-typical tail, divided by the time
 * it needed -- the meaning of ref / MED.  Limits: a slowdown of less than one bucket (12.5 %) may
 * not cross T_k; and pm must leave more room than the slow rank's own share of the fleet's samples
 * (8 ranks, one of them slow on every 10th call: its slow calls are 1.25 % of the fleet, pm = 990
 * puts T_k inside them -- use 950 there).
 *
 * nvrx_histogram_sum: fleet[K][240] (u64, 16-byte aligned) = the column sum of counts[R][K][240]
 *   (u32, 16-byte aligned, rows contiguous); accumulate != 0 adds to what fleet holds (a run-long
 *   fleet), otherwise all K * 240 bins are written.
 * nvrx_histogram_tail_threshold: thr[K] (i32) = T_k of fleet for `permille`; col_valid: [K] u8 or
 *   NULL (all valid); fleet_sums[2] (u64) = {fleet_tail, fleet_total}, written in full.
 * nvrx_histogram_tail_scores: steps 4 and 6 for the R rows of counts.  Column k uses
 *   thr[thr_index ? thr_index[k] : k]; a negative index, like a negative thr, skips the kernel (a
 *   rank whose kernels are a subset of the fleet's, as ref_index of nvrx_scores).  tail_calls and
 *   strag may be NULL.
 * K * 240 and R * K must be below 2^31.  R == 0 or K == 0 launches nothing (outputs untouched).
 * Stream-ordered: kernels on `stream` only, no allocation, no synchronisation, no host read-back;
 * the three calls in a row form a linear sequence that can be captured in a graph. */
typedef struct nvrx_tail_args {
    int64_t R, K;
    const uint32_t* counts;     /* [R][K][NVRX_HIST_BINS] */
    const int32_t* thr;         /* threshold buckets, from nvrx_histogram_tail_threshold */
    const int32_t* thr_index;   /* [K] or NULL */
    const uint64_t* fleet_sums; /* [2] {fleet_tail, fleet_total} */
    uint64_t* tail_ns;          /* [R] */
    uint64_t* total_ns;         /* [R] */
    double* score;              /* [R] */
    uint32_t* tail_calls;       /* [R][K] or NULL */
    uint8_t* strag;             /* [R] or NULL */
    double score_thr;
} nvrx_tail_args;
int nvrx_histogram_sum(const uint32_t* counts, int64_t R, int64_t K, int32_t accumulate,
                       uint64_t* fleet, void* stream);
int nvrx_histogram_tail_threshold(const uint64_t* fleet, int64_t K, int32_t permille,
                                  const uint8_t* col_valid, int32_t* thr, uint64_t* fleet_sums,
                                  void* stream);
int nvrx_histogram_tail_scores(const nvrx_tail_args* args, void* stream);

/* The same tail scores straight from ragged segments, without the counts matrix (960 B per row and
 * kernel: more than the samples themselves where most segments hold a few, as the buckets of
 * record streams do).  No reference counterpart.  Segments as for nvrx_segment_histogram_ragged:
 * segment r * K + k is row r, kernel k; the last min(len, cap) samples are retained; seg_len[s] <= 0
 * contributes nothing; seg_len NULL: seg_off holds R * K + 1 offsets.  By definition
 *   nvrx_segment_fleet_histogram_ragged  writes (accumulate != 0: adds) into fleet[K][240] (u64,
 *     16-byte aligned) what is equal to nvrx_histogram_sum applied to the counts
 *     nvrx_segment_histogram_ragged would write into a zeroed matrix;
 *   nvrx_segment_tail_scores_ragged  writes into tail_ns, total_ns (u64, 8-byte aligned), score,
 *     strag (or NULL) and tail_calls (or NULL; [R][K], written in full) what is equal to
 *     nvrx_histogram_tail_scores applied to those counts, thr / thr_index / fleet_sums / score_thr
 *     as there (steps 4 and 6 of the definition above);
 * nvrx_histogram_tail_threshold on the fleet goes between the two.  Every sum is an exact integer,
 * so the results equal the dense chain's bit for bit and are identical from run to run.
 * K * 240 and R * K must be below 2^31, the retained run at most NVRX_MAX_SEGMENT.  R == 0 or K == 0
 * launches nothing (outputs untouched).  Stream-ordered: kernels on `stream` only, no allocation,
 * no synchronisation, no host read-back; the three calls form a linear sequence that can be
 * captured in a graph. */
typedef struct nvrx_segtail_args {
    int64_t R, K;
    const uint32_t* ns;         /* duration keys */
    const int64_t* seg_off;     /* [R * K] (+ 1 without seg_len) */
    const int32_t* seg_len;     /* [R * K] or NULL */
    int64_t max_len, cap;
    int32_t aligned16;          /* the caller's word that every retained run starts 16-byte aligned */
    const int32_t* thr;         /* threshold buckets, from nvrx_histogram_tail_threshold */
    const int32_t* thr_index;   /* [K] or NULL */
    const uint64_t* fleet_sums; /* [2] {fleet_tail, fleet_total} */
    uint64_t* tail_ns;          /* [R] */
    uint64_t* total_ns;         /* [R] */
    double* score;              /* [R] */
    uint32_t* tail_calls;       /* [R][K] or NULL */
    uint8_t* strag;             /* [R] or NULL */
    double score_thr;
} nvrx_segtail_args;
int nvrx_segment_fleet_histogram_ragged(const uint32_t* ns, const int64_t* seg_off,
                                        const int32_t* seg_len, int64_t R, int64_t K,
                                        int64_t max_len, int64_t cap, int32_t aligned16,
                                        int32_t accumulate, uint64_t* fleet, void* stream);
int nvrx_segment_tail_scores_ragged(const nvrx_segtail_args* args, void* stream);

/* Individual tail scores: a row (rank) against its own histogram history -- the individual leg of
 * the tail scores above, as hist of nvrx_score_args is the individual leg of the median-based
 * scores.  It sees what the relative tail score cannot: a world of one, a degradation that hits
 * every rank together, a large share of the ranks slow on every n-th call.  No reference
 * counterpart.  One fused, stream-ordered pass finds a threshold bucket per (row, kernel) in the
 * history, scores the current counts against it and folds them into the history.  The definition
 * is part of the ABI; every sum is an exact integer, so the result is the same on every run.
 * Inputs: counts C[r][k][b], u32, R rows x K kernels x NVRX_HIST_BINS buckets (what
 *   nvrx_segment_histogram_* writes; 16-byte aligned, rows contiguous);
 *   hist, u32, the same buckets, changed in place: the history of row r, slot s, is the 240 counts
 *   at hist + (r * hist_stride + s) * 240 (16-byte aligned); hist_stride is counted in histograms,
 *   0 means K;  hist_index[K] (i32) or NULL (identity): s = hist_index[k], a negative entry means
 *   column k has no history slot; every other entry must be below the stride (not checked);
 *   col_valid[K] (u8) or NULL (all valid);  permille pm, an integer in [0, 1000];
 *   skip_rows[R] (u8) or NULL;  mode, a bit set of NVRX_HTAIL_SCORE and NVRX_HTAIL_UPDATE, at least
 *   one of them;  score_thr.
 * Terms: w(b) = nvrx_histogram_edge(min(b, 238)) as for the tail scores above;  s = the slot of k;
 *   H = hist as it stands BEFORE this call;  N = sum_b H[r][s][b] (u64);  n = sum_b C[r][k][b].
 * SCORE
 *   eligible     (r, k) iff col_valid[k] != 0, s >= 0, N > 0 and n > 0.
 *   threshold    T[r][k] = the bucket that holds the history's sample of 0-based rank
 *                (pm * (N - 1)) / 1000 (64-bit integer division, the product taken exactly): the
 *                smallest b with sum_{b' <= b} H[r][s][b'] > rank, the rule of step 2 above.
 *   per row      u64 sums mod 2^64 over the eligible k:
 *                    total_ns[r]      = sum_k sum_b           C[r][k][b] * w(b)
 *                    tail_ns[r]       = sum_k sum_{b > T}     C[r][k][b] * w(b)
 *                    base_total_ns[r] = sum_k sum_b           H[r][s][b] * w(b)
 *                    base_tail_ns[r]  = sum_k sum_{b > T}     H[r][s][b] * w(b)
 *                tail_calls[r][k] = sum_{b > T} C[r][k][b] (u32; 0 where not eligible).
 *   score        in f64, each operation rounded separately, each u64 converted to f64 first:
 *                    score[r] = (1.0 - tail_ns[r] / total_ns[r]) /
 *                               (1.0 - base_tail_ns[r] / base_total_ns[r])
 *                NaN when total_ns[r] == 0, base_total_ns[r] == 0 or the denominator is 0.0;
 *                strag[r] = score[r] < score_thr (strict; NaN never).  A first interval has no
 *                history and gives NaN, which is never flagged.
 * UPDATE
 *   for every (r, k) with col_valid[k] != 0, s >= 0, and skip_rows NULL or skip_rows[r] == 0:
 *                    H[r][s][b] = min(H[r][s][b] + C[r][k][b], 2^32 - 1)
 *   (the sum is formed in 64 bits and saturates: a long run never wraps).  With both bits set the
 *   score uses the history from before the update.  A flagged interval can be kept out of the
 *   history without a host round trip: a SCORE call, then an UPDATE call with skip_rows = strag.
 * Two columns of one row must not map to the same slot, and counts and hist must not overlap;
 * neither is checked.  Outputs: tail_ns, total_ns, base_tail_ns, base_total_ns [R] u64 (8-byte
 * aligned), score [R] f64, strag [R] u8 or NULL, tail_calls [R][K] u32 or NULL (ignored without
 * SCORE).  Without SCORE no score output is touched or needed.  K * 240 and R * K must be below
 * 2^31.  R == 0 or K == 0 launches nothing.  Stream-ordered: kernels on `stream` only, no
 * allocation, no synchronisation, no host read-back; capturable as a linear chain.  The four u64
 * outputs are the accumulators of the pass (cleared on the stream first): they must not alias. */
#define NVRX_HTAIL_SCORE 1
#define NVRX_HTAIL_UPDATE 2
typedef struct nvrx_histtail_args {
    int64_t R, K;
    const uint32_t* counts;     /* [R][K][NVRX_HIST_BINS] */
    uint32_t* hist;             /* [R][hist_stride][NVRX_HIST_BINS], in place */
    int64_t hist_stride;        /* in histograms; 0: K */
    const int32_t* hist_index;  /* [K] or NULL */
    const uint8_t* col_valid;   /* [K] or NULL */
    const uint8_t* skip_rows;   /* [R] or NULL */
    int32_t permille;
    int32_t mode;               /* NVRX_HTAIL_SCORE | NVRX_HTAIL_UPDATE */
    double score_thr;
    uint64_t* tail_ns;          /* [R] */
    uint64_t* total_ns;         /* [R] */
    uint64_t* base_tail_ns;     /* [R] */
    uint64_t* base_total_ns;    /* [R] */
    double* score;              /* [R] */
    uint8_t* strag;             /* [R] or NULL */
    uint32_t* tail_calls;       /* [R][K] or NULL */
} nvrx_histtail_args;
int nvrx_histogram_history_scores(const nvrx_histtail_args* args, void* stream);

/* The same individual tail scores straight from ragged segments, without the counts matrix: the
 * individual leg for a fleet that arrives as record streams.  No reference counterpart.  Segments,
 * max_len, cap and aligned16 as in "The same tail scores straight from ragged segments" above:
 * segment r * K + k is row r, kernel k; the last min(len, cap) samples are retained; seg_len[s] <= 0
 * is an empty element; seg_len NULL: seg_off holds R * K + 1 offsets.  By definition
 *   nvrx_segment_history_scores_ragged  writes into tail_ns, total_ns, base_tail_ns, base_total_ns,
 *     score, strag and tail_calls, and changes in hist, exactly what nvrx_histogram_history_scores
 *     does for the same hist, hist_stride, hist_index, col_valid, skip_rows, permille, mode and
 *     score_thr applied to the counts nvrx_segment_histogram_ragged would write into a zeroed
 *     matrix for the same segments.
 * "n > 0" of that definition is "retained length > 0".  An empty element is therefore not eligible,
 * leaves its history slot bit-identical under UPDATE and gives tail_calls = 0; its history is not
 * read.  total, tail (u64 mod 2^64) and calls (u32) are sums of w(bucket(x)) / 1 over the retained
 * samples x; UPDATE adds, saturating, only to the bins the samples fall in.  SCORE, UPDATE and both
 * as there: with both bits the score sees the history from before the call; skip_rows may be the
 * strag a previous call wrote on the device; tail_calls ([R][K] or NULL) is written in full and
 * ignored without SCORE.  The history keeps its format, so one history can be continued by either
 * entry.  Every sum is an exact integer: the results equal the dense chain's bit for bit and are
 * identical from run to run.  hist 16-byte aligned; seg_off and the four u64 outputs 8-byte
 * aligned; mode needs at least one bit; permille in 0..1000; the retained run at most
 * NVRX_MAX_SEGMENT; K * 240 and R * K below 2^31.  R == 0 or K == 0 launches nothing.
 * Stream-ordered: kernels on `stream` only, no allocation, no synchronisation, no host read-back,
 * no scratch; capturable as a linear chain.  The four u64 outputs are the accumulators of the pass
 * (cleared on the stream first): they must not alias. */
typedef struct nvrx_seghist_args {
    int64_t R, K;
    const uint32_t* ns;         /* duration keys */
    const int64_t* seg_off;     /* [R * K] (+ 1 without seg_len) */
    const int32_t* seg_len;     /* [R * K] or NULL */
    int64_t max_len, cap;
    int32_t aligned16;          /* the caller's word that every retained run starts 16-byte aligned */
    uint32_t* hist;             /* [R][hist_stride][NVRX_HIST_BINS], in place */
    int64_t hist_stride;        /* in histograms; 0: K */
    const int32_t* hist_index;  /* [K] or NULL */
    const uint8_t* col_valid;   /* [K] or NULL */
    const uint8_t* skip_rows;   /* [R] or NULL */
    int32_t permille;
    int32_t mode;               /* NVRX_HTAIL_SCORE | NVRX_HTAIL_UPDATE */
    double score_thr;
    uint64_t* tail_ns;          /* [R] */
    uint64_t* total_ns;         /* [R] */
    uint64_t* base_tail_ns;     /* [R] */
    uint64_t* base_total_ns;    /* [R] */
    double* score;              /* [R] */
    uint8_t* strag;             /* [R] or NULL */
    uint32_t* tail_calls;       /* [R][K] or NULL */
} nvrx_seghist_args;
int nvrx_segment_history_scores_ragged(const nvrx_seghist_args* args, void* stream);

/* Tail score attribution: the kernels behind a rank's tail score.  No reference counterpart.  The
 * tail scores above flag a row that is slow on every n-th call; this names the kernels, per row
 * the `top` with the largest excess tail time.  tail_calls counts calls, and a count is not a
 * cost: a cheap kernel called thousands of times has dozens of calls above its 95 % bucket on a
 * healthy rank.  The definition is part of the ABI; terms (w(b), T, eligibility) as in the two
 * sections above.  For a taken element (r, k), as u64 sums mod 2^64:
 *     tail[r][k]  = sum_{b > T} C[r][k][b] * w(b)        total[r][k] = sum_b C[r][k][b] * w(b)
 *     calls[r][k] = sum_{b > T} C[r][k][b]  (u32)        btail, btotal: the base's over the same T
 * The base and T depend on `kind`:
 *   NVRX_ATTR_RELATIVE    base = the fleet row F[u], u = thr_index ? thr_index[k] : k, given as
 *                         base[u] = {btail, btotal} from nvrx_histogram_tail_base;  T = thr[u];
 *                         taken iff u >= 0, thr[u] >= 0 and sum_b C[r][k][b] > 0.
 *   NVRX_ATTR_INDIVIDUAL  base = H[r][s] as it stands when the call runs (READ ONLY here);  T from H
 *                         by the rank rule of nvrx_histogram_history_scores;  taken iff eligible
 *                         there: col_valid[k] != 0, s >= 0, N > 0 and n > 0.
 * Then in f64, each u64 converted first (round to nearest even), every operation rounded separately:
 *     share = btail / btotal
 *     loss  = tail - total * share      (ns; negative when the row's tail is lighter than the base's)
 * An element whose loss is NaN (btotal == 0: every sample of the base in bucket 0, whose weight is
 * 0) is left out, like an absent kernel.  Per row, sum_k tail[r][k] over the taken elements is the
 * score call's tail_ns[r] when that call takes the same elements; loss is the part of that tail
 * beyond what the base's tail share predicts.
 * Outputs, row-major, j < top (1 <= top <= NVRX_MAX_ATTRIBUTION):
 *     idx[r][j]         column of the j-th largest loss (ties: the lower column first;
 *                       -0.0 == +0.0), -1 beyond the elements taken
 *     loss[r][j]        f64, NaN where idx = -1
 *     tail_ns[r][j], total_ns[r][j]   u64, 0 where idx = -1
 *     tail_calls[r][j]  u32, 0 where idx = -1
 *     thr_bucket[r][j]  i32 T, -1 where idx = -1
 *     base_share[r][j]  f64 share, NaN where idx = -1
 *     loss_all[r][k]    f64, dense [R][K], NaN where not taken: workspace and output
 * nvrx_histogram_tail_base: base[K][2] (u64, 16-byte aligned) = {btail, btotal} per kernel of
 *   fleet[K][240] (u64, 16-byte aligned) over b > thr[k], {0, 0} where thr[k] < 0: the per-kernel
 *   sums nvrx_histogram_tail_threshold adds up, computed once and not per row.
 * nvrx_histogram_tail_attribution: two kernels on `stream` (every (r, k) has one owner: no atomics,
 *   no scratch).  counts and hist 16-byte aligned, tail_ns / total_ns / loss / base_share /
 *   loss_all / base 8-byte aligned.  hist_stride, hist_index, col_valid, permille: as
 *   nvrx_histogram_history_scores (individual only); thr, thr_index, base: relative only.
 * K * 240 and R * K must be below 2^31; top outside 1..16 or an unknown kind is an error.  R == 0 or
 * K == 0 launches nothing.  Stream-ordered: no allocation, no synchronisation, no host read-back;
 * capturable as a linear chain. */
typedef struct nvrx_tailattr_args {
    int64_t R, K;
    const uint32_t* counts;     /* [R][K][NVRX_HIST_BINS] */
    int32_t kind, top;          /* NVRX_ATTR_RELATIVE / NVRX_ATTR_INDIVIDUAL; 1..NVRX_MAX_ATTRIBUTION */
    const int32_t* thr;         /* relative: threshold buckets of the fleet */
    const int32_t* thr_index;   /* relative: [K] or NULL */
    const uint64_t* base;       /* relative: [.][2] {btail, btotal}, from nvrx_histogram_tail_base */
    const uint32_t* hist;       /* individual: [R][hist_stride][NVRX_HIST_BINS], read only */
    int64_t hist_stride;        /* in histograms; 0: K */
    const int32_t* hist_index;  /* [K] or NULL */
    const uint8_t* col_valid;   /* individual: [K] or NULL */
    int32_t permille;           /* individual */
    int32_t* idx;               /* [R][top] */
    double* loss;               /* [R][top] */
    uint64_t* tail_ns;          /* [R][top] */
    uint64_t* total_ns;         /* [R][top] */
    uint32_t* tail_calls;       /* [R][top] */
    int32_t* thr_bucket;        /* [R][top] */
    double* base_share;         /* [R][top] */
    double* loss_all;           /* [R][K] */
} nvrx_tailattr_args;
int nvrx_histogram_tail_base(const uint64_t* fleet, int64_t K, const int32_t* thr, uint64_t* base,
                             void* stream);
int nvrx_histogram_tail_attribution(const nvrx_tailattr_args* args, void* stream);

/* The relative tail score attribution straight from ragged segments, without the counts matrix: the
 * step after nvrx_segment_tail_scores_ragged.  No reference counterpart.  Segments, max_len, cap
 * and aligned16 as in "The same tail scores straight from ragged segments" above; thr, thr_index,
 * base and every output as in "Tail score attribution" above.  By definition
 *   nvrx_segment_tail_attribution_ragged  writes into idx, loss, tail_ns, total_ns, tail_calls,
 *     thr_bucket, base_share ([R][top]) and loss_all ([R][K], written in full) what is equal to
 *     nvrx_histogram_tail_attribution with kind = NVRX_ATTR_RELATIVE applied to the counts
 *     nvrx_segment_histogram_ragged would write into a zeroed matrix for the same segments:
 *     an element (r, k) is taken iff u >= 0, thr[u] >= 0, its retained length is > 0 and its loss
 *     is not NaN; tail, total (u64 mod 2^64) and calls (u32) are sums of w(bucket(x)) / 1 over the
 *     retained samples x, tail and calls over bucket(x) > thr[u] only.
 * base[u] = {btail, btotal} comes from nvrx_histogram_tail_base on the fleet of
 * nvrx_segment_fleet_histogram_ragged and the thr of nvrx_histogram_tail_threshold.  Every sum is
 * an exact integer, so the results equal the dense chain's bit for bit and are identical from run
 * to run.  seg_off, base, loss, tail_ns, total_ns, base_share and loss_all 8-byte aligned; top in
 * 1..NVRX_MAX_ATTRIBUTION; K * 240 and R * K below 2^31; the retained run at most
 * NVRX_MAX_SEGMENT.  R == 0 or K == 0 launches nothing (outputs untouched).  Two kernels on
 * `stream` only (every (r, k) has one owner): no allocation, no synchronisation, no host
 * read-back, no scratch, no atomics; capturable as a linear chain with the calls before it. */
typedef struct nvrx_segtailattr_args {
    int64_t R, K;
    const uint32_t* ns;         /* duration keys */
    const int64_t* seg_off;     /* [R * K] (+ 1 without seg_len) */
    const int32_t* seg_len;     /* [R * K] or NULL */
    int64_t max_len, cap;
    int32_t aligned16;          /* the caller's word that every retained run starts 16-byte aligned */
    int32_t top;                /* 1..NVRX_MAX_ATTRIBUTION */
    const int32_t* thr;         /* threshold buckets, from nvrx_histogram_tail_threshold */
    const int32_t* thr_index;   /* [K] or NULL */
    const uint64_t* base;       /* [.][2] {btail, btotal}, from nvrx_histogram_tail_base */
    int32_t* idx;               /* [R][top] */
    double* loss;               /* [R][top] */
    uint64_t* tail_ns;          /* [R][top] */
    uint64_t* total_ns;         /* [R][top] */
    uint32_t* tail_calls;       /* [R][top] */
    int32_t* thr_bucket;        /* [R][top] */
    double* base_share;         /* [R][top] */
    double* loss_all;           /* [R][K] */
} nvrx_segtailattr_args;
int nvrx_segment_tail_attribution_ragged(const nvrx_segtailattr_args* args, void* stream);

/* The individual tail score attribution straight from ragged segments, without the counts matrix:
 * the step after (or between the two launches of) nvrx_segment_history_scores_ragged.  No reference
 * counterpart.  Segments, max_len, cap and aligned16 as in "The same tail scores straight from
 * ragged segments" above; hist, hist_stride, hist_index, col_valid and permille as in
 * nvrx_segment_history_scores_ragged; every output as in "Tail score attribution" above.  By
 * definition
 *   nvrx_segment_history_attribution_ragged  writes into idx, loss, tail_ns, total_ns, tail_calls,
 *     thr_bucket, base_share ([R][top]) and loss_all ([R][K], written in full) what is equal, bit
 *     for bit, to nvrx_histogram_tail_attribution with kind = NVRX_ATTR_INDIVIDUAL for the same
 *     hist, hist_stride, hist_index, col_valid, permille and top applied to the counts
 *     nvrx_segment_histogram_ragged would write into a zeroed matrix for the same segments:
 *     an element (r, k) is taken iff col_valid[k] != 0, its slot s >= 0, the history has N > 0, its
 *     retained length is > 0 and its loss is not NaN; tail, total (u64 mod 2^64) and calls (u32)
 *     are sums of w(bucket(x)) / 1 over the retained samples x, tail and calls over bucket(x) > T
 *     only; T, btail and btotal come from H[r][s] by the rank rule of
 *     nvrx_histogram_history_scores; share = btail / btotal and loss = tail - total * share are
 *     three separately rounded f64 operations; ties go to the lower column, -0.0 == +0.0; beyond
 *     the taken elements the outputs are -1 / NaN / 0.
 * hist is READ ONLY here: run the entry between a SCORE call and an UPDATE call and it sees the
 * history the score saw.  An empty element (seg_len <= 0) gets NaN in loss_all, and its 960 B of
 * history are not read.  Every sum is an exact integer, so the results equal the dense chain's bit
 * for bit and are identical from run to run.  hist 16-byte aligned; seg_off, loss, tail_ns,
 * total_ns, base_share and loss_all 8-byte aligned; top in 1..NVRX_MAX_ATTRIBUTION; permille in
 * 0..1000; hist_stride 0 or, without hist_index, at least K; the retained run at most
 * NVRX_MAX_SEGMENT; K * 240 and R * K below 2^31.  R == 0 or K == 0 launches nothing (outputs
 * untouched).  Two kernels on `stream` only (every (r, k) has one owner): no allocation, no
 * synchronisation, no host read-back, no scratch, no atomics; capturable as a linear chain with
 * the calls around it. */
typedef struct nvrx_seghistattr_args {
    int64_t R, K;
    const uint32_t* ns;         /* duration keys */
    const int64_t* seg_off;     /* [R * K] (+ 1 without seg_len) */
    const int32_t* seg_len;     /* [R * K] or NULL */
    int64_t max_len, cap;
    int32_t aligned16;          /* the caller's word that every retained run starts 16-byte aligned */
    int32_t top;                /* 1..NVRX_MAX_ATTRIBUTION */
    const uint32_t* hist;       /* [R][hist_stride][NVRX_HIST_BINS], read only */
    int64_t hist_stride;        /* in histograms; 0: K */
    const int32_t* hist_index;  /* [K] or NULL */
    const uint8_t* col_valid;   /* [K] or NULL */
    int32_t permille;
    int32_t* idx;               /* [R][top] */
    double* loss;               /* [R][top] */
    uint64_t* tail_ns;          /* [R][top] */
    uint64_t* total_ns;         /* [R][top] */
    uint32_t* tail_calls;       /* [R][top] */
    int32_t* thr_bucket;        /* [R][top] */
    double* base_share;         /* [R][top] */
    double* loss_all;           /* [R][K] */
} nvrx_seghistattr_args;
int nvrx_segment_history_attribution_ragged(const nvrx_seghistattr_args* args, void* stream);

/* The individual tail scores of record streams against a COMPACT history: 64 bytes per (rank,
 * kernel) in place of the dense 960.  No reference counterpart.  A real kernel's durations sit in
 * one to three of the 240 buckets, so the compact history keeps at most NVRX_CHIST_ENTRIES used
 * buckets per element and folds what does not fit into the nearest kept bucket below.
 *
 * Element layout (NVRX_CHIST_BYTES = 64 bytes, 16-byte aligned):
 *   bytes  0..47  u32 count[12]
 *   bytes 48..59  u8  bucket[12]
 *   bytes 60..63  u32 n, the number of used entries
 * Canonical form: n <= 12; entries 0..n-1 have strictly ascending bucket < 240 and count >= 1;
 * entries n..11 are all zero.  An all-zero element is the empty history, so clearing the memory
 * resets it.  The device assumes canonical input and always writes canonical output.
 *
 * The history is chist[R][stride] elements.  Segments, max_len, cap, aligned16, hist_index,
 * hist_stride, col_valid, skip_rows, permille, mode and score_thr mean exactly what they do for
 * nvrx_segment_history_scores_ragged.
 *
 * SCORE is exactly the score of nvrx_segment_history_scores_ragged with H set to the dense
 * expansion of the element before the call: H[bucket[i]] = count[i] for i < n, zero elsewhere.
 * Eligibility, T, the four u64 sums, tail_calls, the three separately rounded f64 operations and
 * strag are unchanged.  The interval's sums come from the samples and are not affected by folding.
 *
 * UPDATE applies to every (r, k) that has col_valid[k], a slot s >= 0, skip_rows[r] = 0 and a
 * retained length > 0.  With c[b] the counts of the retained window and S the element's used
 * buckets:
 *   admission    New = {b : c[b] > 0, b not in S} in ascending order; the first
 *                min(|New|, 12 - |S|) of them are admitted, giving S'.
 *   target       for every b with c[b] > 0: t(b) = max{s in S' : s <= b}, or min S' if there is
 *                no such s.
 *   new counts   count'[t] = min(count[t] + sum_{b : t(b) = t} c[b], 2^32 - 1), the sum taken in 64
 *                bits, so the order of the adds cannot matter.
 *   result       the entries re-sorted, n = |S'|: canonical.
 *   folded[r]    (u64) the sum of c[b] over b not in S' over the row's updated elements; cleared
 *                on the stream first; written only when the UPDATE bit is set.
 * S' is never empty when there is a sample.  An element without samples is bit-identical
 * afterwards and its 64 bytes are not written.  SCORE | UPDATE scores against the history from
 * before the update.
 *
 * Relation to the dense history: where no element ever exceeds 12 buckets (folded == 0) the
 * compact history expands to exactly the dense history nvrx_segment_history_scores_ragged
 * produces, and every output is bit-identical to that entry's.  Folding conserves N (away from
 * saturation), so the rank rule stays meaningful; it only moves weight to a lower edge, and folded
 * says how much.
 *
 * chist 16-byte aligned; seg_off, the four u64 outputs, score and folded 8-byte aligned; mode needs
 * at least one bit; permille in 0..1000; the retained run at most NVRX_MAX_SEGMENT; K * 240 and
 * R * K below 2^31.  folded is required with UPDATE and must not alias the other outputs.  Two
 * columns must not share a slot.  R == 0 or K == 0 launches nothing.  Stream-ordered: kernels on
 * `stream` only, no allocation, no synchronisation, no host read-back, no scratch; capturable as
 * a linear chain. */
#define NVRX_CHIST_ENTRIES 12
#define NVRX_CHIST_BYTES 64
typedef struct nvrx_segchist_args {
    int64_t R, K;
    const uint32_t* ns;         /* duration keys */
    const int64_t* seg_off;     /* [R * K] (+ 1 without seg_len) */
    const int32_t* seg_len;     /* [R * K] or NULL */
    int64_t max_len, cap;
    int32_t aligned16;          /* the caller's word that every retained run starts 16-byte aligned */
    void* chist;                /* [R][hist_stride] elements of NVRX_CHIST_BYTES, in place */
    int64_t hist_stride;        /* in elements; 0: K */
    const int32_t* hist_index;  /* [K] or NULL */
    const uint8_t* col_valid;   /* [K] or NULL */
    const uint8_t* skip_rows;   /* [R] or NULL */
    int32_t permille;
    int32_t mode;               /* NVRX_HTAIL_SCORE | NVRX_HTAIL_UPDATE */
    double score_thr;
    uint64_t* tail_ns;          /* [R] */
    uint64_t* total_ns;         /* [R] */
    uint64_t* base_tail_ns;     /* [R] */
    uint64_t* base_total_ns;    /* [R] */
    double* score;              /* [R] */
    uint8_t* strag;             /* [R] or NULL */
    uint32_t* tail_calls;       /* [R][K] or NULL */
    uint64_t* folded;           /* [R]; required with UPDATE */
} nvrx_segchist_args;
int nvrx_segment_history_scores_compact_ragged(const nvrx_segchist_args* args, void* stream);

/* The individual tail score attribution of record streams against the compact history: what
 * nvrx_segment_history_attribution_ragged is to the dense history.  No reference counterpart.
 * nvrx_segchistattr_args has the fields of nvrx_seghistattr_args in the same order, with `const
 * void* chist` ([R][hist_stride] elements of NVRX_CHIST_BYTES, read only) in the place of hist and
 * hist_stride in elements.  By definition
 *   nvrx_segment_history_attribution_compact_ragged  writes into idx, loss, tail_ns, total_ns,
 *     tail_calls, thr_bucket, base_share ([R][top]) and loss_all ([R][K], written in full) what is
 *     equal, bit for bit, to what nvrx_segment_history_attribution_ragged writes with hist the
 *     dense expansion of chist (H[bucket[i]] = count[i] for i < n, zero elsewhere) and the same
 *     segments, max_len, cap, aligned16, hist_index, col_valid, permille and top: an element
 *     (r, k) is taken iff col_valid[k] != 0, its slot s >= 0, the element's N = sum of count > 0,
 *     its retained length is > 0 and its loss is not NaN.
 * Canonical input is assumed.  chist is READ ONLY here, and the content of the slots no column
 * uses never influences an output: between a SCORE call and an UPDATE call of
 * nvrx_segment_history_scores_compact_ragged the entry sees the history the score saw.  An element
 * that is not valid, has no slot or an empty segment is not read.  Argument checks as for
 * nvrx_segment_history_attribution_ragged, except that chist must be 16-byte aligned, the
 * null-pointer message names chist and there is no K * 240 limit; R * K stays below 2^31.  R == 0
 * or K == 0 launches nothing (outputs untouched).  Two kernels on `stream` only (every (r, k) has
 * one owner): no allocation, no synchronisation, no host read-back, no scratch, no atomics, no
 * clear; capturable as a linear chain with the calls around it. */
typedef struct nvrx_segchistattr_args {
    int64_t R, K;
    const uint32_t* ns;         /* duration keys */
    const int64_t* seg_off;     /* [R * K] (+ 1 without seg_len) */
    const int32_t* seg_len;     /* [R * K] or NULL */
    int64_t max_len, cap;
    int32_t aligned16;          /* the caller's word that every retained run starts 16-byte aligned */
    int32_t top;                /* 1..NVRX_MAX_ATTRIBUTION */
    const void* chist;          /* [R][hist_stride] elements of NVRX_CHIST_BYTES, read only */
    int64_t hist_stride;        /* in elements; 0: K */
    const int32_t* hist_index;  /* [K] or NULL */
    const uint8_t* col_valid;   /* [K] or NULL */
    int32_t permille;
    int32_t* idx;               /* [R][top] */
    double* loss;               /* [R][top] */
    uint64_t* tail_ns;          /* [R][top] */
    uint64_t* total_ns;         /* [R][top] */
    uint32_t* tail_calls;       /* [R][top] */
    int32_t* thr_bucket;        /* [R][top] */
    double* base_share;         /* [R][top] */
    double* loss_all;           /* [R][K] */
} nvrx_segchistattr_args;
int nvrx_segment_history_attribution_compact_ragged(const nvrx_segchistattr_args* args, void* stream);

/* Aging the tail histories: every count shifted right by `shift` bits (halved for shift = 1), so
 * that a history forgets.  No reference counterpart.  Both histories only grow otherwise: counts
 * add up until they saturate, and a compact element that has used its 12 entries folds every
 * further bucket downwards.  Aging concerns SLOTS, not columns: every slot of [R][stride] is
 * aged, and there is no hist_index and no col_valid.
 *
 *   nvrx_compact_history_age    chist[R][stride] elements of NVRX_CHIST_BYTES ("Element layout"
 *     above), in place.  Per element, with s = shift in 1..31:
 *       count'[i] = count[i] >> s for i < n;
 *       the entries with count' >= 1 are kept in their order (the buckets stay strictly
 *       ascending) and moved to the front; n' is their number; entries n'..11 are all zero,
 *       bucket bytes included.
 *     Canonical input gives canonical output; an element whose entries are all evicted becomes
 *     the all-zero (empty) element; an element with n = 0 is not written.  Only the count decides
 *     whether an entry is used: bucket byte 0 with a count >= 1 is the used bucket 0.
 *     evicted[r] (u64, [R] or NULL) is the number of entries freed in row r, the sum of n - n';
 *     full[r] (u64, [R] or NULL) the number of elements of row r with n' = 12 after aging.  Both
 *     are cleared on the stream first and must not alias each other.
 *   nvrx_histogram_history_age  the dense u32 hist[R][stride][NVRX_HIST_BINS], in place: every
 *     word becomes word >> s.  No outputs.
 * Aging commutes with the dense expansion: the expansion of the aged compact history is the aged
 * expansion, so the bit-identity between the two histories (while nothing folds) survives aging;
 * aging by s and then by t is aging by s + t.
 *
 * chist / hist 16-byte aligned; evicted and full 8-byte aligned; shift in 1..31; R * stride below
 * 2^31; for the dense entry also stride * 240 below 2^31 and R * stride * 240 / 4, the 16-byte
 * vectors of the pass, below 2^31.  R == 0 or stride == 0 launches nothing (outputs untouched).
 * Stream-ordered: kernels on `stream` only (a clear of the row outputs when one is given, and
 * the pass), no allocation, no synchronisation, no host read-back, no scratch, no atomics on a
 * history (the non-zero row sums are added with 64-bit integer atomics, which commute: every run
 * gives the same result); capturable as a linear chain. */
int nvrx_compact_history_age(void* chist, int64_t R, int64_t stride, int32_t shift,
                             uint64_t* evicted, uint64_t* full, void* stream);
int nvrx_histogram_history_age(uint32_t* hist, int64_t R, int64_t stride, int32_t shift, void* stream);

/* The individual tail scores of [R][K][240] counts against the COMPACT history: the fourth corner
 * of {counts, record streams} x {dense, compact history}.  No reference counterpart.  It adds no
 * definition; it composes two that stand above.  nvrx_histchist_args has the fields of
 * nvrx_histtail_args in the same order, with `void* chist` ([R][hist_stride] elements of
 * NVRX_CHIST_BYTES, "Element layout" above, changed in place) in the place of hist, hist_stride in
 * elements, and folded at the end.  counts, hist_index, col_valid, skip_rows, permille, mode and
 * score_thr mean exactly what they do for nvrx_histogram_history_scores.
 *   SCORE   is nvrx_histogram_history_scores's SCORE with H the dense expansion of the element
 *           before the call (H[bucket[i]] = count[i] for i < n, zero elsewhere): eligibility
 *           (col_valid, slot >= 0, N > 0, sum_b C > 0), T, the four u64 sums, tail_calls (0 where
 *           not eligible), the three separately rounded f64 operations and the strict strag.
 *   UPDATE  is the compact history's UPDATE ("compact history" above) with c[b] = C[r][k][b]:
 *           admission of the new buckets in ascending order while entries are free, the target
 *           t(b) for every other bin, count' = min(count + sum c, 2^32 - 1) with the sum taken in 64
 *           bits -- every c[b] is a full u32 here and up to 240 of them fold into one entry -- and
 *           folded[r].  It applies to every (r, k) with col_valid[k], a slot >= 0, skip_rows[r] = 0
 *           and sum_b C[r][k][b] > 0; an element without samples is not written.
 *   SCORE | UPDATE scores against the history from before the update.
 * One history can be continued by this entry and nvrx_segment_history_scores_compact_ragged alike:
 * on the counts nvrx_segment_histogram_ragged writes for the same segments both leave the same
 * bytes, folded and outputs.  While nothing folds, the dense expansion and every output equal
 * nvrx_histogram_history_scores's on the dense history bit for bit.
 * counts and chist 16-byte aligned; the four u64 outputs, score and folded 8-byte aligned; mode
 * needs at least one bit; permille in 0..1000; hist_stride 0 or, without hist_index, at least K;
 * K * 240 and R * K below 2^31.  folded is required with UPDATE and must not alias the other
 * outputs.  Two columns must not share a slot, and counts and chist must not overlap (neither is
 * checked).  Canonical input is assumed.  R == 0 or K == 0 launches nothing.  Stream-ordered:
 * kernels on `stream` only (a clear, the pass, with SCORE a finalize), no allocation, no
 * synchronisation, no host read-back, no scratch, no atomics on the history; capturable as a
 * linear chain. */
typedef struct nvrx_histchist_args {
    int64_t R, K;
    const uint32_t* counts;     /* [R][K][NVRX_HIST_BINS] */
    void* chist;                /* [R][hist_stride] elements of NVRX_CHIST_BYTES, in place */
    int64_t hist_stride;        /* in elements; 0: K */
    const int32_t* hist_index;  /* [K] or NULL */
    const uint8_t* col_valid;   /* [K] or NULL */
    const uint8_t* skip_rows;   /* [R] or NULL */
    int32_t permille;
    int32_t mode;               /* NVRX_HTAIL_SCORE | NVRX_HTAIL_UPDATE */
    double score_thr;
    uint64_t* tail_ns;          /* [R] */
    uint64_t* total_ns;         /* [R] */
    uint64_t* base_tail_ns;     /* [R] */
    uint64_t* base_total_ns;    /* [R] */
    double* score;              /* [R] */
    uint8_t* strag;             /* [R] or NULL */
    uint32_t* tail_calls;       /* [R][K] or NULL */
    uint64_t* folded;           /* [R]; required with UPDATE */
} nvrx_histchist_args;
int nvrx_histogram_history_scores_compact(const nvrx_histchist_args* args, void* stream);

/* Conversion between the dense history hist[R][stride][NVRX_HIST_BINS] (u32) and the compact
 * history chist[R][stride] elements of NVRX_CHIST_BYTES, slot by slot.  No reference counterpart.
 *   nvrx_compact_history_from_dense  chist[r][s] = the UPDATE of the empty element with
 *     c[b] = hist[r][s][b]: the 12 lowest used buckets are kept, every bucket above them folds
 *     into the 12th (the sum taken in 64 bits, saturating at 2^32 - 1).  folded[r] (u64, [R] or
 *     NULL; cleared on the stream first) is the number of samples folded in row r.  Every element
 *     is written in full -- an empty dense element gives the all-zero element -- so the target
 *     needs no clear.
 *   nvrx_compact_history_to_dense    hist[r][s] = the dense expansion of chist[r][s]
 *     (H[bucket[i]] = count[i] for i < n, zero elsewhere).  All 240 bins of every element are
 *     written, so the target needs no clear.  Canonical input is assumed.
 * to_dense(from_dense(H)) == H exactly when no element of H uses more than 12 buckets, and
 * from_dense(to_dense(c)) == c for every canonical c.  The two buffers must not overlap (not
 * checked).  hist and chist 16-byte aligned; folded 8-byte aligned; stride * 240 and R * stride
 * below 2^31.  R == 0 or stride == 0 launches nothing (folded untouched).  Stream-ordered: kernels
 * on `stream` only, no allocation, no synchronisation, no host read-back, no scratch, no atomics
 * on a history (the non-zero folded sums are added with 64-bit integer atomics, which commute);
 * capturable as a linear chain. */
int nvrx_compact_history_from_dense(const uint32_t* hist, void* chist, int64_t R, int64_t stride,
                                    uint64_t* folded, void* stream);
int nvrx_compact_history_to_dense(const void* chist, uint32_t* hist, int64_t R, int64_t stride,
                                  void* stream);

/* The individual tail score attribution of [R][K][240] counts against the COMPACT history: what
 * nvrx_histogram_tail_attribution(kind = NVRX_ATTR_INDIVIDUAL) is to the dense history, and the
 * fourth corner of the attributions over {counts, record streams} x {dense, compact history}.  No
 * reference counterpart.  It adds no definition.  nvrx_histchistattr_args has counts and top, then
 * `const void* chist` ([R][hist_stride] elements of NVRX_CHIST_BYTES, "Element layout" above, read
 * only) with hist_stride in elements, hist_index, col_valid and permille, then the eight outputs
 * of nvrx_tailattr_args with the same meaning.  By definition
 *   nvrx_histogram_history_attribution_compact  writes into idx, loss, tail_ns, total_ns,
 *     tail_calls, thr_bucket, base_share ([R][top]) and loss_all ([R][K], written in full) what is
 *     equal, bit for bit, to what nvrx_histogram_tail_attribution writes with kind =
 *     NVRX_ATTR_INDIVIDUAL, hist the dense expansion of chist (H[bucket[i]] = count[i] for i < n,
 *     zero elsewhere) and the same counts, hist_index, col_valid, permille and top: an element
 *     (r, k) is taken iff col_valid[k] != 0, its slot s >= 0, the element's N = sum of count > 0,
 *     sum_b C[r][k][b] > 0 and its loss is not NaN.
 * On the counts nvrx_segment_histogram_ragged writes for the same segments it equals
 * nvrx_segment_history_attribution_compact_ragged.  Canonical input is assumed.  chist is READ
 * ONLY here, and the content of the slots no column uses never influences an output: between a
 * SCORE call and an UPDATE call of nvrx_histogram_history_scores_compact the entry sees the history
 * the score saw.  A column that is not valid or has no slot is not read, neither its element nor
 * its counts.
 * counts and chist 16-byte aligned; the f64 and u64 outputs 8-byte aligned; top in
 * 1..NVRX_MAX_ATTRIBUTION; permille in 0..1000; hist_stride 0 or, without hist_index, at least K;
 * K * 240 and R * K below 2^31.  R == 0 or K == 0 launches nothing (outputs untouched).
 * Stream-ordered: two kernels on `stream` only (every (r, k) has one owner): no allocation, no
 * synchronisation, no host read-back, no scratch, no atomics, no clear; capturable as a linear
 * chain with the calls around it. */
typedef struct nvrx_histchistattr_args {
    int64_t R, K;
    const uint32_t* counts;     /* [R][K][NVRX_HIST_BINS] */
    int32_t top;                /* 1..NVRX_MAX_ATTRIBUTION */
    const void* chist;          /* [R][hist_stride] elements of NVRX_CHIST_BYTES, read only */
    int64_t hist_stride;        /* in elements; 0: K */
    const int32_t* hist_index;  /* [K] or NULL */
    const uint8_t* col_valid;   /* [K] or NULL */
    int32_t permille;
    int32_t* idx;               /* [R][top] */
    double* loss;               /* [R][top] */
    uint64_t* tail_ns;          /* [R][top] */
    uint64_t* total_ns;         /* [R][top] */
    uint32_t* tail_calls;       /* [R][top] */
    int32_t* thr_bucket;        /* [R][top] */
    double* base_share;         /* [R][top] */
    double* loss_all;           /* [R][K] */
} nvrx_histchistattr_args;
int nvrx_histogram_history_attribution_compact(const nvrx_histchistattr_args* args, void* stream);

/* Rank attribution: the ranks behind a kernel's tail loss.  No reference counterpart.  The tail
 * attributions above name, per row, the kernels that cost a rank its score, and leave loss_all[R][K]
 * on the device.  This reads such a matrix column-wise: per kernel, the `top` ranks that lose the
 * most time on it, and how many lose any.  The definition is part of the ABI.
 * Input:  loss       f64 [R][ld], row-major, ld >= K (0: K), 8-byte aligned
 *         row_valid  u8 [R] or NULL: a row with row_valid[r] == 0 counts as not taken for every
 *                    column (the `strag` output of a score call, passed straight in)
 *         top        1..NVRX_MAX_ATTRIBUTION
 * An element (r, k) is TAKEN iff its row is valid and loss[r][k] is not NaN.  Outputs, per column k:
 *     idx[k][j]       i32 [K][top]: the row of the j-th largest taken loss.  Ties go to the lower
 *                     row; -0.0 and +0.0 tie; +-inf and negative losses order like any value; -1
 *                     beyond the taken elements
 *     loss_out[k][j]  f64 [K][top]: that element's bits as they stand in the input (re-read, never
 *                     rebuilt from a sort key: -0.0 stays -0.0); NaN where idx = -1
 *     taken[k]        i32: the number of taken elements
 *     positive[k]     i32: the number of taken elements with loss > 0.0 (the ranks that lost time
 *                     on the kernel at all)
 * No f64 column sums: they would depend on the order of the additions.
 * nvrx_rank_attribution_plan: pure host function, the launch plan of a shape: tiles (workgroups
 *   along K, 64 columns each), splits (>= 1: workgroups along R; 1 means one kernel that writes the
 *   outputs, more a second kernel that merges the splits' partial lists) and work_bytes (0 with one
 *   split).  work_bytes does not decrease as R or top grow with the other two fixed.  R == 0 or
 *   K == 0: tiles 0, splits 1, work_bytes 0.  Any output pointer may be NULL.  Negative R or K or a
 *   top out of range is an error.  One plan serves both entries: nvrx_score_rank_attribution
 *   (below) launches the same grid and sizes and lays out `work` the same way.
 * nvrx_rank_attribution: `work` is device memory of at least work_bytes, 8-byte aligned (may be
 *   NULL when work_bytes is 0); its content is unspecified afterwards.  R * ld below 2^31.  R == 0
 *   or K == 0 launches nothing and leaves the outputs untouched.  A top out of range, ld below K, a
 *   missing loss or output, a missing work where the plan needs one, or a misaligned loss, loss_out
 *   or work is an error.  Stream-ordered: one or two kernels on `stream` only (every (column,
 *   split) has one owner): no allocation, no synchronisation, no host read-back, no atomics, no
 *   clear, no scratch; capturable as a linear chain with the calls around it.  Two calls on the
 *   same input write the same bytes. */
typedef struct nvrx_rankattr_args {
    int64_t R, K;
    const double* loss;         /* [R][ld] */
    int64_t ld;                 /* row stride in elements; 0: K */
    const uint8_t* row_valid;   /* [R] or NULL */
    int32_t top;                /* 1..NVRX_MAX_ATTRIBUTION */
    int32_t* idx;               /* [K][top] */
    double* loss_out;           /* [K][top] */
    int32_t* taken;             /* [K] */
    int32_t* positive;          /* [K] */
    void* work;                 /* work_bytes of nvrx_rank_attribution_plan, or NULL when 0 */
} nvrx_rankattr_args;
int nvrx_rank_attribution_plan(int64_t R, int64_t K, int32_t top, int64_t* tiles, int64_t* splits,
                               int64_t* work_bytes);
int nvrx_rank_attribution(const nvrx_rankattr_args* args, void* stream);

/* ---------------------------------------------------------------- scoring */
/* ref[k] = min over r of med[r][k] if num[r][k] > 0 for every r, else NaN.
 * scratch: >= 2*K uint32 of device memory. */
int nvrx_kernel_ref(const int32_t* num, const float* med, int64_t R, int64_t K, float* ref,
                    uint32_t* scratch, void* stream);
/* times[0:total] = -1; times[ids[i]] = float32(med[i]) for i < n: the float32 pack of
 * _all_reduce_times (kernel ids first, section ids offset by the kernel count). */
int nvrx_pack_min_times(const double* med, const int32_t* ids, int64_t n, float* times,
                        int64_t total, void* stream);
int nvrx_scores(const nvrx_score_args* args, void* stream);
/* partials: [nshards][R][6], combined in shard order 0..nshards-1.
 * score = n > 0 ? sum(s*w)/sum(w) : NaN; round_f32 != 0 rounds to float32 (the
 * gather_on_rank0 tensor); err |= 2 when n > 0 and sum(w) == 0.
 * Any output pointer may be NULL. strag_* = score < thr (strict; NaN never). */
int nvrx_finalize_scores(const double* partials, int64_t R, int64_t nshards, int32_t round_f32,
                         double thr_rel, double thr_ind, double* gpu_rel, double* gpu_ind,
                         uint8_t* strag_rel, uint8_t* strag_ind, int32_t* err, void* stream);
/* Sections, R rows x S sections: med [R][S] f64, present [R][S] u8.
 * rel: ref_s = min over rows of float32(med) when ref_in == NULL (every row must be
 *      present, else NaN; computed into ref_work [S]), or ref_in[ref_index ? ref_index[s] : s]
 *      (float32, !(>= 0) = missing => NaN score);
 * ind: hist[R][S] f64 updated to min(hist, med) first.
 * out_rel / out_ind [R][S] f64 (NaN where absent); round_f32 as above.  Either may be NULL;
 * err |= 1 when a present med == 0 (ZeroDivisionError). */
int nvrx_section_scores(const double* med, const uint8_t* present, int64_t R, int64_t S,
                        const float* ref_in, const int32_t* ref_index, float* ref_work,
                        double* hist, int32_t round_f32, double* out_rel, double* out_ind,
                        int32_t* err, void* stream);
int nvrx_stragglers(const double* score, int64_t n, double thr, uint8_t* mask, void* stream);

/* Score attribution: the kernels behind a rank's GPU score.  No reference counterpart (the
 * reference reports the score alone).  The score of a row is sum_k s_k*w_k / sum_k w_k with
 * s_k = base_k / MED_k and w_k = NUM_k * AVG_k (base: the relative reference or the individual
 * history), so
 *     1 - score = sum_k w_k * (1 - s_k) / sum_k w_k
 * and loss_k = w_k * (1 - s_k) is the time (us, weighted as the score weights it) the rank lost
 * on kernel k against its base.  Per row the call returns the `top` largest losses.
 * Inputs: the fields of nvrx_score_args with the same meaning; `kind` selects the base
 * (NVRX_ATTR_RELATIVE: ref / ref_index / ref_missing; NVRX_ATTR_INDIVIDUAL: hist / hist_index /
 * hist_stride).  The history is READ ONLY here: it is taken as the report's nvrx_scores left it
 * (already min(hist, MED)).  An element is eligible exactly when nvrx_scores adds it to the sum
 * of that kind (col_valid NULL or nonzero, num > 0; relative: ref >= 0 and not missing).  An
 * eligible element with MED == 0 sets *err |= 1 and is left out; one whose loss is NaN (a NaN
 * AVG, say) is left out like an absent kernel; what is left out adds nothing to wsum either.
 * Per element, in f64 with separately rounded operations:
 *     m = MED;  w = NUM * AVG;  s = base / m;  loss = w * (1.0 - s)
 * Outputs, row-major, j < top (1 <= top <= NVRX_MAX_ATTRIBUTION):
 *     idx[r][j]    column of the j-th largest loss (ties: the lower column first; -0.0 == +0.0),
 *                  -1 beyond the number of elements taken
 *     loss[r][j]   its loss (negative when a caller's reference exceeds MED); NaN where idx = -1
 *     score[r][j]  its s; NaN where idx = -1
 *     wsum[r]      sum of w over the elements taken, in a fixed order (run-to-run identical);
 *                  may be NULL, as may err
 * K < 2^31.  R == 0 or K == 0 launches nothing (the outputs are untouched).  Stream-ordered: kernels on `stream` only, no allocation, no
 * synchronisation (capturable in a graph). */
#define NVRX_MAX_ATTRIBUTION 16
#define NVRX_ATTR_RELATIVE 0
#define NVRX_ATTR_INDIVIDUAL 1
typedef struct nvrx_attribution_args {
    int64_t R, K;
    int32_t value_f64;
    const int32_t* num;
    const void* med;
    const void* avg;
    const uint8_t* col_valid;
    const float* ref;
    const int32_t* ref_index;
    const uint32_t* ref_missing;
    const void* hist;
    const int32_t* hist_index;
    int64_t hist_stride;
    int32_t kind, top;
    int32_t* idx;   /* [R][top] */
    double* loss;   /* [R][top] */
    double* score;  /* [R][top] */
    double* wsum;   /* [R] or NULL */
    int32_t* err;   /* [1] or NULL */
} nvrx_attribution_args;
int nvrx_score_attribution(const nvrx_attribution_args* args, void* stream);

/* Score rank attribution: the ranks behind a kernel's score loss.  No reference counterpart.  The
 * converse of "Score attribution" above, as "Rank attribution" is the converse of the tail
 * attributions: per kernel, the `top` ranks that lose the most on it, and how many lose anything.
 * The definition is part of the ABI.
 * Inputs: the input fields of nvrx_attribution_args with the same meaning (R, K, value_f64, num,
 * med, avg, col_valid, ref, ref_index, ref_missing, hist, hist_index, hist_stride, kind); the
 * history is READ ONLY.  row_valid u8 [R] or NULL and top as in nvrx_rankattr_args.
 * Let L[r][k] be the element's loss exactly as nvrx_score_attribution defines it (f64, every
 * operation rounded separately:  m = MED;  w = NUM * AVG;  s = base / m;  loss = w * (1.0 - s))
 * where nvrx_score_attribution would take the element -- it is eligible for `kind`, MED != 0 and
 * the loss is not NaN -- and NaN where it would not.  An eligible element with MED == 0 in a row
 * that is valid sets *err |= 1 (err may be NULL; it is not written otherwise).  Outputs:
 *     idx [K][top], loss [K][top], taken [K], positive [K]   equal, bit for bit, to what
 *                     nvrx_rank_attribution writes for the matrix L with the same row_valid and top
 *                     (ties to the lower row, -0.0 ties with +0.0, -1 / NaN beyond the taken)
 *     score [K][top]  f64: the winner's s; NaN where idx = -1
 * The stored loss and score are recomputed from the inputs at the winner's (row, column), never
 * rebuilt from a sort key: a -0.0 loss stays -0.0.  No f64 column sums: they would depend on the
 * order of the additions.  L itself is never stored.
 * ONE PLAN SERVES BOTH ENTRIES: the grid and `work` are those of nvrx_rank_attribution_plan(R, K,
 * top) -- same tiles, same splits, same work_bytes, same layout of the partial lists.  `work` is
 * device memory of at least work_bytes, 8-byte aligned (may be NULL when work_bytes is 0); its
 * content is unspecified afterwards.  R and K below 2^31.  R == 0 or K == 0 launches nothing and
 * leaves the outputs untouched.  A top or kind out of range, a missing input or output, a kind
 * without its base, hist_index without hist_stride, a missing work where the plan needs one, or a
 * misaligned loss, score or work is an error.  Stream-ordered: one or two kernels on `stream` only:
 * no allocation, no synchronisation, no host read-back, no clear, no scratch, no atomics other than
 * the OR into err; capturable as a linear chain with the calls around it.  Two calls on the same
 * inputs write the same bytes whatever `work` held. */
typedef struct nvrx_scorerank_args {
    int64_t R, K;
    int32_t value_f64;
    const int32_t* num;
    const void* med;
    const void* avg;
    const uint8_t* col_valid;
    const float* ref;
    const int32_t* ref_index;
    const uint32_t* ref_missing;
    const void* hist;
    const int32_t* hist_index;
    int64_t hist_stride;
    int32_t kind, top;
    const uint8_t* row_valid;   /* [R] or NULL */
    int32_t* idx;               /* [K][top] */
    double* loss;               /* [K][top] */
    double* score;              /* [K][top] */
    int32_t* taken;             /* [K] */
    int32_t* positive;          /* [K] */
    int32_t* err;               /* [1] or NULL */
    void* work;                 /* work_bytes of nvrx_rank_attribution_plan, or NULL when 0 */
} nvrx_scorerank_args;
int nvrx_score_rank_attribution(const nvrx_scorerank_args* args, void* stream);

/* Statistics of section CPU timings (ms, float64): section s = vals[off[s] : off[s+1]]
 * (off: [nsec+1], device).  MIN, MAX, MED = lower median s[(n-1)/2] (torch.median),
 * AVG, STD = unbiased (NaN for n == 1), NUM -- Detector._get_section_summaries
 * (straggler.py:171-197).  max_len bounds every section's length (any length: sections
 * longer than 16384 timings are sorted in a device scratch buffer instead of LDS). */
int nvrx_section_stats(const double* vals, const int64_t* off, int64_t nsec, int64_t max_len,
                       int32_t* num, double* mn, double* mx, double* med, double* avg,
                       double* sd, void* stream);

/* ---------------------------------------------------------------- record streams */
/* A record is one kernel execution: the slot of its composite kernel name and its duration
 * key (end - start, CuptiProfiler.cpp:187; nvrx_duration_key above 3.76 s). */
typedef struct nvrx_record {
    uint32_t slot;
    uint32_t ns;
} nvrx_record;

/* Bucket nstreams push-ordered record streams (stream t = recs[rec_off[t] : rec_off[t+1]],
 * one per rank) by slot, keeping for every (stream, slot) only its LAST `cap` records
 * (CircularBuffer semantics; order inside a bucket is push order).  Outputs (device):
 *   seg_off [nstreams*nslots] int64, seg_len [nstreams*nslots] int32:
 *       bucket (t, s) = out_ns[seg_off[t*nslots+s] : + seg_len[t*nslots+s]]; every bucket
 *       starts 16-byte aligned, so it feeds nvrx_segment_stats_ragged(aligned16=1); where a
 *       stream's buckets lie inside its region is unspecified (slots with few records are
 *       laid out first and assembled in LDS)
 *   out_ns  [>= nvrx_records_bucket_capacity(n, nstreams, nslots)] uint32, 16-byte aligned
 *   counts  [nstreams*nslots] int32: total pushes per (stream, slot) on return */
int64_t nvrx_records_bucket_capacity(int64_t n, int64_t nstreams, int64_t nslots);
int nvrx_records_bucket(const nvrx_record* recs, const int64_t* rec_off, int64_t nstreams,
                        int64_t nslots, int64_t cap, int64_t* seg_off, int32_t* seg_len,
                        uint32_t* out_ns, int32_t* counts, void* stream);
/* The whole per-(stream, slot) statistics of record streams (ring retention +
 * CuptiProfiler::getStats for every stream): nvrx_records_bucket, then
 * nvrx_segment_stats_ragged(aligned16) over the buckets (runs of <= 128 samples bit-exact in
 * every field).  out->* are [nstreams*nslots]; max_len bounds every stream's length
 * (host-known); col_ref (optional, [2*nslots]) as for nvrx_segment_stats_strided (rows =
 * streams), produced by a column reduction; counts may be NULL here (the pushes per bucket are
 * then not written: 4 B per (stream, slot) less).  On return seg_len[g] < 0 marks a bucket of
 * -seg_len[g] records whose statistics the bucketing kernel computed itself; neither its
 * seg_off[g] nor its records in out_ns are written. */
int nvrx_records_stats(const nvrx_record* recs, const int64_t* rec_off, int64_t nstreams,
                       int64_t nslots, int64_t cap, int32_t mode, int64_t max_len, int64_t* seg_off,
                       int32_t* seg_len, uint32_t* out_ns, int32_t* counts,
                       const nvrx_stats_soa* out, uint32_t* col_ref, void* stream);
/* Slots one bucketing pass counts (its per-slot counters live in LDS).  Any nslots is accepted:
 * a larger slot table is bucketed in passes over ranges of this many slots, each re-reading the
 * streams (the reference's per-kernel map is unbounded, CuptiProfiler.cpp:189-198);
 * nvrx_records_bucket_capacity accounts for the passes' regions of out_ns. */
int64_t nvrx_records_max_slots(void);

/* ---------------------------------------------------------------- profiler handle */
/* Replacement of nvrx_cupti_module.CuptiProfiler: owns device-resident per-kernel
 * duration records; only one instance may exist (CuptiProfiler.cpp:83-90). */
typedef struct nvrx_profiler nvrx_profiler;

typedef struct nvrx_profiler_config {
    int64_t buffer_size;              /* bytes of host record buffer per flush (CUPTI bufferSize) */
    int64_t num_buffers;              /* CUPTI numBuffers (kept for API parity) */
    int64_t stats_max_len_per_kernel; /* ring capacity per kernel (statsMaxLenPerKernel) */
    int32_t device;                   /* HIP device ordinal */
    int32_t mode;                     /* NVRX_STATS_EXACT (default) or NVRX_STATS_FAST */
} nvrx_profiler_config;

int nvrx_profiler_create(const nvrx_profiler_config* cfg, nvrx_profiler** out);
int nvrx_profiler_destroy(nvrx_profiler* p);
int nvrx_profiler_initialize(nvrx_profiler* p);
int nvrx_profiler_shutdown(nvrx_profiler* p);
int nvrx_profiler_start(nvrx_profiler* p);
int nvrx_profiler_stop(nvrx_profiler* p);
int nvrx_profiler_reset(nvrx_profiler* p);
/* Register a composite kernel name ("%s_blk_%d_%d_%d_grid_%d_%d_%d") -> slot. */
int nvrx_profiler_register_kernel(nvrx_profiler* p, const char* name, uint32_t* slot);
/* Slots are valid until the next nvrx_profiler_reset, which forgets every kernel (the
 * reference clears its per-kernel map, CuptiProfiler.cpp:148-152): names are registered again
 * (from slot 0) in the next report interval. */
/* Append host records (push order).  Ignored while stopped (records are dropped).  Staged
 * host records move to the device log once buffer_size bytes of them wait (and at every
 * get_stats / get_records / reset). */
int nvrx_profiler_push(nvrx_profiler* p, const nvrx_record* recs, int64_t n);
/* Slot-numbering generation: bumped by every nvrx_profiler_reset (slots are renumbered from 0
 * after it).  A caller that builds device records from registered slots reads it after
 * registering and passes it to nvrx_profiler_ingest. */
int nvrx_profiler_generation(nvrx_profiler* p, uint64_t* generation);
/* Append n DEVICE records (push order, after every record staged before) to the device log:
 * one copy kernel enqueued on `stream`, so dev_recs must stay valid until that stream reaches
 * it; later profiler calls order themselves after it.  Ignored while stopped.  `generation`
 * must be the current nvrx_profiler_generation (NVRX_ERR_STATE otherwise: the slots were
 * numbered before a reset).  Records whose slot is not registered at this call are dropped
 * (never counted, even if that slot number is handed out later).  The copy is the library's
 * own kernel: a live capture leaves it out.  No
 * reference counterpart: the device-side entry of an external tracer (SURVEY 8(b)
 * nvrx_ingest_records). */
int nvrx_profiler_ingest(nvrx_profiler* p, const nvrx_record* dev_recs, int64_t n,
                         uint64_t generation, void* stream);
/* *count = captured / pushed durations of 3.76 s or more (stored as wide keys, nothing lost)
 * since the last reset: a diagnostic of hung or very long kernels. */
int nvrx_profiler_saturated(nvrx_profiler* p, int64_t* count);
/* Flush, then compute stats of every slot with >= 1 record.  Synchronous.
 * Returns the number of kernels in *count; fills up to `cap_out` entries of slots
 * (sorted by kernel name, as std::map in getStats) and host SoA outputs.  The result is
 * cached: a size query (cap_out = 0) followed by the copying call computes once, unless
 * records arrived in between. */
int nvrx_profiler_get_stats(nvrx_profiler* p, int64_t cap_out, int64_t* count, uint32_t* slots,
                            int32_t* num, float* mn, float* mx, float* med, float* avg,
                            float* sd);
int nvrx_profiler_kernel_name(nvrx_profiler* p, uint32_t slot, char* buf, int64_t buflen);
/* Flush, then the quantiles (nvrx_segment_quantiles_ragged) of every slot with >= 1 record, over
 * the records its ring retains.  Synchronous.  *count = number of kernels; fills up to cap_out
 * entries of slots (sorted by kernel name, like get_stats), num (retained records) and out
 * ([nq][cap_out] host f32 us: quantile j of entry i at out[j * cap_out + i]).  The record log and
 * get_stats' cached result are left as they are; the call's own kernels are not captured.  No
 * reference counterpart: CuptiProfiler::getStats has no quantile beyond the median. */
int nvrx_profiler_get_quantiles(nvrx_profiler* p, const int32_t* permille, int32_t nq,
                                int64_t cap_out, int64_t* count, uint32_t* slots, int32_t* num,
                                float* out);
/* Flush, then the histogram (nvrx_segment_histogram_ragged) of every slot with >= 1 record, over
 * the records its ring retains.  Synchronous.  *count = number of kernels; fills up to cap_out
 * entries of slots (sorted by kernel name, like get_stats), num (retained records) and out
 * ([cap_out][NVRX_HIST_BINS] host u32: bin b of entry i at out[i * 240 + b]).  The record log and
 * get_stats' cached result are left as they are; the call's own kernels are not captured. */
int nvrx_profiler_get_histograms(nvrx_profiler* p, int64_t cap_out, int64_t* count,
                                 uint32_t* slots, int32_t* num, uint32_t* out);
/* Flush, then copy the record log since the last reset ({slot, ns}, push order per slot;
 * after a compaction only the records the rings can still retain) into host `out`
 * (up to cap_out records; *count = log length).  Synchronous.  No reference counterpart:
 * it lets a caller (the live-capture parity check) recompute the statistics elsewhere. */
int nvrx_profiler_get_records(nvrx_profiler* p, int64_t cap_out, int64_t* count,
                              nvrx_record* out);
/* Live kernel-dispatch capture (CuptiProfiler.cpp:96-203).  nvrx_capture_configure registers
 * the library as a rocprofiler-sdk tool; it must run before the process's first HIP call
 * (NVRX_ERR_STATE otherwise).  Once the runtime has initialised, nvrx_profiler_capture_available()
 * returns 1 and every kernel enqueued while a profiler handle is started is pushed into it, once it
 * has completed, under the reference's composite key "%s_blk_%d_%d_%d_grid_%d_%d_%d" (mangled name,
 * block dims, grid dims in blocks, a partial last block counted) with its integer-ns duration;
 * nvrx_profiler_stop / _get_stats flush the capture first.  By default the runtime's HSA queues are
 * intercepted and each dispatch gets a completion record in device memory (NVRX_CAPTURE_DELIVERY=
 * queue); callback / buffer / callback_counted use rocprofiler-sdk's kernel-dispatch tracing.  As CUPTI_ACTIVITY_KIND_CONCURRENT_KERNEL does (CuptiProfiler.cpp:118,
 * 179), copies and fills are not kernels: the ROCm runtime's blit kernels ("__amd_rocclr_*",
 * which carry out hipMemcpy* / hipMemset*) are left out unless NVRX_CAPTURE_RUNTIME_KERNELS=1. */
int nvrx_capture_configure(void);
int nvrx_profiler_capture_available(void);
/* Deliver the dispatch records completed so far to the started / stopped profiler
 * (cuptiActivityFlushAll(0), CuptiProfiler.cpp:138).  Synchronous; no-op without capture. */
int nvrx_capture_flush(void);
/* Cost accounting of the live capture since configuration (process-wide, monotone): delivery
 * callbacks (queue delivery: harvests), records in them, dispatch records handed to a profiler,
 * wall time spent inside this library's delivery callbacks, and the number and wall time of
 * report-time flushes.  No reference counterpart (CUPTI's
 * cost is not exposed either); tools/capture_cost.cpp reads it.  runtime_kernels counts the runtime
 * blit dispatches left out (above), own_kernels the library's own report kernels left out: while
 * get_stats / get_records / reset / ingest run, the dispatches of the calling thread are marked
 * (a rocprofiler-sdk external correlation id) and not captured, while other threads' kernels
 * still are, as CUPTI keeps its activity enabled through getStats.  All zero without capture. */
typedef struct nvrx_capture_counters {
    int64_t callbacks, headers, dispatches, callback_ns, flushes, flush_ns, runtime_kernels,
        own_kernels;
    /* where the flushes' time goes: summed over flushes, the time from a flush's start to the
     * first buffer callback it delivered, the callbacks delivered during flushes, and the time
     * from a flush's last callback to its return */
    int64_t flush_first_cb_ns, flush_callbacks, flush_tail_ns;
    /* flush completeness (capture.cpp, top): job dispatches counted at enqueue (the external
     * correlation id request), flushes that waited for every counted dispatch enqueued before
     * them, flushes without that count (marking off: NVRX_CAPTURE_MARKING=0 or the service
     * refused; a 200 us quiet period / the ENQUEUE count / the buffer flush alone), counted
     * flushes that timed out (NVRX_CAPTURE_FLUSH_TIMEOUT_MS, default 1000: a kernel still running)
     * and the dispatches they gave up on (delivered to a later report).  delivery: 0 buffer,
     * 1 callback (default), 2 callback_counted, -1 capture not configured; marking: 1 when the
     * request service is on. */
    int64_t enqueues_counted, counted_flushes, quiet_flushes, flush_timeouts, owed_abandoned;
    int32_t delivery, marking;
    /* queue delivery (3): HSA queues intercepted, dispatches given a completion record of the
     * device ring, dispatches given a pooled HSA signal instead (ring full or absent), packets
     * whose own completion signal was chained behind them, and ring records found past their
     * expected value (0 unless the packet processor does not decrement by one) */
    int64_t queues, ring_records, pool_signals, chained_signals, ring_anomalies;
    /* (ABI 6) queue delivery: dispatches not captured because NVRX_CAPTURE_MAX_PENDING (default
     * 2^20) dispatches already waited for a harvest, or no completion signal was left -- a profiler
     * started for a very long time with no stop, get_stats or flush in between.  The reference's
     * CUPTI buffer pool drops records the same way when every buffer is in use (BufferPool.cpp:44-52);
     * at every start the library harvests once half the completion ring waits, so a started /
     * stopped profiler (a detection section per step) never reaches the bound. */
    int64_t dropped;
} nvrx_capture_counters;
int nvrx_capture_stats(nvrx_capture_counters* out);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* NVRX_STRAGGLER_H */
