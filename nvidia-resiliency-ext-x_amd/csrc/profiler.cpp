// profiler.cpp -- the nvrx_profiler handle of libnvrx_hip.so (declared in include/nvrx_straggler.h):
// what replaces the reference's nvrx_cupti_module.CuptiProfiler (straggler/cupti_src/
// CuptiProfiler.cpp, cupti_module_py.cpp).
//
// Records (pushed, ingested or captured) are kept as a device-resident log in push order; a report
// buckets the log per kernel (records.hip: ring retention of the last statsMaxLenPerKernel) and
// reduces the buckets with one of the segment kernels.  Statistics, quantiles and histograms share
// that pass (report_pass); they differ in the reduction launched and in how a result row is copied.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "abi_util.h"

using nvrx::check_permille;
using nvrx::fail;
using nvrx::hip_status;
using nvrx::S;

struct nvrx_profiler {
    nvrx_profiler_config cfg{};
    std::mutex mu;
    std::mutex ctx_mu;  // start / stop against a report's capture pause (CaptureSelf fallback)
    bool initialized = false;
    bool started = false;
    // kernels seen since the last reset (the keys of CuptiProfiler's _kernelDurations map,
    // which reset() clears, CuptiProfiler.cpp:148-152): slots are renumbered from 0 after
    // every reset, so a long job with changing launch shapes never runs out of slots
    std::unordered_map<std::string, uint32_t> name_to_slot;
    std::vector<std::string> names;
    // live-capture fast path: (kernel id, block, grid) -> slot, no string work per record
    std::unordered_map<nvrx::DispatchKey, uint32_t, nvrx::DispatchKeyHash> key_to_slot;
    std::vector<nvrx_record> staged;  // host records not yet in the device log
    uint64_t saturated = 0;           // wide-key durations (>= 3.76 s) since the last reset
    uint64_t version = 0;             // bumped whenever the record set or the slot table changes
    uint64_t generation = 1;          // slot numbering epoch: bumped by every reset
    hipStream_t stream = nullptr;
    hipEvent_t ingest_ev = nullptr;   // last nvrx_profiler_ingest copy (on the caller's stream)
    bool ingest_pending = false;
    // device record log (push order since the last reset)
    nvrx_record* d_log = nullptr;
    int64_t log_n = 0, log_cap = 0;
    nvrx_record* h_pinned = nullptr;  // pinned staging of the host -> device drain
    int64_t pinned_cap = 0;
    // pinned staging of a report's small transfers: the bucketing's stream offsets up, the six
    // statistics columns down in one copy (pageable copies each cost a blocking round trip)
    char* h_small = nullptr;
    size_t small_bytes = 0;
    // work buffers (grown on demand)
    void* d_work = nullptr;
    size_t work_bytes = 0;
    // the last get_stats result, valid while version == cache_version: the name-sorted slots
    // with records and the six downloaded columns (num, mn, mx, med, avg, sd; c_col bytes apart)
    uint64_t cache_version = ~(uint64_t)0;
    std::vector<uint32_t> c_order;
    std::vector<char> c_host;
    size_t c_col = 0;
    // staged host records move to the device log once `drain_records` wait (at push, and
    // at stop for the live capture -- on the caller's thread, never on rocprofiler's), so
    // host memory stays bounded between reports
    int64_t drain_records = (int64_t)1 << 16;
};

namespace {

std::mutex g_instance_mu;
nvrx_profiler* g_instance = nullptr;

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int grow_log(nvrx_profiler* p, int64_t need) {
    if (need <= p->log_cap) return NVRX_OK;
    int64_t cap = std::max<int64_t>(need, std::max<int64_t>(1 << 16, p->log_cap * 2));
    nvrx_record* nl = nullptr;
    hipError_t e = hipMalloc(&nl, (size_t)cap * sizeof(nvrx_record));
    if (e != hipSuccess) return hip_status(e, "nvrx_profiler: hipMalloc(record log)");
    if (p->log_n > 0) {
        e = hipMemcpyAsync(nl, p->d_log, (size_t)p->log_n * sizeof(nvrx_record),
                           hipMemcpyDeviceToDevice, p->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
        if (e != hipSuccess) {
            (void)hipFree(nl);
            return hip_status(e, "nvrx_profiler: grow record log");
        }
    }
    if (p->d_log) (void)hipFree(p->d_log);
    p->d_log = nl;
    p->log_cap = cap;
    return NVRX_OK;
}

int ensure_work(nvrx_profiler* p, size_t bytes) {
    if (bytes <= p->work_bytes) return NVRX_OK;
    if (p->d_work) (void)hipFree(p->d_work);
    p->d_work = nullptr;
    p->work_bytes = 0;
    size_t b = std::max(bytes, p->work_bytes * 2);
    hipError_t e = hipMalloc(&p->d_work, b);
    if (e != hipSuccess) return hip_status(e, "nvrx_profiler: hipMalloc(work)");
    p->work_bytes = b;
    return NVRX_OK;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// p->h_small holding at least `bytes` (grown on demand)
int ensure_small(nvrx_profiler* p, size_t bytes) {
    if (bytes <= p->small_bytes) return NVRX_OK;
    if (p->h_small) (void)hipHostFree(p->h_small);
    p->h_small = nullptr;
    p->small_bytes = 0;
    const size_t b = std::max<size_t>(bytes, 4096);
    hipError_t e = hipHostMalloc((void**)&p->h_small, b, 0);
    if (e != hipSuccess) return hip_status(e, "nvrx_profiler: hipHostMalloc(small staging)");
    p->small_bytes = b;
    return NVRX_OK;
}

struct Work {  // carve of d_work for one bucketing pass over the record log
    int64_t* rec_off;
    int64_t* seg_off;
    int32_t* seg_len;
    int32_t* counts;
    uint32_t* ns;
    int64_t* dst_off;  // compaction only
    size_t bytes;
};

Work carve(char* base, int64_t nslots, int64_t ns_cap) {
    Work w{};
    size_t o = 0;
    auto take = [&](size_t b) {
        char* p = base ? base + o : nullptr;
        o += align256(b);
        return p;
    };
    w.rec_off = (int64_t*)take(2 * sizeof(int64_t));
    w.seg_off = (int64_t*)take(nslots * sizeof(int64_t));
    w.seg_len = (int32_t*)take(nslots * sizeof(int32_t));
    w.counts = (int32_t*)take(nslots * sizeof(int32_t));
    w.ns = (uint32_t*)take(ns_cap * sizeof(uint32_t));
    w.dst_off = (int64_t*)take(nslots * sizeof(int64_t));
    w.bytes = o;
    return w;
}

// Bucket the whole device log (one stream).  Caller holds p->mu.
int bucket_log(nvrx_profiler* p, int64_t nslots, int force_stable, Work& w) {
    const int64_t ns_cap = nvrx::records_bucket_capacity(p->log_n, 1, nslots);
    Work probe = carve(nullptr, nslots, ns_cap);
    int rc = ensure_work(p, probe.bytes);
    if (rc) return rc;
    w = carve((char*)p->d_work, nslots, ns_cap);
    // (a report has sized h_small for its download already -- report_pass -- so this keeps the
    // allocation: h_small is never reallocated under a pending copy)
    rc = ensure_small(p, 2 * sizeof(int64_t));
    if (rc) return rc;
    int64_t* off = (int64_t*)p->h_small;  // (the previous use of h_small has completed: synchronous calls)
    off[0] = 0;
    off[1] = p->log_n;
    hipError_t e = hipMemcpyAsync(w.rec_off, off, 2 * sizeof(int64_t), hipMemcpyHostToDevice, p->stream);
    if (e != hipSuccess) return hip_status(e, "nvrx_profiler: rec_off upload");
    e = nvrx::records_bucket(p->d_log, w.rec_off, 1, nslots, p->cfg.stats_max_len_per_kernel,
                             force_stable, w.seg_off, w.seg_len, w.ns, w.counts, p->stream);
    return hip_status(e, "nvrx_profiler: records_bucket");
}

// Move staged host records into the device log (through a pinned buffer: a DMA copy, no
// kernel launch that a started capture could record); compact the log when it is much larger
// than what the rings can retain.  Caller holds p->mu.
int flush_locked(nvrx_profiler* p) {
    DeviceGuard g(p->cfg.device);
    if (p->ingest_pending) {  // device-ingested records were copied on the caller's stream
        hipError_t e = hipStreamWaitEvent(p->stream, p->ingest_ev, 0);
        if (e != hipSuccess) return hip_status(e, "nvrx_profiler: wait for ingest");
        p->ingest_pending = false;
    }
    if (!p->staged.empty()) {
        const int64_t add = (int64_t)p->staged.size();
        int rc = grow_log(p, p->log_n + add);
        if (rc) return rc;
        if (add > p->pinned_cap) {
            if (p->h_pinned) (void)hipHostFree(p->h_pinned);
            p->h_pinned = nullptr;
            p->pinned_cap = 0;
            const int64_t c = std::max<int64_t>(add, p->drain_records);
            hipError_t e = hipHostMalloc((void**)&p->h_pinned, (size_t)c * sizeof(nvrx_record), 0);
            if (e != hipSuccess) return hip_status(e, "nvrx_profiler: hipHostMalloc(staging)");
            p->pinned_cap = c;
        }
        std::memcpy(p->h_pinned, p->staged.data(), (size_t)add * sizeof(nvrx_record));
        hipError_t e = hipMemcpyAsync(p->d_log + p->log_n, p->h_pinned,
                                      (size_t)add * sizeof(nvrx_record), hipMemcpyHostToDevice,
                                      p->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
        if (e != hipSuccess) return hip_status(e, "nvrx_profiler: flush");
        p->log_n += add;
        p->staged.clear();
        if (p->staged.capacity() > (size_t)4 * p->drain_records) p->staged.shrink_to_fit();
    }
    const int64_t nslots = (int64_t)p->names.size();
    const int64_t cap = p->cfg.stats_max_len_per_kernel;
    const int64_t retain_bound = nslots * (cap > 0 ? cap : p->log_n);
    if (cap > 0 && p->log_n > (int64_t)1 << 22 && p->log_n > 4 * retain_bound) {
        // compaction keeps exactly the records a later retention step could still keep
        Work w;
        int rc = bucket_log(p, nslots, /*force_stable=*/1, w);
        if (rc) return rc;
        std::vector<int32_t> len(nslots);
        hipError_t e = hipMemcpyAsync(len.data(), w.seg_len, nslots * sizeof(int32_t),
                                      hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
        if (e != hipSuccess) return hip_status(e, "nvrx_profiler: compaction lengths");
        std::vector<int64_t> dst(nslots);
        int64_t tot = 0;
        for (int64_t s = 0; s < nslots; ++s) dst[s] = tot, tot += len[s];
        nvrx_record* nl = nullptr;
        e = hipMalloc(&nl, (size_t)std::max<int64_t>(tot, 1) * sizeof(nvrx_record));
        if (e != hipSuccess) return hip_status(e, "nvrx_profiler: hipMalloc(compaction)");
        e = hipMemcpyAsync(w.dst_off, dst.data(), nslots * sizeof(int64_t), hipMemcpyHostToDevice,
                           p->stream);
        if (e == hipSuccess)
            e = nvrx::records_unbucket(w.seg_off, w.seg_len, w.dst_off, w.ns, nslots, nl, p->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
        if (e != hipSuccess) {
            (void)hipFree(nl);
            return hip_status(e, "nvrx_profiler: compaction");
        }
        (void)hipFree(p->d_log);
        p->d_log = nl;
        p->log_n = tot;
        p->log_cap = std::max<int64_t>(tot, 1);
    }
    return NVRX_OK;
}

// The report's own kernels (bucketing, statistics, copies) must not be captured as dispatches
// of the profiled job -- the reference's getStats runs on the host and adds nothing.  They are
// marked by thread (capture_self_begin: rocprofiler-sdk's external correlation id of every
// dispatch this thread makes until the guard ends), so kernels that OTHER threads launch during
// the report are still captured, as CUPTI keeps its activity enabled through getStats.  If the
// marking is unavailable, the dispatch context is paused instead (kernels other threads launch
// meanwhile are then lost); start / stop wait for a pause to end (ctx_mu), and the capture is
// restarted only if the profiler is still started.  Neither makes the flush cheaper
// (rocprofiler_flush_buffer).
struct CaptureSelf {
    nvrx_profiler* p;
    bool marked = false, paused = false;
    std::unique_lock<std::mutex> ctx;
    explicit CaptureSelf(nvrx_profiler* q) : p(q) {
        if (!nvrx::capture_ready()) return;
        marked = nvrx::capture_self_begin();
        if (marked) return;
        ctx = std::unique_lock<std::mutex>(p->ctx_mu);
        bool started;
        {
            std::lock_guard<std::mutex> lk(p->mu);
            started = p->started;
        }
        if (started) paused = nvrx::capture_stop(p) == 0;
    }
    ~CaptureSelf() {
        if (marked) nvrx::capture_self_end();
        if (!paused) return;
        bool started;
        {
            std::lock_guard<std::mutex> lk(p->mu);
            started = p->started;
        }
        if (started) (void)nvrx::capture_start(p);
    }
};

uint32_t slot_of_name(nvrx_profiler* p, const std::string& key) {
    auto it = p->name_to_slot.find(key);
    if (it != p->name_to_slot.end()) return it->second;
    const uint32_t slot = (uint32_t)p->names.size();
    p->name_to_slot.emplace(key, slot);
    p->names.push_back(key);
    return slot;
}

// How every call that reads the record log begins: its own kernels are not captured, completed
// dispatches are delivered (CuptiProfiler.cpp:138 cuptiActivityFlushAll; before the lock), then
// under p->mu, on the profiler's device, the staged records move to the device log.  rc: that
// flush's status.  (Members are initialised in this order.)
struct LogAccess {
    CaptureSelf self;
    int delivered;
    std::lock_guard<std::mutex> lk;
    DeviceGuard g;
    int rc;
    explicit LogAccess(nvrx_profiler* p)
        : self(p), delivered(nvrx::capture_flush()), lk(p->mu), g(p->cfg.device), rc(flush_locked(p)) {}
};

// One report pass over the record log (caller: inside a LogAccess).  The log is bucketed per
// kernel, `reduce(w, extra, nslots, keep, stream)` launches a reduction over the buckets (keep:
// a bound on the retained length) into `extra`, extra_bytes of device memory that begin with
// num [nslots] (int32), and `copy_out(order, host)` receives the downloaded copy of `extra` with
// the kernels that have records in std::map order of getStats (CuptiProfiler.cpp:137-145: sorted
// by composite name).  An empty log or no kernels: nothing runs, copy_out is not called.  The
// log and the slot table are left as they are.
template <class Reduce, class CopyOut>
int report_pass(nvrx_profiler* p, const char* fn, size_t extra_bytes, Reduce reduce, CopyOut copy_out) {
    const int64_t nslots = (int64_t)p->names.size();
    if (p->log_n == 0 || nslots == 0) return NVRX_OK;
    // both buffers are sized before bucket_log, whose own ensure_work / ensure_small then keep the
    // allocations: `extra` follows the bucketing's carve, and h_small is not reallocated between
    // the bucketing's upload and the download
    const size_t carve_bytes = carve(nullptr, nslots, nvrx::records_bucket_capacity(p->log_n, 1, nslots)).bytes;
    int rc = ensure_work(p, carve_bytes + extra_bytes);
    if (rc == NVRX_OK) rc = ensure_small(p, extra_bytes);
    if (rc) return rc;
    Work w;
    rc = bucket_log(p, nslots, 0, w);
    if (rc) return rc;
    char* extra = (char*)p->d_work + carve_bytes;
    hipError_t e = reduce(w, extra, nslots, std::min<int64_t>(p->cfg.stats_max_len_per_kernel, p->log_n),
                          p->stream);
    if (e != hipSuccess) return hip_status(e, (std::string(fn) + ": reduction").c_str());
    e = hipMemcpyAsync(p->h_small, extra, extra_bytes, hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) return hip_status(e, (std::string(fn) + ": download").c_str());
    const int32_t* hnum = (const int32_t*)p->h_small;
    std::vector<uint32_t> order;
    for (int64_t s = 0; s < nslots; ++s)
        if (hnum[s] > 0) order.push_back((uint32_t)s);
    std::sort(order.begin(), order.end(),
              [&](uint32_t a, uint32_t b) { return p->names[a] < p->names[b]; });
    copy_out(order, (const char*)p->h_small);
    return NVRX_OK;
}

// report_pass for a getter without a cache: count, slots and num are copied here, `row(i, slot,
// host)` copies result row `slot` to output position i; at most cap_out rows.
template <class Reduce, class Row>
int report_rows(nvrx_profiler* p, const char* fn, size_t extra_bytes, int64_t cap_out, int64_t* count,
                uint32_t* slots, int32_t* num, Reduce reduce, Row row) {
    *count = 0;
    return report_pass(p, fn, extra_bytes, reduce, [&](const std::vector<uint32_t>& order, const char* h) {
        *count = (int64_t)order.size();
        const int64_t m = std::min<int64_t>(cap_out, *count);
        for (int64_t i = 0; i < m; ++i) {
            if (slots) slots[i] = order[i];
            if (num) num[i] = ((const int32_t*)h)[order[i]];
            row(i, order[i], h);
        }
    });
}

}  // namespace

namespace nvrx {
// the capture's delivery (capture_drain / q_harvest): one batch of completed dispatches.  A dispatch
// enqueued while the profiler was started may complete (and its record arrive) after stop;
// it is still counted, as CUPTI delivers the activity records of kernels launched while the
// activity kind was enabled (bufferCompleted, CuptiProfiler.cpp:168-203, pushes regardless
// of _isStarted).
void profiler_push_dispatches(nvrx_profiler* p, const DispatchRec* r, size_t n,
                              std::string (*composite_name)(const DispatchKey&)) {
    {
        std::lock_guard<std::mutex> lk(p->mu);
        if (!p->initialized) return;
        for (size_t i = 0; i < n; ++i) {
            uint32_t slot;
            auto it = p->key_to_slot.find(r[i].key);
            if (it != p->key_to_slot.end()) {
                slot = it->second;
            } else {
                slot = slot_of_name(p, composite_name(r[i].key));  // CuptiProfiler.cpp:182-185
                p->key_to_slot.emplace(r[i].key, slot);
            }
            // CuptiProfiler.cpp:187 keeps f32(end - start): the duration key carries exactly
            // that for any u64 (the integer ns below 3.76 s)
            const uint32_t key = nvrx_duration_key(r[i].ns);
            if (key >= NVRX_KEY_WIDE) ++p->saturated;
            p->staged.push_back(nvrx_record{slot, key});
        }
        ++p->version;
    }
}
}  // namespace nvrx

extern "C" {

int nvrx_profiler_create(const nvrx_profiler_config* cfg, nvrx_profiler** out) {
    NVRX_CHECK_ARG(cfg && out, "nvrx_profiler_create: null argument");
    NVRX_CHECK_ARG(cfg->stats_max_len_per_kernel > 0 &&
                       cfg->stats_max_len_per_kernel <= NVRX_MAX_SEGMENT,
                   "nvrx_profiler_create: statsMaxLenPerKernel must be in [1, 2^30]");
    NVRX_CHECK_ARG(cfg->mode == NVRX_STATS_FAST || cfg->mode == NVRX_STATS_EXACT,
                   "nvrx_profiler_create: unknown mode");
    if (cfg->stats_max_len_per_kernel > ((int64_t)1 << 24))
        std::fprintf(stderr, "nvrx_profiler_create: statsMaxLenPerKernel=%lld: rings above 2^24 samples "
                             "are reduced in device scratch of up to 4 B per retained sample (4 GiB at "
                             "2^30) by one workgroup per kernel -- slow\n",
                     (long long)cfg->stats_max_len_per_kernel);
    std::lock_guard<std::mutex> lk(g_instance_mu);
    if (g_instance)  // CuptiProfiler.cpp:86-87
        return fail(NVRX_ERR_SINGLETON, "Only one CuptiProfiler instance is allowed.");
    auto* p = new nvrx_profiler();
    p->cfg = *cfg;
    // the drain watermark follows the host buffer size (CUPTI bufferSize, cupti.py:25)
    if (cfg->buffer_size >= (int64_t)sizeof(nvrx_record) * 1024)
        p->drain_records = cfg->buffer_size / (int64_t)sizeof(nvrx_record);
    {
        DeviceGuard g(cfg->device);
        hipError_t e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&p->ingest_ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            if (p->stream) (void)hipStreamDestroy(p->stream);
            delete p;
            return hip_status(e, "nvrx_profiler_create: stream/event");
        }
    }
    g_instance = p;
    *out = p;
    return NVRX_OK;
}

int nvrx_profiler_destroy(nvrx_profiler* p) {
    NVRX_CHECK_ARG(p, "nvrx_profiler_destroy: null handle");
    // no capture callback may touch the handle after this: capture_detach delivers what is
    // pending, unhooks the handle and waits for any callback still running
    nvrx::capture_detach(p);
    {
        std::lock_guard<std::mutex> lk(g_instance_mu);
        if (g_instance == p) g_instance = nullptr;
    }
    {
        DeviceGuard g(p->cfg.device);
        if (p->stream) (void)hipStreamSynchronize(p->stream);
        if (p->d_log) (void)hipFree(p->d_log);
        if (p->d_work) (void)hipFree(p->d_work);
        if (p->h_pinned) (void)hipHostFree(p->h_pinned);
        if (p->h_small) (void)hipHostFree(p->h_small);
        if (p->ingest_ev) (void)hipEventDestroy(p->ingest_ev);
        if (p->stream) (void)hipStreamDestroy(p->stream);
    }
    delete p;
    return NVRX_OK;
}

int nvrx_profiler_initialize(nvrx_profiler* p) {
    NVRX_CHECK_ARG(p, "nvrx_profiler_initialize: null handle");
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->initialized)
        std::fprintf(stderr, "CuptiProfiler::initializeProfiling subsequent call.\n");
    p->initialized = true;
    return NVRX_OK;
}

int nvrx_profiler_shutdown(nvrx_profiler* p) {
    NVRX_CHECK_ARG(p, "nvrx_profiler_shutdown: null handle");
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->initialized)
        std::fprintf(stderr, "CuptiProfiler::shutdownProfiling called while not initialized.\n");
    p->initialized = false;
    p->started = false;
    return NVRX_OK;
}

int nvrx_profiler_start(nvrx_profiler* p) {
    NVRX_CHECK_ARG(p, "nvrx_profiler_start: null handle");
    std::lock_guard<std::mutex> ctx(p->ctx_mu);  // not inside a report's pause
    {
        std::lock_guard<std::mutex> lk(p->mu);
        if (p->started) std::fprintf(stderr, "CuptiProfiler::startProfiling subsequent call.\n");
        p->started = true;
    }
    // live capture (CuptiProfiler.cpp:115-118 enables the activity kind)
    if (nvrx::capture_start(p) != 0)
        return fail(NVRX_ERR_STATE, "nvrx_profiler_start: rocprofiler_start_context failed");
    return NVRX_OK;
}

int nvrx_profiler_stop(nvrx_profiler* p) {
    NVRX_CHECK_ARG(p, "nvrx_profiler_stop: null handle");
    std::lock_guard<std::mutex> ctx(p->ctx_mu);  // not inside a report's pause
    const int rc = nvrx::capture_stop(p);
    nvrx::capture_drain(p);  // callback delivery: completed dispatches queued so far (before p->mu)
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->started) std::fprintf(stderr, "CuptiProfiler::stopProfiling called while not profiling.\n");
    p->started = false;
    if (rc != 0) return fail(NVRX_ERR_STATE, "nvrx_profiler_stop: rocprofiler_stop_context failed");
    // bounded host memory: what the capture delivered so far moves to the device log here,
    // on the caller's thread, once a buffer's worth waits
    if ((int64_t)p->staged.size() >= p->drain_records) return flush_locked(p);
    return NVRX_OK;
}

int nvrx_profiler_reset(nvrx_profiler* p) {
    NVRX_CHECK_ARG(p, "nvrx_profiler_reset: null handle");
    CaptureSelf self(p);
    (void)nvrx::capture_flush();  // CuptiProfiler.cpp:149: flush, then clear (outside the lock)
    std::lock_guard<std::mutex> lk(p->mu);
    DeviceGuard g(p->cfg.device);
    if (p->ingest_pending) {  // an ingest copy may still target the log
        (void)hipEventSynchronize(p->ingest_ev);
        p->ingest_pending = false;
    }
    // CuptiProfiler.cpp:148-152: clear every kernel's ring -- and forget the kernels, so
    // the slots are renumbered from 0 in the next interval
    p->staged.clear();
    p->log_n = 0;
    p->names.clear();
    p->name_to_slot.clear();
    p->key_to_slot.clear();
    p->saturated = 0;
    ++p->version;
    ++p->generation;  // slots handed out before this reset are void
    return NVRX_OK;
}

int nvrx_profiler_generation(nvrx_profiler* p, uint64_t* generation) {
    NVRX_CHECK_ARG(p && generation, "nvrx_profiler_generation: null argument");
    std::lock_guard<std::mutex> lk(p->mu);
    *generation = p->generation;
    return NVRX_OK;
}

int nvrx_profiler_register_kernel(nvrx_profiler* p, const char* name, uint32_t* slot) {
    NVRX_CHECK_ARG(p && name && slot, "nvrx_profiler_register_kernel: null argument");
    std::lock_guard<std::mutex> lk(p->mu);
    const size_t before = p->names.size();
    *slot = slot_of_name(p, name);
    if (p->names.size() != before) ++p->version;  // a cached get_stats result is stale
    return NVRX_OK;
}

int nvrx_profiler_push(nvrx_profiler* p, const nvrx_record* recs, int64_t n) {
    NVRX_CHECK_ARG(p && (n == 0 || recs) && n >= 0, "nvrx_profiler_push: bad arguments");
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->started) return NVRX_OK;  // activity disabled: records are not captured
    const uint32_t nslots = (uint32_t)p->names.size();
    for (int64_t i = 0; i < n; ++i)
        if (recs[i].slot >= nslots) return fail(NVRX_ERR_INVALID, "nvrx_profiler_push: unknown slot");
    for (int64_t i = 0; i < n; ++i) p->saturated += recs[i].ns >= NVRX_KEY_WIDE;
    p->staged.insert(p->staged.end(), recs, recs + n);
    ++p->version;
    if ((int64_t)p->staged.size() >= p->drain_records) return flush_locked(p);
    return NVRX_OK;
}

int nvrx_profiler_ingest(nvrx_profiler* p, const nvrx_record* dev_recs, int64_t n,
                         uint64_t generation, void* stream) {
    NVRX_CHECK_ARG(p && n >= 0 && (n == 0 || dev_recs), "nvrx_profiler_ingest: bad arguments");
    CaptureSelf self(p);  // the ingest copy is the library's own kernel, not the job's
    std::lock_guard<std::mutex> lk(p->mu);
    if (generation != p->generation)
        return fail(NVRX_ERR_STATE, "nvrx_profiler_ingest: slots of another generation (a reset "
                                    "renumbered them; register the kernels again)");
    if (!p->started || n == 0) return NVRX_OK;  // activity disabled: records are not captured
    DeviceGuard g(p->cfg.device);
    int rc = flush_locked(p);  // host records staged earlier come first (push order)
    if (rc) return rc;
    rc = grow_log(p, p->log_n + n);
    if (rc) return rc;
    // a copy that drops (slot := UINT32_MAX) records of slots not registered at this call
    hipError_t e = nvrx::records_ingest(p->d_log + p->log_n, dev_recs, n, (uint32_t)p->names.size(),
                                        S(stream));
    if (e == hipSuccess) e = hipEventRecord(p->ingest_ev, S(stream));
    if (e != hipSuccess) return hip_status(e, "nvrx_profiler_ingest");
    p->ingest_pending = true;
    p->log_n += n;
    ++p->version;
    return NVRX_OK;
}

int nvrx_profiler_saturated(nvrx_profiler* p, int64_t* count) {
    NVRX_CHECK_ARG(p && count, "nvrx_profiler_saturated: null argument");
    std::lock_guard<std::mutex> lk(p->mu);
    *count = (int64_t)p->saturated;
    return NVRX_OK;
}

int nvrx_profiler_get_stats(nvrx_profiler* p, int64_t cap_out, int64_t* count, uint32_t* slots,
                            int32_t* num, float* mn, float* mx, float* med, float* avg, float* sd) {
    NVRX_CHECK_ARG(p && count && cap_out >= 0, "nvrx_profiler_get_stats: bad arguments");
    LogAccess log(p);
    if (log.rc) return log.rc;
    if (p->cache_version != p->version) {
        // recompute (a size query followed by the copy call reuses this result): the six columns
        // num, mn, mx, med, avg, sd, each 256-B aligned: one span, one copy
        p->c_order.clear();
        const int64_t nslots = (int64_t)p->names.size();
        const size_t col = p->c_col = align256((size_t)nslots * 4), span = 5 * col + (size_t)nslots * 4;
        const int rc = report_pass(
            p, "nvrx_profiler_get_stats", span,
            [&](Work& w, char* x, int64_t n, int64_t keep, hipStream_t st) {
                const auto f = [&](int c) { return (float*)(x + c * col); };
                const nvrx_stats_soa soa{(int32_t*)x, f(1), f(2), f(3), f(4), f(5)};
                return nvrx::segment_stats_ragged(w.ns, w.seg_off, w.seg_len, n, keep,
                                                  p->cfg.stats_max_len_per_kernel, p->cfg.mode, true,
                                                  soa, nullptr, 0, st);
            },
            [&](const std::vector<uint32_t>& order, const char* h) {
                p->c_order = order;
                p->c_host.assign(h, h + span);
            });
        if (rc) return rc;
        p->cache_version = p->version;
    }
    *count = (int64_t)p->c_order.size();
    const int64_t m = std::min<int64_t>(cap_out, *count);
    float* const outs[5] = {mn, mx, med, avg, sd};
    for (int64_t i = 0; i < m; ++i) {
        const uint32_t s = p->c_order[i];
        if (slots) slots[i] = s;
        if (num) num[i] = ((const int32_t*)p->c_host.data())[s];
        for (int c = 0; c < 5; ++c)
            if (outs[c]) outs[c][i] = ((const float*)(p->c_host.data() + (c + 1) * p->c_col))[s];
    }
    return NVRX_OK;
}

int nvrx_profiler_get_quantiles(nvrx_profiler* p, const int32_t* permille, int32_t nq,
                                int64_t cap_out, int64_t* count, uint32_t* slots, int32_t* num,
                                float* out) {
    NVRX_CHECK_ARG(p, "nvrx_profiler_get_quantiles: null handle");
    if (int rc = check_permille("nvrx_profiler_get_quantiles", permille, nq)) return rc;
    NVRX_CHECK_ARG(count, "nvrx_profiler_get_quantiles: null count");
    NVRX_CHECK_ARG(cap_out >= 0, "nvrx_profiler_get_quantiles: negative cap_out");
    LogAccess log(p);
    if (log.rc) return log.rc;
    // num [nslots] (256-B aligned), then the quantiles [nq][nslots]
    const int64_t nslots = (int64_t)p->names.size();
    const size_t q0 = align256((size_t)nslots * 4);
    return report_rows(
        p, "nvrx_profiler_get_quantiles", q0 + (size_t)nq * (size_t)nslots * 4, cap_out, count, slots, num,
        [&](Work& w, char* x, int64_t n, int64_t keep, hipStream_t st) {
            return nvrx::segment_quantiles_ragged(w.ns, w.seg_off, w.seg_len, n, keep,
                                                  p->cfg.stats_max_len_per_kernel, true, permille, nq,
                                                  (float*)(x + q0), (int32_t*)x, st);
        },
        [&](int64_t i, uint32_t s, const char* h) {
            if (out)
                for (int32_t j = 0; j < nq; ++j) out[j * cap_out + i] = ((const float*)(h + q0))[j * nslots + s];
        });
}

int nvrx_profiler_get_histograms(nvrx_profiler* p, int64_t cap_out, int64_t* count,
                                 uint32_t* slots, int32_t* num, uint32_t* out) {
    NVRX_CHECK_ARG(p, "nvrx_profiler_get_histograms: null handle");
    NVRX_CHECK_ARG(count, "nvrx_profiler_get_histograms: null count");
    NVRX_CHECK_ARG(cap_out >= 0, "nvrx_profiler_get_histograms: negative cap_out");
    LogAccess log(p);
    if (log.rc) return log.rc;
    // num [nslots] (256-B aligned), then the counts [nslots][240]
    const int64_t nslots = (int64_t)p->names.size();
    const size_t c0 = align256((size_t)nslots * 4);
    return report_rows(
        p, "nvrx_profiler_get_histograms", c0 + (size_t)nslots * NVRX_HIST_BINS * 4, cap_out, count, slots, num,
        [&](Work& w, char* x, int64_t n, int64_t keep, hipStream_t st) {
            return nvrx::segment_histogram_ragged(w.ns, w.seg_off, w.seg_len, n, keep,
                                                  p->cfg.stats_max_len_per_kernel, true, 0,
                                                  (uint32_t*)(x + c0), (int32_t*)x, st);
        },
        [&](int64_t i, uint32_t s, const char* h) {
            if (out)
                std::memcpy(out + i * NVRX_HIST_BINS, (const uint32_t*)(h + c0) + (size_t)s * NVRX_HIST_BINS,
                            NVRX_HIST_BINS * sizeof(uint32_t));
        });
}

int nvrx_profiler_get_records(nvrx_profiler* p, int64_t cap_out, int64_t* count,
                              nvrx_record* out) {
    NVRX_CHECK_ARG(p && count && cap_out >= 0 && (cap_out == 0 || out),
                   "nvrx_profiler_get_records: bad arguments");
    LogAccess log(p);
    if (log.rc) return log.rc;
    *count = p->log_n;
    const int64_t m = std::min<int64_t>(cap_out, p->log_n);
    if (m == 0) return NVRX_OK;
    hipError_t e = hipMemcpyAsync(out, p->d_log, (size_t)m * sizeof(nvrx_record),
                                  hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    return hip_status(e, "nvrx_profiler_get_records: download");
}

int nvrx_profiler_kernel_name(nvrx_profiler* p, uint32_t slot, char* buf, int64_t buflen) {
    NVRX_CHECK_ARG(p && buf && buflen > 0, "nvrx_profiler_kernel_name: bad arguments");
    std::lock_guard<std::mutex> lk(p->mu);
    NVRX_CHECK_ARG(slot < p->names.size(), "nvrx_profiler_kernel_name: unknown slot");
    const std::string& s = p->names[slot];
    if ((int64_t)s.size() + 1 > buflen)
        return fail(NVRX_ERR_INVALID, "nvrx_profiler_kernel_name: buffer too small");
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return NVRX_OK;
}

}  // extern "C"
