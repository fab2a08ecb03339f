// tail_checks_host.cpp -- a stand-alone host of abi.cpp's argument checks for the tail-score
// entries, for a sanitizer build (make -C tests/native tail_checks_host builds it with
// -fsanitize=address,undefined on the host side and links abi.cpp itself into the program; the
// launch functions behind the checks come from libnvrx_hip.so and are never reached).  Every call
// below is refused at a check, so the program needs no GPU: it drives each entry with null and
// misaligned arguments, the cases of tests/test_*_abi.py, and compares status and message.
//
// Usage: tail_checks_host        exit status 0 when every case is refused as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "nvrx_straggler.h"

static int failures = 0, cases = 0;

static void expect(int rc, const char* want, const char* what) {
    ++cases;
    const char* msg = nvrx_last_error();
    if (rc != NVRX_ERR_INVALID || !std::strstr(msg, want)) {
        std::fprintf(stderr, "tail_checks_host: %s: status %d, message \"%s\", expected \"%s\"\n", what, rc,
                     msg, want);
        ++failures;
    }
}
#define EXPECT(call, want) expect((call), want, #call)

// never dereferenced: the calls stop at a check
template <typename T>
static T* fake(uintptr_t addr = 0x10000) { return reinterpret_cast<T*>(addr); }

template <typename A>
static void segments(A& a) {
    a.R = 2;
    a.K = 3;
    a.ns = fake<const uint32_t>();
    a.seg_off = fake<const int64_t>();
    a.max_len = 8;
}
template <typename A>
static void score_outputs(A& a) {
    a.permille = 990;
    a.mode = NVRX_HTAIL_SCORE | NVRX_HTAIL_UPDATE;
    a.tail_ns = fake<uint64_t>(0x20000);
    a.total_ns = fake<uint64_t>(0x20100);
    a.base_tail_ns = fake<uint64_t>(0x20200);
    a.base_total_ns = fake<uint64_t>(0x20300);
    a.score = fake<double>(0x20400);
}
template <typename A>
static void attribution_outputs(A& a) {
    a.top = 4;
    a.idx = fake<int32_t>(0x30000);
    a.loss = fake<double>(0x30100);
    a.tail_ns = fake<uint64_t>(0x30200);
    a.total_ns = fake<uint64_t>(0x30300);
    a.tail_calls = fake<uint32_t>(0x30400);
    a.thr_bucket = fake<int32_t>(0x30500);
    a.base_share = fake<double>(0x30600);
    a.loss_all = fake<double>(0x30700);
}

// the request and the outputs of an individual score: the same cases for every such entry
template <typename A, typename F>
static void history_cases(const A& good, F call) {
    A a = good;
    a.mode = 0;
    EXPECT(call(&a), ": mode must be NVRX_HTAIL_SCORE, NVRX_HTAIL_UPDATE or both");
    a = good;
    a.mode = 4;
    EXPECT(call(&a), ": mode must be");
    a = good;
    a.permille = 1001;
    EXPECT(call(&a), ": permille outside [0, 1000]");
    a = good;
    a.hist_stride = -1;
    EXPECT(call(&a), ": negative hist_stride");
    a = good;
    a.hist_stride = 2;
    EXPECT(call(&a), ": hist_stride below K without hist_index");
    a = good;
    a.tail_ns = nullptr;
    EXPECT(call(&a), ": null tail_ns");
    a = good;
    a.base_total_ns = nullptr;
    EXPECT(call(&a), ": null base_total_ns");
    a = good;
    a.score = nullptr;
    EXPECT(call(&a), ": null score");
    a = good;
    a.R = -1;
    EXPECT(call(&a), ": negative R");
}
template <typename A, typename F>
static void folded_cases(const A& good, F call) {
    A a = good;
    a.folded = nullptr;
    EXPECT(call(&a), ": null folded");
    a = good;
    a.folded = a.total_ns;
    EXPECT(call(&a), ": folded aliases another output");
    a = good;
    a.folded = fake<uint64_t>(0x40004);
    EXPECT(call(&a), ": folded not 8-byte aligned");
    a = good;
    a.base_tail_ns = fake<uint64_t>(0x20204);
    EXPECT(call(&a), ": base_tail_ns not 8-byte aligned");
    a = good;
    a.chist = fake<void>(0x50008);
    EXPECT(call(&a), ": chist not 16-byte aligned");
    a = good;
    a.chist = nullptr;
    EXPECT(call(&a), ": null chist");
}
template <typename A, typename F>
static void attribution_cases(const A& good, F call) {
    A a = good;
    a.top = 0;
    EXPECT(call(&a), ": top must be in [1, NVRX_MAX_ATTRIBUTION = 16]");
    a = good;
    a.top = 17;
    EXPECT(call(&a), ": top must be in [1, NVRX_MAX_ATTRIBUTION = 16]");
    a = good;
    a.idx = nullptr;
    EXPECT(call(&a), ": null idx");
    a = good;
    a.tail_calls = nullptr;
    EXPECT(call(&a), ": null tail_calls");
    a = good;
    a.loss_all = nullptr;
    EXPECT(call(&a), ": null loss_all");
    a = good;
    a.K = -1;
    EXPECT(call(&a), ": negative K");
}
template <typename A, typename F>
static void attribution_alignment_cases(const A& good, F call) {  // the record-stream entries
    A a = good;
    a.loss = fake<double>(0x30104);
    EXPECT(call(&a), ": loss not 8-byte aligned");
    a = good;
    a.base_share = fake<double>(0x30604);
    EXPECT(call(&a), ": base_share not 8-byte aligned");
    a = good;
    a.loss_all = fake<double>(0x30704);
    EXPECT(call(&a), ": loss_all not 8-byte aligned");
    a = good;
    a.seg_off = fake<const int64_t>(0x10004);
    EXPECT(call(&a), ": seg_off not 8-byte aligned");
    a = good;
    a.seg_off = nullptr;
    EXPECT(call(&a), ": null seg_off");
}

int main() {
    const auto none = static_cast<void*>(nullptr);
    {
        EXPECT(nvrx_histogram_history_scores(nullptr, none), "nvrx_histogram_history_scores: null args");
        nvrx_histtail_args a{};
        a.R = 2;
        a.K = 3;
        a.counts = fake<const uint32_t>();
        a.hist = fake<uint32_t>(0x50000);
        score_outputs(a);
        auto call = [&](const nvrx_histtail_args* p) { return nvrx_histogram_history_scores(p, none); };
        history_cases(a, call);
        nvrx_histtail_args b = a;
        b.total_ns = fake<uint64_t>(0x20104);
        EXPECT(call(&b), ": the u64 outputs are not 8-byte aligned");
        b = a;
        b.hist = nullptr;
        EXPECT(call(&b), ": null hist");
    }
    {
        EXPECT(nvrx_segment_history_scores_ragged(nullptr, none), ": null args");
        nvrx_seghist_args a{};
        segments(a);
        a.hist = fake<uint32_t>(0x50000);
        score_outputs(a);
        auto call = [&](const nvrx_seghist_args* p) { return nvrx_segment_history_scores_ragged(p, none); };
        history_cases(a, call);
        nvrx_seghist_args b = a;
        b.score = fake<double>(0x20404);
        EXPECT(call(&b), ": score not 8-byte aligned");
        b = a;
        b.hist = fake<uint32_t>(0x50008);
        EXPECT(call(&b), ": hist not 16-byte aligned");
    }
    {
        EXPECT(nvrx_segment_history_scores_compact_ragged(nullptr, none), ": null args");
        nvrx_segchist_args a{};
        segments(a);
        a.chist = fake<void>(0x50000);
        score_outputs(a);
        a.folded = fake<uint64_t>(0x40000);
        auto call = [&](const nvrx_segchist_args* p) {
            return nvrx_segment_history_scores_compact_ragged(p, none);
        };
        history_cases(a, call);
        folded_cases(a, call);
    }
    {
        EXPECT(nvrx_histogram_history_scores_compact(nullptr, none), ": null args");
        nvrx_histchist_args a{};
        a.R = 2;
        a.K = 3;
        a.counts = fake<const uint32_t>();
        a.chist = fake<void>(0x50000);
        score_outputs(a);
        a.folded = fake<uint64_t>(0x40000);
        auto call = [&](const nvrx_histchist_args* p) { return nvrx_histogram_history_scores_compact(p, none); };
        history_cases(a, call);
        folded_cases(a, call);
        nvrx_histchist_args b = a;
        b.counts = fake<const uint32_t>(0x10008);
        EXPECT(call(&b), ": counts not 16-byte aligned");
    }
    {
        EXPECT(nvrx_histogram_tail_attribution(nullptr, none), ": null args");
        nvrx_tailattr_args a{};
        a.R = 2;
        a.K = 3;
        a.counts = fake<const uint32_t>();
        a.kind = NVRX_ATTR_RELATIVE;
        a.thr = fake<const int32_t>(0x60000);
        a.base = fake<const uint64_t>(0x60100);
        attribution_outputs(a);
        auto call = [&](const nvrx_tailattr_args* p) { return nvrx_histogram_tail_attribution(p, none); };
        attribution_cases(a, call);
        nvrx_tailattr_args b = a;
        b.kind = 7;
        EXPECT(call(&b), ": unknown kind");
        b = a;
        b.base = nullptr;
        EXPECT(call(&b), ": the relative kind needs base");
        b = a;
        b.loss = fake<double>(0x30104);
        EXPECT(call(&b), ": the 8-byte outputs are not 8-byte aligned");
        b = a;
        b.kind = NVRX_ATTR_INDIVIDUAL;
        b.permille = -1;
        EXPECT(call(&b), ": permille outside [0, 1000]");
        b.permille = 990;
        EXPECT(call(&b), ": the individual kind needs hist");
    }
    {
        EXPECT(nvrx_segment_tail_attribution_ragged(nullptr, none), ": null args");
        nvrx_segtailattr_args a{};
        segments(a);
        a.thr = fake<const int32_t>(0x60000);
        a.base = fake<const uint64_t>(0x60100);
        attribution_outputs(a);
        auto call = [&](const nvrx_segtailattr_args* p) { return nvrx_segment_tail_attribution_ragged(p, none); };
        attribution_cases(a, call);
        attribution_alignment_cases(a, call);
        nvrx_segtailattr_args b = a;
        b.thr = nullptr;
        EXPECT(call(&b), ": null thr");
        b = a;
        b.base = fake<const uint64_t>(0x60104);
        EXPECT(call(&b), ": base not 8-byte aligned");
    }
    {
        EXPECT(nvrx_segment_history_attribution_ragged(nullptr, none), ": null args");
        nvrx_seghistattr_args a{};
        segments(a);
        a.hist = fake<const uint32_t>(0x50000);
        a.permille = 990;
        attribution_outputs(a);
        auto call = [&](const nvrx_seghistattr_args* p) { return nvrx_segment_history_attribution_ragged(p, none); };
        attribution_cases(a, call);
        attribution_alignment_cases(a, call);
        nvrx_seghistattr_args b = a;
        b.hist_stride = 1;
        EXPECT(call(&b), ": hist_stride below K without hist_index");
        b = a;
        b.K = ((int64_t)1 << 31) / 240 + 1;
        b.R = 1;
        EXPECT(call(&b), ": K * 240 must be below 2^31");
    }
    {
        EXPECT(nvrx_segment_history_attribution_compact_ragged(nullptr, none), ": null args");
        nvrx_segchistattr_args a{};
        segments(a);
        a.chist = fake<const void>(0x50000);
        a.permille = 990;
        attribution_outputs(a);
        auto call = [&](const nvrx_segchistattr_args* p) {
            return nvrx_segment_history_attribution_compact_ragged(p, none);
        };
        attribution_cases(a, call);
        attribution_alignment_cases(a, call);
        nvrx_segchistattr_args b = a;
        b.chist = nullptr;
        EXPECT(call(&b), ": null chist");
        b = a;
        b.R = 1 << 16;
        b.K = 1 << 16;
        EXPECT(call(&b), ": R * K must be below 2^31");
    }
    {   // aging and conversion: slots, not columns
        uint64_t* const ev = fake<uint64_t>(0x70000);
        EXPECT(nvrx_compact_history_age(fake<void>(0x50000), -1, 4, 1, ev, nullptr, none), ": negative R");
        EXPECT(nvrx_compact_history_age(fake<void>(0x50000), 1 << 16, 1 << 16, 1, ev, nullptr, none),
               ": R * stride must be below 2^31");
        EXPECT(nvrx_compact_history_age(fake<void>(0x50000), 2, 4, 0, ev, nullptr, none), ": shift outside [1, 31]");
        EXPECT(nvrx_compact_history_age(nullptr, 2, 4, 1, ev, nullptr, none), ": null chist");
        EXPECT(nvrx_compact_history_age(fake<void>(0x50000), 2, 4, 1, ev, ev, none), ": full aliases evicted");
        EXPECT(nvrx_histogram_history_age(fake<uint32_t>(0x50000), 2, -4, 1, none), ": negative stride");
        EXPECT(nvrx_histogram_history_age(fake<uint32_t>(0x50000), 1, ((int64_t)1 << 31) / 240 + 1, 1, none),
               ": stride * 240 must be below 2^31");
        EXPECT(nvrx_histogram_history_age(fake<uint32_t>(0x50008), 2, 4, 1, none), ": hist not 16-byte aligned");
        EXPECT(nvrx_compact_history_from_dense(nullptr, fake<void>(0x50000), 2, 4, nullptr, none), ": null hist");
        EXPECT(nvrx_compact_history_from_dense(fake<const uint32_t>(0x60000), fake<void>(0x50000), 2, 4,
                                               fake<uint64_t>(0x70004), none),
               ": folded not 8-byte aligned");
        EXPECT(nvrx_compact_history_to_dense(fake<const void>(0x50008), fake<uint32_t>(0x60000), 2, 4, none),
               ": chist not 16-byte aligned");
    }
    std::printf("tail_checks_host: %d cases, %d failures\n", cases, failures);
    return failures != 0;
}
