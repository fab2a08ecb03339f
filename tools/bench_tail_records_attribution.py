#!/usr/bin/env python3
"""Cost of the tail score attribution of record streams (segment_tail_attribution.hip: the loss
per (rank, kernel) straight from the bucketed samples, no [R, K, 240] counts) against the row pass
it follows, against what a user had to do without it, and against the dense chain.

Streams: synth.synth_records over a Zipf push order (synth.zipf_counts / zipf_order: 47,482
records per rank at K = 2,048), R ranks, bucketed once by ops.records_bucket (every bucket written
out); fleet, thresholds and sums from the record-stream chain.  In one process, interleaved:
  a          ops.segment_tail_scores_ragged with tail_calls: the row pass on the same buckets
  b_top8 / b_top16   ops.histogram_tail_base + ops.segment_tail_attribution_ragged
  c          what ordering by tail_calls costs: a, the [R, K] u32 copy to a pinned host buffer and
             a stable descending argsort per row there (wall clock around all three; the other
             legs are timed with HIP events)
  d_top8 / d_top16   (--dense) ops.segment_histogram_ragged into the counts + histogram_tail_base +
             histogram_tail_attribution(kind="relative"): the dense chain on the same buckets
Prints one JSON line (and writes it to --out).  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nvidia-resiliency-ext-x_amd"))

TOPS = (8, 16)


def _summary(ms):
    s = sorted(ms)
    n = len(s)
    return dict(median_ms=statistics.median(s), min_ms=s[0], max_ms=s[-1],
                p10_ms=s[(n - 1) // 10], p90_ms=s[(9 * (n - 1)) // 10], n=n)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--R", type=int, default=1024)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--permille", type=int, default=990)
    ap.add_argument("--dense", action="store_true", help="also time the dense chain (R * K * 960 B)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nvidia_resiliency_ext.straggler import histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_tail_records_attribution: no HIP device")
    dev = torch.device("cuda:0")
    R, K, cap, pm, B = a.R, a.K, a.cap, a.permille, histograms.BINS
    calls_per = synth.zipf_counts(K)
    slot, occ = synth.zipf_order(calls_per)
    N = slot.size
    t32 = lambda x: torch.from_numpy(x.view(np.int32)).to(dev)  # noqa: E731
    recs = synth.synth_records(R, t32(slot), t32(occ), K, int(calls_per.max()))
    rec_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * N
    need = ops.records_bucket_capacity(R * N, R, K)
    bucket = (torch.empty(R * K, dtype=torch.int64, device=dev),
              torch.empty(R * K, dtype=torch.int32, device=dev),
              torch.empty(max(need, 1), dtype=torch.int32, device=dev),
              torch.empty(R * K, dtype=torch.int32, device=dev))
    seg_off, seg_len, out_ns, _ = ops.records_bucket(recs, rec_off, K, cap, out=bucket)
    del recs
    assert int(seg_len.min()) >= 0
    max_len = int(seg_len.max())
    samples = int(seg_len.sum(dtype=torch.int64))
    lane_class = int(((seg_len > 0) & (seg_len <= 16)).sum())
    wave_class = int((seg_len > 16).sum())
    fleet = ops.segment_fleet_histogram_ragged(out_ns, seg_off, seg_len, K, max_len, aligned16=True)
    thr, sums = ops.histogram_tail_threshold(fleet, pm)

    score = ops.TailScores(torch.empty(R, dtype=torch.float64, device=dev),
                           torch.empty(R, dtype=torch.int64, device=dev),
                           torch.empty(R, dtype=torch.int64, device=dev),
                           torch.empty(R, dtype=torch.uint8, device=dev))
    calls = torch.empty((R, K), dtype=torch.int32, device=dev)
    host_calls = torch.empty((R, K), dtype=torch.int32).pin_memory()
    base = torch.empty((K, 2), dtype=torch.int64, device=dev)
    loss_all = torch.empty((R, K), dtype=torch.float64, device=dev)
    new = {t: ops.TailAttribution.packed(torch.empty(ops.TailAttribution.PACKED * R * t, dtype=torch.uint8,
                                                     device=dev), R, t, loss_all) for t in TOPS}

    def leg_a():
        ops.segment_tail_scores_ragged(out_ns, seg_off, seg_len, K, max_len, thr, sums, aligned16=True,
                                       out=score, tail_calls=calls)

    def leg_b(top):
        ops.histogram_tail_base(fleet, thr, out=base)
        ops.segment_tail_attribution_ragged(out_ns, seg_off, seg_len, K, max_len, thr, base, top=top,
                                            aligned16=True, out=new[top])

    def leg_c():
        leg_a()
        host_calls.copy_(calls, non_blocking=True)
        torch.cuda.synchronize()
        # descending by count, ties to the lower column: ~x reverses the order of u32
        return np.argsort(~host_calls.numpy().view(np.uint32), axis=1, kind="stable")

    legs = {"a": leg_a}
    for t in TOPS:
        legs[f"b_top{t}"] = lambda t=t: leg_b(t)
    if a.dense:
        counts = torch.zeros((R * K, B), dtype=torch.int32, device=dev)
        dloss = torch.empty((R, K), dtype=torch.float64, device=dev)
        dense = {t: ops.TailAttribution.packed(torch.empty(ops.TailAttribution.PACKED * R * t,
                                                           dtype=torch.uint8, device=dev), R, t, dloss)
                 for t in TOPS}

        def leg_d(top):
            ops.segment_histogram_ragged(out_ns, seg_off, seg_len, max_len, aligned16=True, out=counts)
            ops.histogram_tail_base(fleet, thr, out=base)
            ops.histogram_tail_attribution(counts.view(R, K, B), top=top, kind="relative", thr=thr,
                                           base=base, out=dense[top])

        for t in TOPS:
            legs[f"d_top{t}"] = lambda t=t: leg_d(t)
    times = {k: [] for k in legs}
    times["c"] = []
    for it in range(a.warmup + a.reps):
        for name, fn in legs.items():  # interleaved: every leg sees the same drift
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        order = leg_c()
        if it >= a.warmup:
            times["c"].append((time.perf_counter() - t0) * 1e3)
        if it % 5 == 4:
            print(f"bench_tail_records_attribution: {it + 1} of {a.warmup + a.reps}", file=sys.stderr,
                  flush=True)
    # what was timed is right: the dense chain's bits, and top 8 is the head of top 16
    torch.cuda.synchronize()
    assert torch.equal(new[8].idx, new[16].idx[:, :8])
    if a.dense:
        for t in TOPS:
            for f in ("idx", "tail_ns", "total_ns", "tail_calls", "thr_bucket"):
                assert torch.equal(getattr(new[t], f), getattr(dense[t], f)), (t, f)
            for f in ("loss", "base_share"):
                x, y = getattr(new[t], f), getattr(dense[t], f)
                assert torch.equal(torch.isnan(x), torch.isnan(y)), (t, f)
                assert torch.equal(x.nan_to_num(0.0).view(torch.int64), y.nan_to_num(0.0).view(torch.int64)), (t, f)
    idx16 = new[16].idx.cpu().numpy()
    differs = float((order[:, 0] != idx16[:, 0]).mean())  # rows a count and the cost order differently

    res = {k: _summary(v) for k, v in times.items()}
    med = {k: res[k]["median_ms"] for k in times}
    line = dict(
        tool="bench_tail_records_attribution", device=torch.cuda.get_device_name(0),
        shape=dict(R=R, K=K, cap=cap, permille=pm, records=R * N, retained_samples=samples,
                   longest_bucket=max_len, lane_class_segments=lane_class,
                   wave_class_segments=wave_class, tail_calls_bytes=4 * R * K,
                   loss_all_bytes=8 * R * K, dense_counts_bytes=R * K * B * 4),
        warmup=a.warmup, reps=a.reps, **res,
        ratio_b_over_a={f"top{t}": med[f"b_top{t}"] / med["a"] for t in TOPS},
        ratio_b_over_c={f"top{t}": med[f"b_top{t}"] / med["c"] for t in TOPS},
        rows_whose_first_kernel_differs_by_count=differs,
    )
    if a.dense:
        line["ratio_b_over_d"] = {f"top{t}": med[f"b_top{t}"] / med[f"d_top{t}"] for t in TOPS}
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
