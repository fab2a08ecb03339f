#!/usr/bin/env python3
"""Cost of the tail scores of record streams (segment_tail.hip: two passes over the bucketed
samples, no [R, K, 240] counts) against the dense chain they replace and against the bytes they
move.

Streams: synth.synth_records over a Zipf push order (synth.zipf_counts / zipf_order: 47,482
records per rank at K = 2,048), R ranks, bucketed once by ops.records_bucket (every bucket written
out).  In one process, interleaved, timed with HIP events:
  bucket       ops.records_bucket alone
  fleet        ops.segment_fleet_histogram_ragged
  tail         ops.segment_tail_scores_ragged
  tail_calls   the same with tail_calls
  stats        ops.segment_stats_ragged on the same buckets (the class kernels of a report), for scale
  dense_hist / dense_sum / dense_tail   (--dense) ops.segment_histogram_ragged into the counts,
               ops.histogram_sum, ops.histogram_tail_scores: the chain on the same buckets
Floor of a pass: 4 B per retained sample + 12 B per segment at the float4 copy rate of DESIGN 3
(6.3 TB/s).  Prints one JSON line (and writes it to --out).  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nvidia-resiliency-ext-x_amd"))

COPY_TB_S = 6.3  # measured float4 copy rate


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
        raise SystemExit("bench_tail_records: no HIP device")
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
    assert int(seg_len.min()) >= 0
    max_len = int(seg_len.max())
    samples = int(seg_len.sum(dtype=torch.int64))
    fleet = torch.empty((K, B), dtype=torch.int64, device=dev)
    ops.segment_fleet_histogram_ragged(out_ns, seg_off, seg_len, K, max_len, aligned16=True, out=fleet)
    thr, sums = ops.histogram_tail_threshold(fleet, pm)

    def scores():
        return ops.TailScores(torch.empty(R, dtype=torch.float64, device=dev),
                              torch.empty(R, dtype=torch.int64, device=dev),
                              torch.empty(R, dtype=torch.int64, device=dev),
                              torch.empty(R, dtype=torch.uint8, device=dev))

    new, new_c, calls = scores(), scores(), torch.empty((R, K), dtype=torch.int32, device=dev)
    stats = ops.SegmentStats.empty(R * K, dev)
    legs = {
        "bucket": lambda: ops.records_bucket(recs, rec_off, K, cap, out=bucket),
        "fleet": lambda: ops.segment_fleet_histogram_ragged(out_ns, seg_off, seg_len, K, max_len,
                                                            aligned16=True, out=fleet),
        "tail": lambda: ops.segment_tail_scores_ragged(out_ns, seg_off, seg_len, K, max_len, thr, sums,
                                                       aligned16=True, out=new),
        "tail_calls": lambda: ops.segment_tail_scores_ragged(out_ns, seg_off, seg_len, K, max_len, thr,
                                                             sums, aligned16=True, out=new_c,
                                                             tail_calls=calls),
        "stats": lambda: ops.segment_stats_ragged(out_ns, seg_off, seg_len, max_len, aligned16=True,
                                                  out=stats),
    }
    if a.dense:
        counts = torch.zeros((R * K, B), dtype=torch.int32, device=dev)
        dfleet = torch.empty((K, B), dtype=torch.int64, device=dev)
        dense = scores()
        legs["dense_hist"] = lambda: ops.segment_histogram_ragged(out_ns, seg_off, seg_len, max_len,
                                                                  aligned16=True, out=counts)
        legs["dense_sum"] = lambda: ops.histogram_sum(counts.view(R, K, B), out=dfleet)
        legs["dense_tail"] = lambda: ops.histogram_tail_scores(counts.view(R, K, B), thr, sums, out=dense)
    times = {k: [] for k in legs}
    for it in range(a.warmup + a.reps):
        for name, fn in legs.items():  # interleaved: every leg sees the same drift
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    # what was timed is right: with and without tail_calls agree, and with the dense chain
    assert torch.equal(new.score.view(torch.int64), new_c.score.view(torch.int64))
    if a.dense:
        assert torch.equal(fleet, dfleet)
        assert torch.equal(new.score.view(torch.int64), dense.score.view(torch.int64))
        assert torch.equal(new.tail_ns, dense.tail_ns) and torch.equal(new.total_ns, dense.total_ns)

    res = {k: _summary(v) for k, v in times.items()}
    med = {k: res[k]["median_ms"] for k in times}
    pass_bytes = 4 * samples + 12 * R * K
    floor = pass_bytes / (COPY_TB_S * 1e12) * 1e3
    line = dict(
        tool="bench_tail_records", device=torch.cuda.get_device_name(0),
        shape=dict(R=R, K=K, cap=cap, permille=pm, records=R * N, retained_samples=samples,
                   longest_bucket=max_len, records_bytes=8 * R * N, dense_counts_bytes=R * K * B * 4,
                   pass_bytes=pass_bytes),
        warmup=a.warmup, reps=a.reps, **res, pass_floor_ms=floor,
        fraction_of_copy_rate={k: floor / med[k] for k in ("fleet", "tail", "tail_calls")},
        new_ms=med["fleet"] + med["tail"],
    )
    if a.dense:
        line["dense_ms"] = med["dense_hist"] + med["dense_sum"] + med["dense_tail"]
        line["ratio_new_over_dense"] = line["new_ms"] / line["dense_ms"]
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
