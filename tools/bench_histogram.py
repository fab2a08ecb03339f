#!/usr/bin/env python3
"""Cost of the histogram kernel against the statistics kernel that reads the same bytes.

Shape: configs[1]'s matrix -- R x K segments of s_push pushed samples, the last `cap` retained.
In one process, interleaved, timed with HIP events:
  (a) ops.segment_stats_strided(mode=STATS_FAST)     the yardstick (unchanged code)
  (b) ops.segment_histogram_strided on the same input (synth.synth_matrix: every segment's
      samples cluster in one to three buckets, as a real kernel's durations do)
  (c) ops.segment_histogram_strided on spread input of the same shape (keys uniform over
      many octaves: nearly every sample of a wave in another bucket)
and, alone, (d) one segment of 2^20 samples (the one-workgroup kernel).
(b) against (c) is the cost of the counting; (b) / (a) the aim of DESIGN 3.10 (<= 1.0).
Prints one JSON line (and writes it to --out).  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nvidia-resiliency-ext-x_amd"))


def _summary(ms):
    s = sorted(ms)
    n = len(s)
    return dict(median_ms=statistics.median(s), min_ms=s[0], max_ms=s[-1],
                p10_ms=s[(n - 1) // 10], p90_ms=s[(9 * (n - 1)) // 10], n=n)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--R", type=int, default=64)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--s-push", type=int, default=10000)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--long-len", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nvidia_resiliency_ext.straggler import histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_histogram: no HIP device")
    dev = torch.device("cuda:0")
    nseg, S, cap = a.R * a.K, a.s_push, a.cap
    ns = synth.synth_matrix(a.R, a.K, S, device=dev).view(-1)
    # spread: 2^e + a uniform offset below 2^e, e uniform in [10, 30): 160 buckets in use
    g = torch.Generator(device=dev).manual_seed(240)
    spread = torch.empty(nseg * S, dtype=torch.int32, device=dev)
    chunk = 1 << 26
    for i in range(0, nseg * S, chunk):
        m = min(chunk, nseg * S - i)
        e = torch.randint(10, 30, (m,), generator=g, device=dev, dtype=torch.int64)
        frac = torch.randint(0, 1 << 30, (m,), generator=g, device=dev, dtype=torch.int64)
        spread[i:i + m] = ((1 << e) + (frac >> (30 - e))).to(torch.int32)
        del e, frac
    stats = ops.SegmentStats.empty(nseg, dev)
    hc = torch.empty((nseg, histograms.BINS), dtype=torch.int32, device=dev)
    hs = torch.empty((nseg, histograms.BINS), dtype=torch.int32, device=dev)
    legs = {
        "stats_fast": lambda: ops.segment_stats_strided(ns, nseg, S, 0, S, cap=cap, mode=ops.STATS_FAST,
                                                        out=stats),
        "histogram_clustered": lambda: ops.segment_histogram_strided(ns, nseg, S, 0, S, cap=cap, out=hc),
        "histogram_spread": lambda: ops.segment_histogram_strided(spread, nseg, S, 0, S, cap=cap, out=hs),
    }
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
    keep = min(S, cap)
    # every retained sample is counted once, and a few segments equal numpy's bincount
    assert bool((hc.sum(1) == keep).all()) and bool((hs.sum(1) == keep).all())
    used = {}
    for name, src, h in (("clustered", ns, hc), ("spread", spread, hs)):
        for s in (0, nseg // 2, nseg - 1):
            seg = src[s * S + S - keep: (s + 1) * S].cpu().numpy().view(np.uint32)
            want = np.bincount(histograms.bucket_of(seg), minlength=histograms.BINS)
            assert np.array_equal(h[s].cpu().numpy(), want), (name, s)
        nz = (h[:: max(1, nseg // 4096)] > 0).sum(1).float()
        used[name] = dict(mean=float(nz.mean()), max=int(nz.max()))

    # the one-workgroup kernel: one long segment
    L = a.long_len
    long_ns = torch.randint(1000, 3_000_000, (L,), dtype=torch.int32, device=dev)
    hl = torch.empty((1, histograms.BINS), dtype=torch.int32, device=dev)
    lt = []
    for it in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.segment_histogram_strided(long_ns, 1, L, 0, L, out=hl)
        e1.record()
        e1.synchronize()
        if it >= a.warmup:
            lt.append(e0.elapsed_time(e1))
    want = np.bincount(histograms.bucket_of(long_ns.cpu().numpy().view(np.uint32)), minlength=histograms.BINS)
    assert np.array_equal(hl[0].cpu().numpy(), want)

    res = {k: _summary(v) for k, v in times.items()}
    base = res["stats_fast"]["median_ms"]
    bytes_read = nseg * keep * 4
    line = dict(
        tool="bench_histogram", device=torch.cuda.get_device_name(0),
        shape=dict(R=a.R, K=a.K, s_push=S, cap=cap, nseg=nseg, bytes_read=bytes_read,
                   bytes_written=nseg * histograms.BINS * 4),
        warmup=a.warmup, reps=a.reps, **res,
        ratio_clustered_over_stats=res["histogram_clustered"]["median_ms"] / base,
        ratio_spread_over_stats=res["histogram_spread"]["median_ms"] / base,
        ratio_spread_over_clustered=res["histogram_spread"]["median_ms"] / res["histogram_clustered"]["median_ms"],
        read_gb_per_s={k: bytes_read / (v["median_ms"] * 1e-3) / 1e9 for k, v in res.items()},
        buckets_in_use_per_segment=used,
        long_segment=dict(samples=L, bytes=4 * L, **_summary(lt)),
    )
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
