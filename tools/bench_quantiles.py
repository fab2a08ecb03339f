#!/usr/bin/env python3
"""Cost of the quantile kernels against the statistics kernel that reads the same bytes.

Shape: configs[1]'s matrix -- R x K segments of s_push pushed samples, the last `cap` retained,
built on the device by synth.synth_matrix.  In one process, interleaved, timed with HIP events:
  (a) ops.segment_stats_strided(mode=STATS_FAST)        the yardstick (unchanged code)
  (b) ops.segment_quantiles_strided((500, 900, 990))
  (c) ops.segment_quantiles_strided with 8 quantiles
and, for information, the streaming path on one segment of 2^20 samples (4 passes over it).
Prints one JSON line (and writes it to --out).  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nvidia-resiliency-ext-x_amd"))

PM3 = (500, 900, 990)
PM8 = (0, 1, 250, 500, 900, 990, 999, 1000)


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
    ap.add_argument("--stream-len", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from nvidia_resiliency_ext.straggler import ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_quantiles: no HIP device")
    dev = torch.device("cuda:0")
    nseg, S, cap = a.R * a.K, a.s_push, a.cap
    ns = synth.synth_matrix(a.R, a.K, S, device=dev).view(-1)
    stats = ops.SegmentStats.empty(nseg, dev)
    q3 = torch.empty((len(PM3), nseg), dtype=torch.float32, device=dev)
    q8 = torch.empty((len(PM8), nseg), dtype=torch.float32, device=dev)
    legs = {
        "stats_fast": lambda: ops.segment_stats_strided(ns, nseg, S, 0, S, cap=cap, mode=ops.STATS_FAST,
                                                        out=stats),
        "quantiles_3": lambda: ops.segment_quantiles_strided(ns, nseg, S, 0, S, PM3, cap=cap, out=q3),
        "quantiles_8": lambda: ops.segment_quantiles_strided(ns, nseg, S, 0, S, PM8, cap=cap, out=q8),
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
    # the rows the legs share agree (MED of an even n averages two samples: compare MIN / MAX)
    assert torch.equal(q8[0], stats.min) and torch.equal(q8[7], stats.max)
    assert torch.equal(q8[3], q3[0]) and torch.equal(q8[4], q3[1]) and torch.equal(q8[5], q3[2])

    # streaming path: one long segment, re-read once per pass
    L = a.stream_len
    long_ns = torch.randint(1000, 3_000_000, (L,), dtype=torch.int32, device=dev)
    qs = torch.empty((len(PM3), 1), dtype=torch.float32, device=dev)
    st = []
    for it in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.segment_quantiles_strided(long_ns, 1, L, 0, L, PM3, out=qs)
        e1.record()
        e1.synchronize()
        if it >= a.warmup:
            st.append(e0.elapsed_time(e1))
    # checked on the host: np.sort of the keys, the integer rank, (float)ns / 1000.0f
    import numpy as np

    srt = np.sort(long_ns.cpu().numpy().view(np.uint32))
    want = np.array([srt[(p * (L - 1)) // 1000] for p in PM3]).astype(np.float32) / np.float32(1000)
    assert np.array_equal(qs[:, 0].cpu().numpy().view(np.uint32), want.view(np.uint32))

    res = {k: _summary(v) for k, v in times.items()}
    base = res["stats_fast"]["median_ms"]
    bytes_read = nseg * min(S, cap) * 4
    line = dict(
        tool="bench_quantiles", device=torch.cuda.get_device_name(0),
        shape=dict(R=a.R, K=a.K, s_push=S, cap=cap, nseg=nseg, bytes_read=bytes_read),
        warmup=a.warmup, reps=a.reps, **res,
        ratio_q3_over_stats=res["quantiles_3"]["median_ms"] / base,
        ratio_q8_over_stats=res["quantiles_8"]["median_ms"] / base,
        read_gb_per_s={k: bytes_read / (v["median_ms"] * 1e-3) / 1e9 for k, v in res.items()},
        streaming=dict(samples=L, passes=4, bytes_per_pass=4 * L, bytes_reread=16 * L, **_summary(st)),
    )
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
