#!/usr/bin/env python3
"""Cost of the tail-score kernels against the expression the docs recommended for the fleet.

Counts: MatrixReporter.histograms over synth.synth_matrix, R rows x K kernels x 240 u32 (built in
blocks of rows, a fresh seed per block).  In one process, interleaved, timed with HIP events:
  (a) counts.sum(0, dtype=torch.int64)          the yardstick for (b)
  (b) ops.histogram_sum                         entry 1
  (c) ops.histogram_tail_threshold              entry 2
  (d) ops.histogram_tail_scores                 entry 3 without tail_calls
  (e) ops.histogram_tail_scores(tail_calls=)    entry 3 with tail_calls
(b) and (d) read 960 B per (row, kernel) once: their floor is that at the float4 copy rate of
DESIGN 3 (6.3 TB/s).  Prints one JSON line (and writes it to --out).  Needs a GPU: no fallback.
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
    ap.add_argument("--R", type=int, default=64)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--s-push", type=int, default=256)
    ap.add_argument("--block", type=int, default=64, help="rows per synth block")
    ap.add_argument("--permille", type=int, default=990)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nvidia_resiliency_ext.straggler import batch, histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_tail_scores: no HIP device")
    dev = torch.device("cuda:0")
    R, K, S, B = a.R, a.K, a.s_push, histograms.BINS
    counts = torch.empty((R, K, B), dtype=torch.int32, device=dev)
    for r0 in range(0, R, a.block):
        n = min(a.block, R - r0)
        ns = synth.synth_matrix(n, K, S, seed=synth.SEED + r0, device=dev)
        batch.MatrixReporter(n, K, cap=S, device=dev).histograms(ns, S, out=counts[r0:r0 + n])
    del ns
    fleet = torch.empty((K, B), dtype=torch.int64, device=dev)
    thr = torch.empty(K, dtype=torch.int32, device=dev)
    sums = torch.empty(2, dtype=torch.int64, device=dev)
    out = ops.TailScores(torch.empty(R, dtype=torch.float64, device=dev),
                         torch.empty(R, dtype=torch.int64, device=dev),
                         torch.empty(R, dtype=torch.int64, device=dev),
                         torch.empty(R, dtype=torch.uint8, device=dev))
    calls = torch.empty((R, K), dtype=torch.int32, device=dev)
    keep = {}

    def torch_sum():
        keep["torch"] = counts.sum(0, dtype=torch.int64)

    legs = {
        "a_torch_sum": torch_sum,
        "b_histogram_sum": lambda: ops.histogram_sum(counts, out=fleet),
        "c_tail_threshold": lambda: ops.histogram_tail_threshold(fleet, a.permille, thr=thr, fleet_sums=sums),
        "d_tail_scores": lambda: ops.histogram_tail_scores(counts, thr, sums, out=out),
        "e_tail_scores_calls": lambda: ops.histogram_tail_scores(counts, thr, sums, out=out, tail_calls=calls),
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
    # what was timed is right: the fleet is torch's sum, a few rows equal the numpy helper
    assert torch.equal(fleet, keep["torch"])
    assert int(fleet.sum()) == R * K * S
    T = histograms.tail_threshold(fleet.cpu().numpy(), a.permille)
    assert thr.cpu().numpy().tolist() == T.tolist()
    w = np.asarray(histograms.weights(), dtype=object)
    for r in (0, R // 2, R - 1):
        c = counts[r].cpu().numpy().view(np.uint32).astype(object)
        above = np.arange(B)[None, :] > T[:, None]
        assert int(out.total_ns[r]) == int((c * w).sum())
        assert int(out.tail_ns[r]) == int((c * w * above).sum())
        assert calls[r].cpu().numpy().tolist() == (c * above).sum(1).tolist()

    res = {k: _summary(v) for k, v in times.items()}
    row_bytes = R * K * B * 4
    floor_ms = row_bytes / (COPY_TB_S * 1e12) * 1e3
    score = out.score.cpu().numpy()
    line = dict(
        tool="bench_tail_scores", device=torch.cuda.get_device_name(0),
        shape=dict(R=R, K=K, s_push=S, permille=a.permille, bytes_read_per_pass=row_bytes),
        warmup=a.warmup, reps=a.reps, **res,
        ratio_b_over_a=res["b_histogram_sum"]["median_ms"] / res["a_torch_sum"]["median_ms"],
        copy_floor_ms=floor_ms,
        fraction_of_copy_rate={k: floor_ms / res[k]["median_ms"]
                               for k in ("a_torch_sum", "b_histogram_sum", "d_tail_scores",
                                         "e_tail_scores_calls")},
        read_gb_per_s={k: row_bytes / (res[k]["median_ms"] * 1e-3) / 1e9
                       for k in ("a_torch_sum", "b_histogram_sum", "d_tail_scores",
                                 "e_tail_scores_calls")},
        score=dict(min=float(np.nanmin(score)), max=float(np.nanmax(score))),
    )
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
