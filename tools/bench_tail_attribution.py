#!/usr/bin/env python3
"""Cost of the tail score attribution (the kernels behind a rank's tail score) against what a user
had to do before it existed, and against the bytes it moves.

Counts: MatrixReporter.histograms over synth.synth_matrix, R rows x K kernels x 240 u32 (built in
blocks of rows, a fresh seed per block); the history is one such interval.  In one process,
interleaved, timed with HIP events (host legs with a wall clock around a synchronised region):
  rel        ops.histogram_tail_base + histogram_tail_attribution(kind="relative")   960 B + 16 B
  ind        ops.histogram_tail_attribution(kind="individual")                     1,920 B + 16 B
  rel_old    what a user did before: histogram_tail_scores(tail_calls=True), the [R, K] u32 copied
             to the host, ordered there (numpy argsort per row) -- by calls, not by cost
  ind_old    the same with histogram_history_scores(update=False, tail_calls=True)
  rel_score / ind_score   the score-only calls on the same bytes, for scale
Each leg's floor is its bytes at the float4 copy rate of DESIGN 3 (6.3 TB/s): 960 B (relative) or
1,920 B (individual) per (row, kernel) plus 16 B for loss_all written and read.  Prints one JSON
line (and writes it to --out).  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--permille", type=int, default=950)
    ap.add_argument("--top", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nvidia_resiliency_ext.straggler import batch, histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_tail_attribution: no HIP device")
    dev = torch.device("cuda:0")
    R, K, S, B, pm, top = a.R, a.K, a.s_push, histograms.BINS, a.permille, a.top
    counts = torch.empty((R, K, B), dtype=torch.int32, device=dev)
    hist = torch.empty((R, K, B), dtype=torch.int32, device=dev)
    for r0 in range(0, R, a.block):
        n = min(a.block, R - r0)
        rep = batch.MatrixReporter(n, K, cap=S, device=dev)
        rep.histograms(synth.synth_matrix(n, K, S, seed=synth.SEED + r0, device=dev), S,
                       out=counts[r0:r0 + n])
        rep.histograms(synth.synth_matrix(n, K, S, seed=synth.SEED + R + r0, device=dev), S,
                       out=hist[r0:r0 + n])
    fleet = ops.histogram_sum(counts)
    thr, sums = ops.histogram_tail_threshold(fleet, pm)
    base = torch.empty((K, 2), dtype=torch.int64, device=dev)
    out_rel = ops.TailAttribution.empty(R, K, top, dev)
    out_ind = ops.TailAttribution.empty(R, K, top, dev)
    calls = torch.empty((R, K), dtype=torch.int32, device=dev)
    rel = ops.TailScores(torch.empty(R, dtype=torch.float64, device=dev),
                         torch.empty(R, dtype=torch.int64, device=dev),
                         torch.empty(R, dtype=torch.int64, device=dev),
                         torch.empty(R, dtype=torch.uint8, device=dev))
    ind = ops.HistoryTailScores.empty(R, dev)

    def new_rel():
        ops.histogram_tail_base(fleet, thr, out=base)
        ops.histogram_tail_attribution(counts, top=top, kind="relative", thr=thr, base=base, out=out_rel)

    def new_ind():
        ops.histogram_tail_attribution(counts, top=top, kind="individual", hist=hist, permille=pm,
                                       out=out_ind)

    def order(c):
        h = c.cpu().numpy().view(np.uint32)
        return np.argsort(-h.astype(np.int64), axis=1, kind="stable")[:, :top]

    def old_rel():
        ops.histogram_tail_scores(counts, thr, sums, out=rel, tail_calls=calls)
        return order(calls)

    def old_ind():
        ops.histogram_history_scores(counts, hist, permille=pm, update=False, out=ind, tail_calls=calls)
        return order(calls)

    device_legs = {
        "rel": new_rel, "ind": new_ind,
        "rel_score": lambda: ops.histogram_tail_scores(counts, thr, sums, out=rel),
        "ind_score": lambda: ops.histogram_history_scores(counts, hist, permille=pm, update=False, out=ind),
    }
    host_legs = {"rel_old": old_rel, "ind_old": old_ind}
    times = {k: [] for k in list(device_legs) + list(host_legs)}
    for it in range(a.warmup + a.reps):
        for name, fn in device_legs.items():  # interleaved: every leg sees the same drift
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
        for name, fn in host_legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()  # ends with the host ordering: synchronised by its copy
            if it >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    # what was timed is right: on a few rows both legs equal the host twins
    rows = sorted({0, R // 2, R - 1})
    c = counts.cpu().numpy().view(np.uint32)[rows]
    want = histograms.tail_attribution(c, pm, top, fleet=fleet.cpu().numpy())
    assert np.array_equal(out_rel.idx.cpu().numpy()[rows], want.idx)
    assert np.array_equal(out_rel.loss.cpu().numpy()[rows], want.loss, equal_nan=True)
    want = histograms.history_attribution(c, hist.cpu().numpy().view(np.uint32)[rows], pm, top)
    assert np.array_equal(out_ind.idx.cpu().numpy()[rows], want.idx)
    assert np.array_equal(out_ind.loss.cpu().numpy()[rows], want.loss, equal_nan=True)

    res = {k: _summary(v) for k, v in times.items()}
    med = {k: res[k]["median_ms"] for k in times}
    per = dict(rel=960 + 16, ind=1920 + 16, rel_score=960, ind_score=1920)
    floor = {k: R * K * v / (COPY_TB_S * 1e12) * 1e3 for k, v in per.items()}
    line = dict(
        tool="bench_tail_attribution", device=torch.cuda.get_device_name(0),
        shape=dict(R=R, K=K, s_push=S, permille=pm, top=top, bytes_per_element=per),
        warmup=a.warmup, reps=a.reps, **res, copy_floor_ms=floor,
        fraction_of_copy_rate={k: floor[k] / med[k] for k in per},
        ratio_rel_over_old=med["rel"] / med["rel_old"], ratio_ind_over_old=med["ind"] / med["ind_old"],
        ratio_rel_over_score=med["rel"] / med["rel_score"],
        ratio_ind_over_score=med["ind"] / med["ind_score"],
        d2h_bytes=dict(new=ops.TailAttribution.PACKED * R * top, old=4 * R * K),
    )
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
