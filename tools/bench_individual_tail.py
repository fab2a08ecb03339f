#!/usr/bin/env python3
"""Cost of the individual tail scores (a rank against its own histogram history) against the bare
add that moves the same bytes.

Counts: MatrixReporter.histograms over synth.synth_matrix, R rows x K kernels x 240 u32 (built in
blocks of rows, a fresh seed per block); the history starts as one such interval.  In one process,
interleaved, timed with HIP events:
  (a) hist += counts (torch)                      the yardstick: reads 960 + 960 B and writes 960 B
                                                  per (row, kernel) and does none of the work
  (b) ops.histogram_history_scores                SCORE | UPDATE fused, the same 2,880 B
  (c) ops.histogram_history_scores(update=False)  SCORE only, 1,920 B
  (c0) ops.histogram_tail_scores                  the relative score on the same counts, 960 B
  (d) ops.histogram_history_scores(score=False)   UPDATE only, 2,880 B
  (e) (b) with tail_calls
Each leg's floor is its bytes at the float4 copy rate of DESIGN 3 (6.3 TB/s).  Prints one JSON line
(and writes it to --out).  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nvidia-resiliency-ext-x_amd"))

COPY_TB_S = 6.3  # measured float4 copy rate
PASSES = dict(a_torch_add=3, b_fused=3, c_score_only=2, c0_relative_tail_scores=1, d_update_only=3,
              e_fused_calls=3)  # 960-byte passes per (row, kernel)


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
        raise SystemExit("bench_individual_tail: no HIP device")
    dev = torch.device("cuda:0")
    R, K, S, B, pm = a.R, a.K, a.s_push, histograms.BINS, a.permille
    counts = torch.empty((R, K, B), dtype=torch.int32, device=dev)
    for r0 in range(0, R, a.block):
        n = min(a.block, R - r0)
        ns = synth.synth_matrix(n, K, S, seed=synth.SEED + r0, device=dev)
        batch.MatrixReporter(n, K, cap=S, device=dev).histograms(ns, S, out=counts[r0:r0 + n])
    del ns
    hist = counts.clone()       # the kernels' history
    hist_torch = counts.clone()  # leg (a)'s own
    out = ops.HistoryTailScores.empty(R, dev)
    calls = torch.empty((R, K), dtype=torch.int32, device=dev)
    fleet = ops.histogram_sum(counts)
    thr, sums = ops.histogram_tail_threshold(fleet, pm)
    rel = ops.TailScores(torch.empty(R, dtype=torch.float64, device=dev),
                         torch.empty(R, dtype=torch.int64, device=dev),
                         torch.empty(R, dtype=torch.int64, device=dev),
                         torch.empty(R, dtype=torch.uint8, device=dev))

    legs = {
        "a_torch_add": lambda: hist_torch.add_(counts),
        "b_fused": lambda: ops.histogram_history_scores(counts, hist, permille=pm, out=out),
        "c_score_only": lambda: ops.histogram_history_scores(counts, hist, permille=pm, update=False, out=out),
        "c0_relative_tail_scores": lambda: ops.histogram_tail_scores(counts, thr, sums, out=rel),
        "d_update_only": lambda: ops.histogram_history_scores(counts, hist, permille=pm, score=False),
        "e_fused_calls": lambda: ops.histogram_history_scores(counts, hist, permille=pm, out=out,
                                                              tail_calls=calls),
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
    # what was timed is right: three updates per iteration went into the history, and on fresh
    # copies of a few rows the fused call equals the host twin
    n_upd = 3 * (a.warmup + a.reps)
    assert torch.equal(hist[R - 1], counts[R - 1] * (n_upd + 1))
    for r in (0, R // 2, R - 1):
        c, h = counts[r:r + 1].contiguous(), (counts[r:r + 1] * 2).contiguous()
        want = histograms.history_scores(c.cpu().numpy(), h.cpu().numpy(), pm)
        got = ops.histogram_history_scores(c, h, permille=pm, tail_calls=True)
        assert got.score.cpu().numpy().view(np.uint64).tolist() == want.score.view(np.uint64).tolist()
        assert got.tail_ns.cpu().numpy().view(np.uint64).tolist() == want.tail_ns.tolist()
        assert got.tail_calls.cpu().numpy().view(np.uint32).tolist() == want.tail_calls.tolist()
        assert np.array_equal(h.cpu().numpy().view(np.uint32), want.hist)

    res = {k: _summary(v) for k, v in times.items()}
    pass_bytes = R * K * B * 4
    floor = {k: PASSES[k] * pass_bytes / (COPY_TB_S * 1e12) * 1e3 for k in legs}
    med = {k: res[k]["median_ms"] for k in legs}
    score = out.score.cpu().numpy()
    line = dict(
        tool="bench_individual_tail", device=torch.cuda.get_device_name(0),
        shape=dict(R=R, K=K, s_push=S, permille=pm, bytes_per_pass=pass_bytes, passes=PASSES),
        warmup=a.warmup, reps=a.reps, **res,
        copy_floor_ms=floor,
        fraction_of_copy_rate={k: floor[k] / med[k] for k in legs},
        gb_per_s={k: PASSES[k] * pass_bytes / (med[k] * 1e-3) / 1e9 for k in legs},
        ratio_b_over_a=med["b_fused"] / med["a_torch_add"],
        ratio_b_over_c_plus_d=med["b_fused"] / (med["c_score_only"] + med["d_update_only"]),
        ratio_c_over_c0=med["c_score_only"] / med["c0_relative_tail_scores"],
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
