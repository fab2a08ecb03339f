#!/usr/bin/env python3
"""Cost of the individual tail score attribution of [R, K, 240] counts against the compact history
(histogram_history_compact_attribution.hip: 64 B per (rank, kernel)) next to the dense-history
entry (histogram_attribution.hip, kind individual: 960 B) on the same inputs, in the same process.

Counts: MatrixReporter.histograms over synth.synth_matrix (R ranks, K kernels, S pushes), built in
row blocks.  The history is one such interval, absorbed once by the compact update; nothing may
fold there, and the dense history is its expansion (ops.compact_history_to_dense).  Before
anything is timed the new entry's outputs are compared with the dense entry's, byte for byte.
Per shape of --shapes, interleaved, timed with HIP events:
  compact_attribution   ops.histogram_history_attribution_compact, top --top
  dense_attribution     ops.histogram_tail_attribution(kind="individual") on the expanded history
Bytes of an attribution per element: the counts (960 B), the history (64 B / 960 B), loss_all
written by the loss kernel (8 B); the select kernel's read of loss_all and the winners' second
read are left out of the figure (8 B per element, top per row).  Prints one JSON line (and writes
it to --out).  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nvidia-resiliency-ext-x_amd"))

COPY_TB_S = 6.3  # measured float4 copy rate
FIELDS = ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share", "loss_all")
BLOCK = 512  # rows of counts built at a time


def _summary(ms):
    s = sorted(ms)
    n = len(s)
    return dict(median_ms=statistics.median(s), min_ms=s[0], max_ms=s[-1],
                p10_ms=s[(n - 1) // 10], p90_ms=s[(9 * (n - 1)) // 10], n=n)


def one_shape(R, K, a, torch, batch, histograms, ops, synth, dev):
    S, pm, top, B, CB = a.S, a.permille, a.top, histograms.BINS, histograms.CHIST_BYTES
    counts = torch.empty((R, K, B), dtype=torch.int32, device=dev)
    for r0 in range(0, R, BLOCK):
        n = min(BLOCK, R - r0)
        ns = synth.synth_matrix(n, K, S, seed=synth.SEED + r0, device=dev)
        batch.MatrixReporter(n, K, cap=S, device=dev).histograms(ns, S, out=counts[r0:r0 + n])
        del ns
    chist = torch.zeros((R, K, CB), dtype=torch.uint8, device=dev)
    folded = torch.zeros(R, dtype=torch.int64, device=dev)
    ops.histogram_history_scores_compact(counts, chist, permille=pm, score=False, folded=folded)
    if int(folded.sum()):
        raise SystemExit("bench_compact_counts_attribution: the history interval folded; the dense "
                         "history would not be the expansion of the compact one")
    hist = ops.compact_history_to_dense(chist)
    entries = chist.view(torch.int32)[:, :, -1]  # n of every element
    out_c = ops.TailAttribution.empty(R, K, top, dev)
    out_d = ops.TailAttribution.empty(R, K, top, dev)
    legs = {
        "compact_attribution": lambda: ops.histogram_history_attribution_compact(
            counts, chist, permille=pm, top=top, out=out_c),
        "dense_attribution": lambda: ops.histogram_tail_attribution(
            counts, kind="individual", hist=hist, permille=pm, top=top, out=out_d),
    }
    # what is timed is right: the two entries give the same bytes
    for f in FIELDS:
        getattr(out_c, f).view(torch.uint8).fill_(0x5A)
        getattr(out_d, f).view(torch.uint8).fill_(0xA5)
    for leg in legs.values():
        leg()
    for f in FIELDS:
        x, y = getattr(out_c, f), getattr(out_d, f)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f
    taken = int((out_c.idx >= 0).sum())
    times = {k: [] for k in legs}
    for it in range(a.warmup + a.reps):
        for name, leg in legs.items():  # interleaved: every leg sees the same drift
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            leg()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    res = {k: _summary(v) for k, v in times.items()}
    med = {k: res[k]["median_ms"] for k in times}
    per = dict(compact_attribution=4 * B + CB + 8, dense_attribution=8 * B + 8)
    nbytes = {k: v * R * K for k, v in per.items()}
    return dict(
        shape=dict(R=R, K=K, S=S, permille=pm, top=top, counts_bytes=R * K * B * 4,
                   compact_history_bytes=R * K * CB, dense_history_bytes=R * K * B * 4,
                   entries_mean=float(entries.float().mean()), entries_max=int(entries.max()),
                   winners_taken=taken),
        outputs_equal_dense=True, **res, bytes=nbytes, bytes_per_element=per,
        floor_ms={k: v / (COPY_TB_S * 1e12) * 1e3 for k, v in nbytes.items()},
        fraction_of_copy_rate={k: v / (COPY_TB_S * 1e12) * 1e3 / med[k] for k, v in nbytes.items()},
        ratio_compact_over_dense_attribution=med["compact_attribution"] / med["dense_attribution"],
    )


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--shapes", default="1024x2048,4096x2048", help="R x K, comma separated")
    ap.add_argument("--S", type=int, default=64, help="pushes per (rank, kernel) of the interval")
    ap.add_argument("--permille", type=int, default=990)
    ap.add_argument("--top", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from nvidia_resiliency_ext.straggler import batch, histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_compact_counts_attribution: no HIP device")
    dev = torch.device("cuda:0")
    runs = []
    for shape in a.shapes.split(","):
        R, K = (int(x) for x in shape.lower().split("x"))
        runs.append(one_shape(R, K, a, torch, batch, histograms, ops, synth, dev))
        torch.cuda.empty_cache()
    line = dict(tool="bench_compact_counts_attribution", device=torch.cuda.get_device_name(0),
                warmup=a.warmup, reps=a.reps, runs=runs)
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
