#!/usr/bin/env python3
"""Cost of score attribution against the scores kernel that reads the same bytes.

Random f32 statistics [R][K] on the device (no statistics kernel runs), the relative reference by
ops.kernel_ref.  Per shape (4,096 x 2,048 and 16,384 x 2,048), in one process, interleaved, timed
with HIP events:
  (a) ops.scores, relative only, in-kernel finalize      the yardstick (unchanged code)
  (b) ops.score_attribution(kind="relative", top=8)
  (c) ops.score_attribution(kind="relative", top=16)
Both read NUM / MED / AVG once: 12 B per element; attribution writes (12 + 8) * top B per row.
Prints one JSON line (and writes it to --out).  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nvidia-resiliency-ext-x_amd"))

SHAPES = ((4096, 2048), (16384, 2048))


def _summary(ms):
    s = sorted(ms)
    n = len(s)
    return dict(median_ms=statistics.median(s), min_ms=s[0], max_ms=s[-1],
                p10_ms=s[(n - 1) // 10], p90_ms=s[(9 * (n - 1)) // 10], n=n)


def bench_shape(R, K, warmup, reps):
    import torch

    from nvidia_resiliency_ext.straggler import ops

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(R + K)
    num = torch.randint(1, 50, (R, K), dtype=torch.int32, device=dev, generator=g)
    med = torch.empty((R, K), dtype=torch.float32, device=dev).uniform_(10.0, 1000.0, generator=g)
    avg = med * torch.empty_like(med).uniform_(0.9, 1.4, generator=g)
    ref = ops.kernel_ref(num, med)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    fz = dict(gpu_rel=torch.empty(R, dtype=torch.float64, device=dev),
              strag_rel=torch.empty(R, dtype=torch.uint8, device=dev), thr_rel=0.75)
    outs = {top: ops.ScoreAttribution(torch.empty((R, top), dtype=torch.int32, device=dev),
                                      torch.empty((R, top), dtype=torch.float64, device=dev),
                                      torch.empty((R, top), dtype=torch.float64, device=dev),
                                      torch.empty(R, dtype=torch.float64, device=dev))
            for top in (8, 16)}
    legs = {
        "scores_rel": lambda: ops.scores(num, med, avg, ref=ref, err=err, finalize=fz),
        "attribution_top8": lambda: ops.score_attribution(num, med, avg, top=8, kind="relative",
                                                          ref=ref, err=err, out=outs[8]),
        "attribution_top16": lambda: ops.score_attribution(num, med, avg, top=16, kind="relative",
                                                           ref=ref, err=err, out=outs[16]),
    }
    times = {k: [] for k in legs}
    for it in range(warmup + reps):
        for name, fn in legs.items():  # interleaved: every leg sees the same drift
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1))
    # the legs agree: the largest loss of every row, and the first 8 of 16 are the 8
    loss = (num.double() * avg.double()) * (1.0 - ref.double()[None, :] / med.double())
    assert torch.equal(outs[16].loss[:, 0], loss.max(dim=1).values)
    assert torch.equal(outs[16].idx[:, :8], outs[8].idx) and int(err.item()) == 0
    assert torch.allclose(1.0 - loss.sum(dim=1) / outs[8].wsum, fz["gpu_rel"], rtol=0, atol=1e-12)
    res = {k: _summary(v) for k, v in times.items()}
    base = res["scores_rel"]["median_ms"]
    read = 12 * R * K
    return dict(R=R, K=K, bytes_read=read, **res,
                ratio_top8_over_scores=res["attribution_top8"]["median_ms"] / base,
                ratio_top16_over_scores=res["attribution_top16"]["median_ms"] / base,
                bytes_written={"attribution_top8": 20 * 8 * R + 8 * R,
                               "attribution_top16": 20 * 16 * R + 8 * R},
                read_gb_per_s={k: read / (v["median_ms"] * 1e-3) / 1e9 for k, v in res.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attribution",
                                                  "bench_attribution.json"))
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_attribution: no HIP device")
    line = dict(tool="bench_attribution", device=torch.cuda.get_device_name(0), warmup=a.warmup,
                reps=a.reps, shapes=[bench_shape(R, K, a.warmup, a.reps) for R, K in SHAPES])
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
