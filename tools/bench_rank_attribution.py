#!/usr/bin/env python3
"""Cost of the rank attribution (per kernel, the ranks behind its tail loss: ops.rank_attribution)
against what a user would write today, against the bytes it moves, and against the attribution
entry that produced the matrix.

Per shape R x K and per top, two inputs:
  real    the loss_all of the relative tail attribution (what MatrixReporter.tail_scores(attribute=8)
          runs: ops.histogram_tail_base + histogram_tail_attribution) over the histograms of
          synth.synth_matrix, built in blocks of rows with a fresh seed per block (NaN where a
          kernel is not taken; the share is reported as real_nan_share)
  dense   a dense random f64 matrix (normal), no NaN
In one process, interleaved, timed with HIP events:
  ranks   ops.rank_attribution(loss, top)                 reads 8 R K bytes once
  topk    torch.topk(loss, top, dim=0)                    no NaN rule, no tie rule: timing only
  attr    the attribution entry that produced `real`      960 + 16 bytes per (row, kernel)
The floor is 8 R K bytes at the float4 copy rate of DESIGN 3 (6.3 TB/s).  Prints one JSON line per
shape (and appends it to --out).  Needs a GPU: no fallback.
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
    ap.add_argument("--R", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--tops", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--s-push", type=int, default=256)
    ap.add_argument("--block", type=int, default=256, help="rows per synth block")
    ap.add_argument("--permille", type=int, default=950)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nvidia_resiliency_ext.straggler import batch, histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_rank_attribution: no HIP device")
    dev = torch.device("cuda:0")
    K, S, B, pm = a.K, a.s_push, histograms.BINS, a.permille
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for R in a.R:
        counts = torch.empty((R, K, B), dtype=torch.int32, device=dev)
        for r0 in range(0, R, a.block):
            n = min(a.block, R - r0)
            rep = batch.MatrixReporter(n, K, cap=S, device=dev)
            rep.histograms(synth.synth_matrix(n, K, S, seed=synth.SEED + r0, device=dev), S,
                           out=counts[r0:r0 + n])
        del rep
        fleet = ops.histogram_sum(counts)
        thr, _ = ops.histogram_tail_threshold(fleet, pm)
        base = torch.empty((K, 2), dtype=torch.int64, device=dev)
        att = ops.TailAttribution.empty(R, K, 8, dev)

        def attr():
            ops.histogram_tail_base(fleet, thr, out=base)
            ops.histogram_tail_attribution(counts, top=8, kind="relative", thr=thr, base=base, out=att)

        attr()
        inputs = dict(real=att.loss_all,
                      dense=torch.randn((R, K), dtype=torch.float64, device=dev,
                                        generator=torch.Generator(device=dev).manual_seed(R)))
        legs, outs = {"attr": attr}, {}
        for top in a.tops:
            work = torch.empty(max(ops.rank_attribution_plan(R, K, top)[2], 8), dtype=torch.uint8,
                               device=dev)
            for name, x in inputs.items():
                out = outs[name, top] = ops.RankAttribution.empty(K, top, dev)
                legs[f"ranks_{name}_top{top}"] = \
                    lambda x=x, top=top, out=out, work=work: ops.rank_attribution(x, top, out=out, work=work)
                legs[f"topk_{name}_top{top}"] = lambda x=x, top=top: torch.topk(x, top, dim=0)
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
        # what was timed is right: on a few columns it equals the host twin
        cols = sorted({0, K // 2, K - 1})
        for (name, top), out in outs.items():
            want = histograms.rank_attribution(inputs[name][:, cols].cpu().numpy(), top)
            assert np.array_equal(out.idx.cpu().numpy()[cols], want.idx), (name, top)
            assert np.array_equal(out.loss.cpu().numpy()[cols].view(np.uint64), want.loss.view(np.uint64))
            assert np.array_equal(out.taken.cpu().numpy()[cols], want.taken)
            assert np.array_equal(out.positive.cpu().numpy()[cols], want.positive)

        res = {k: _summary(v) for k, v in times.items()}
        med = {k: res[k]["median_ms"] for k in times}
        floor = R * K * 8 / (COPY_TB_S * 1e12) * 1e3
        ratios = {}
        for top in a.tops:
            for name in inputs:
                m = med[f"ranks_{name}_top{top}"]
                ratios[f"{name}_top{top}"] = dict(
                    over_topk=m / med[f"topk_{name}_top{top}"], fraction_of_copy_rate=floor / m,
                    over_attr=m / med["attr"])
        nan_share = float(torch.isnan(inputs["real"]).double().mean())
        line = dict(tool="bench_rank_attribution", device=torch.cuda.get_device_name(0),
                    shape=dict(R=R, K=K, s_push=S, permille=pm, tops=a.tops, real_nan_share=nan_share,
                               plan={top: ops.rank_attribution_plan(R, K, top) for top in a.tops}),
                    warmup=a.warmup, reps=a.reps, **res, copy_floor_ms=floor, ratios=ratios)
        txt = json.dumps(line)
        print(txt, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(txt + "\n")
        del counts, att, inputs, legs, outs, fleet


if __name__ == "__main__":
    main()
