#!/usr/bin/env python3
"""Cost of the score rank attribution (per kernel, the ranks behind its score loss:
ops.score_rank_attribution) against what a user had to write before it existed, against the
column-wise select alone, and against the bytes it moves.

Per shape R x K: f32 statistics num / med / avg [R, K] from MatrixReporter.report over
synth.synth_matrix, built in blocks of rows with a fresh seed per block (two reports per block, so
that the individual history differs from the statistics); the relative reference is
ops.kernel_ref over all rows.  Per kind and top, in one process, interleaved, timed with HIP
events:
  fused     ops.score_rank_attribution                       reads 12 R K bytes (individual: 16)
  unfused   the loss matrix by torch expressions (f64 [R, K], NaN where not taken), then
            ops.rank_attribution on it                       what the parent commit offers
  select    ops.rank_attribution alone on that matrix, precomputed
The floor is 12 R K bytes (f32, relative) at the float4 copy rate of DESIGN 3 (6.3 TB/s).  What
each leg wrote is checked on three columns against the host twin.  Prints one JSON line per shape
(and appends it to --out).  Needs a GPU: no fallback.
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nvidia_resiliency_ext.straggler import batch, histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_score_rank_attribution: no HIP device")
    dev = torch.device("cuda:0")
    K, S = a.K, a.s_push
    nan = float("nan")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for R in a.R:
        num = torch.empty((R, K), dtype=torch.int32, device=dev)
        med = torch.empty((R, K), dtype=torch.float32, device=dev)
        avg = torch.empty((R, K), dtype=torch.float32, device=dev)
        hist = torch.empty((R, K), dtype=torch.float32, device=dev)
        for r0 in range(0, R, a.block):
            n = min(a.block, R - r0)
            rep = batch.MatrixReporter(n, K, cap=S, device=dev)
            for rnd in (1, 0):  # the history from another interval, the statistics from this one
                rep.report(synth.synth_matrix(n, K, S, seed=synth.SEED + r0 + rnd * 7919, device=dev), S)
            st = rep.stats.view(n, K)
            num[r0:r0 + n], med[r0:r0 + n], avg[r0:r0 + n] = st.num, st.med, st.avg
            hist[r0:r0 + n] = rep.hist
        del rep, st
        ref = ops.kernel_ref(num, med)
        bases = dict(relative=dict(ref=ref), individual=dict(hist=hist))

        def loss_matrix(kind):
            """loss_all by torch expressions: what a user of the parent commit writes."""
            m = med.double()
            w = num.double() * avg.double()
            base = ref.double()[None, :] if kind == "relative" else hist.double()
            s = base / m
            loss = w * (1.0 - s)
            take = (num > 0) & (m != 0) & ~torch.isnan(loss)
            if kind == "relative":
                take &= (ref >= 0)[None, :]
            return torch.where(take, loss, torch.full_like(loss, nan))

        legs, outs = {}, {}
        for kind, base in bases.items():
            pre = loss_matrix(kind)
            for top in a.tops:
                work = torch.empty(max(ops.rank_attribution_plan(R, K, top)[2], 8), dtype=torch.uint8,
                                   device=dev)
                fo = outs["fused", kind, top] = ops.ScoreRankAttribution.empty(K, top, dev)
                uo = outs["unfused", kind, top] = ops.RankAttribution.empty(K, top, dev)
                so = outs["select", kind, top] = ops.RankAttribution.empty(K, top, dev)
                legs[f"fused_{kind}_top{top}"] = lambda kind=kind, top=top, fo=fo, work=work, base=base: \
                    ops.score_rank_attribution(num, med, avg, top=top, kind=kind, out=fo, work=work, **base)
                legs[f"unfused_{kind}_top{top}"] = lambda kind=kind, top=top, uo=uo, work=work: \
                    ops.rank_attribution(loss_matrix(kind), top, out=uo, work=work)
                legs[f"select_{kind}_top{top}"] = lambda pre=pre, top=top, so=so, work=work: \
                    ops.rank_attribution(pre, top, out=so, work=work)
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
        # what was timed is right: on three columns it equals the host twin
        cols = sorted({0, K // 2, K - 1})
        h = {k: v[:, cols].cpu().numpy() for k, v in dict(num=num, med=med, avg=avg, hist=hist).items()}
        href = ref[cols].cpu().numpy()
        for (leg, kind, top), out in outs.items():
            kw = dict(ref=href) if kind == "relative" else dict(hist=h["hist"])
            want = histograms.score_rank_attribution(h["num"], h["med"], h["avg"], top, kind, **kw)
            tag = (leg, kind, top)
            assert np.array_equal(out.idx.cpu().numpy()[cols], want.idx), tag
            assert np.array_equal(out.loss.cpu().numpy()[cols].view(np.uint64), want.loss.view(np.uint64)), tag
            assert np.array_equal(out.taken.cpu().numpy()[cols], want.taken), tag
            assert np.array_equal(out.positive.cpu().numpy()[cols], want.positive), tag
            if leg == "fused":
                assert np.array_equal(out.score.cpu().numpy()[cols].view(np.uint64),
                                      want.score.view(np.uint64)), tag

        res = {k: _summary(v) for k, v in times.items()}
        m = {k: res[k]["median_ms"] for k in times}
        floor = R * K * 12 / (COPY_TB_S * 1e12) * 1e3
        ratios = {}
        for kind in bases:
            for top in a.tops:
                f = m[f"fused_{kind}_top{top}"]
                ratios[f"{kind}_top{top}"] = dict(
                    fused_over_unfused=f / m[f"unfused_{kind}_top{top}"],
                    fused_over_select=f / m[f"select_{kind}_top{top}"],
                    fraction_of_copy_rate=floor * (1 if kind == "relative" else 16 / 12) / f)
        line = dict(tool="bench_score_rank_attribution", device=torch.cuda.get_device_name(0),
                    shape=dict(R=R, K=K, s_push=S, tops=a.tops,
                               plan={top: ops.rank_attribution_plan(R, K, top) for top in a.tops}),
                    warmup=a.warmup, reps=a.reps, **res, copy_floor_ms=floor, ratios=ratios)
        txt = json.dumps(line)
        print(txt, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(txt + "\n")
        del num, med, avg, hist, legs, outs, bases


if __name__ == "__main__":
    main()
