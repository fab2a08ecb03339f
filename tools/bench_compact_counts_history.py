#!/usr/bin/env python3
"""Cost of the individual tail scores of [R, K, 240] counts against the compact history
(histogram_history_compact.hip: 64 B per (rank, kernel)) next to the dense-history entry
(histogram_history.hip: 960 B) on the same inputs, in the same process, and of the two
conversions between the histories.

Counts: MatrixReporter.histograms over synth.synth_matrix (R ranks, K kernels, S pushes).  Each
history is one such interval (the same counts absorbed once); the update legs keep absorbing, which
changes no byte count.  Interleaved, timed with HIP events:
  compact_score / compact_update / compact_fused   ops.histogram_history_scores_compact
  dense_score / dense_update / dense_fused         ops.histogram_history_scores
  from_dense / to_dense                            ops.compact_history_from_dense / _to_dense
Bytes per element: the counts (960 B) are read by every leg; the compact legs add 64 B of history
read (score) or read and written (update, fused), the dense legs 960 B likewise; a conversion moves
960 + 64 B.  The tool asserts that nothing folds and that every output of the compact entry equals
the dense entry's bit for bit.  Prints one JSON line (and writes it to --out).  Needs a GPU: no
fallback.
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
    ap.add_argument("--S", type=int, default=64, help="pushes per (rank, kernel) of the interval")
    ap.add_argument("--permille", type=int, default=990)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from nvidia_resiliency_ext.straggler import batch, histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_compact_counts_history: no HIP device")
    dev = torch.device("cuda:0")
    R, K, S, pm, B, CB = a.R, a.K, a.S, a.permille, histograms.BINS, histograms.CHIST_BYTES
    rep = batch.MatrixReporter(R, K, cap=S, device=dev)
    counts = rep.histograms(synth.synth_matrix(R, K, S, device=dev), S).clone()
    del rep
    torch.cuda.empty_cache()
    used = (counts != 0).sum(2)

    def compact(chist, **kw):
        return ops.histogram_history_scores_compact(counts, chist, permille=pm, **kw)

    def dense(hist, **kw):
        return ops.histogram_history_scores(counts, hist, permille=pm, **kw)

    chist = torch.zeros((R, K, CB), dtype=torch.uint8, device=dev)
    hist = torch.zeros((R, K, B), dtype=torch.int32, device=dev)
    folded = torch.zeros(R, dtype=torch.int64, device=dev)
    compact(chist, score=False, folded=folded)  # the histories: one such interval
    dense(hist, score=False)
    assert int(folded.sum()) == 0, "the history folded"
    assert torch.equal(ops.compact_history_to_dense(chist), hist)
    names = ("compact_score", "compact_fused", "dense_score", "dense_fused")
    outs = {k: ops.HistoryTailScores.empty(R, dev) for k in names}
    calls = {k: torch.empty((R, K), dtype=torch.int32, device=dev) for k in names}
    chist2 = torch.empty_like(chist)
    hist2 = torch.empty_like(hist)
    cfold = torch.zeros(R, dtype=torch.int64, device=dev)
    legs = {
        "compact_score": lambda: compact(chist, update=False, out=outs["compact_score"],
                                         tail_calls=calls["compact_score"]),
        "dense_score": lambda: dense(hist, update=False, out=outs["dense_score"],
                                     tail_calls=calls["dense_score"]),
        "compact_update": lambda: compact(chist, score=False, folded=folded),
        "dense_update": lambda: dense(hist, score=False),
        "compact_fused": lambda: compact(chist, out=outs["compact_fused"], folded=folded,
                                         tail_calls=calls["compact_fused"]),
        "dense_fused": lambda: dense(hist, out=outs["dense_fused"], tail_calls=calls["dense_fused"]),
        "from_dense": lambda: ops.compact_history_from_dense(hist, out=chist2, folded=cfold),
        "to_dense": lambda: ops.compact_history_to_dense(chist, out=hist2),
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
        # what is timed is right: nothing folds, and the two entries give the same bits
        assert int(folded.sum()) == 0 and int(cfold.sum()) == 0
        for m in ("score", "fused"):
            x, y = outs["compact_" + m], outs["dense_" + m]
            for n in ("score", "tail_ns", "total_ns", "base_tail_ns", "base_total_ns", "strag"):
                assert torch.equal(getattr(x, n).view(torch.uint8), getattr(y, n).view(torch.uint8)), (m, n)
            assert torch.equal(calls["compact_" + m], calls["dense_" + m]), m
    assert torch.equal(chist2, chist) and torch.equal(hist2, hist)
    assert torch.equal(ops.compact_history_to_dense(chist), hist)

    res = {k: _summary(v) for k, v in times.items()}
    med = {k: res[k]["median_ms"] for k in times}
    E = R * K
    per = dict(compact_score=960 + CB + 4, compact_update=960 + 2 * CB, compact_fused=960 + 2 * CB + 4,
               dense_score=2 * 960 + 4, dense_update=3 * 960, dense_fused=3 * 960 + 4,
               from_dense=960 + CB, to_dense=960 + CB)
    nbytes = {k: v * E for k, v in per.items()}
    line = dict(
        tool="bench_compact_counts_history", device=torch.cuda.get_device_name(0),
        shape=dict(R=R, K=K, S=S, permille=pm, elements=E, counts_bytes=E * B * 4,
                   compact_history_bytes=E * CB, dense_history_bytes=E * B * 4,
                   used_buckets_mean=float(used.float().mean()), used_buckets_max=int(used.max()),
                   entries_max=int(chist.view(torch.int32)[:, :, -1].max())),
        folded=0, warmup=a.warmup, reps=a.reps, **res, bytes_per_element=per, bytes=nbytes,
        floor_ms={k: v / (COPY_TB_S * 1e12) * 1e3 for k, v in nbytes.items()},
        fraction_of_copy_rate={k: v / (COPY_TB_S * 1e12) * 1e3 / med[k] for k, v in nbytes.items()},
        ns_per_element={k: med[k] * 1e6 / E for k in med},
        ratio_compact_over_dense={m: med["compact_" + m] / med["dense_" + m]
                                  for m in ("score", "update", "fused")},
    )
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
