#!/usr/bin/env python3
"""Cost of the individual tail scores of record streams against the compact history
(segment_history_compact.hip: 64 B per (rank, kernel)) next to the dense-history entry
(segment_history.hip: 960 B) on the same inputs, in the same process.

Streams: synth.synth_records over a Zipf push order (synth.zipf_counts / zipf_order: 47,482
records per rank at K = 2,048), R ranks, bucketed once by ops.records_bucket (every bucket written
out).  Each history is one such interval (the same buckets absorbed once); the update legs keep
absorbing, which changes no byte count.  Interleaved, timed with HIP events:
  compact_score / compact_update / compact_fused   ops.segment_history_scores_compact_ragged
  dense_score / dense_update / dense_fused         ops.segment_history_scores_ragged
The dense legs run only if both histories fit in free device memory (--no-dense leaves them out).
Bytes of the compact entry: 64 B of history per non-empty element read, 64 B written per updated
element, 4 B per retained sample, 12 B per segment; of the dense entry as
tools/bench_individual_tail_records.py counts them.  Prints one JSON line (and writes it to
--out).  Needs a GPU: no fallback.
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
    ap.add_argument("--R", type=int, default=1024)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--permille", type=int, default=990)
    ap.add_argument("--no-dense", action="store_true", help="time the compact legs only")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nvidia_resiliency_ext.straggler import histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_compact_history: no HIP device")
    dev = torch.device("cuda:0")
    R, K, cap, pm, B, CB = a.R, a.K, a.cap, a.permille, histograms.BINS, histograms.CHIST_BYTES
    calls_per = synth.zipf_counts(K)
    slot, occ = synth.zipf_order(calls_per)
    N = slot.size
    t32 = lambda x: torch.from_numpy(x.view(np.int32)).to(dev)  # noqa: E731
    recs = synth.synth_records(R, t32(slot), t32(occ), K, int(calls_per.max()))
    rec_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * N
    need = ops.records_bucket_capacity(R * N, R, K)
    bucket = (torch.empty(R * K, dtype=torch.int64, device=dev),
              torch.empty(R * K, dtype=torch.int32, device=dev),
              torch.empty(max(need, 1), dtype=torch.int32, device=dev),
              torch.empty(R * K, dtype=torch.int32, device=dev))
    seg_off, seg_len, out_ns, _ = ops.records_bucket(recs, rec_off, K, cap, out=bucket)
    del recs
    torch.cuda.empty_cache()
    assert int(seg_len.min()) >= 0
    max_len = int(seg_len.max())
    samples = int(seg_len.sum(dtype=torch.int64))
    nonempty = int((seg_len > 0).sum())

    def compact(chist, **kw):
        return ops.segment_history_scores_compact_ragged(out_ns, seg_off, seg_len, K, max_len, chist,
                                                         permille=pm, aligned16=True, **kw)

    def dense(hist, **kw):
        return ops.segment_history_scores_ragged(out_ns, seg_off, seg_len, K, max_len, hist,
                                                 permille=pm, aligned16=True, **kw)

    chist = torch.zeros((R, K, CB), dtype=torch.uint8, device=dev)
    folded = torch.zeros(R, dtype=torch.int64, device=dev)
    compact(chist, score=False, folded=folded)  # the history: one such interval
    folded_first = int(folded.sum())
    entries = chist.view(torch.int32)[:, :, -1]  # n of every element
    outs = {k: ops.HistoryTailScores.empty(R, dev)
            for k in ("compact_score", "compact_fused", "dense_score", "dense_fused")}
    legs = {
        "compact_score": lambda: compact(chist, update=False, out=outs["compact_score"]),
        "compact_update": lambda: compact(chist, score=False, folded=folded),
        "compact_fused": lambda: compact(chist, out=outs["compact_fused"], folded=folded),
    }
    free = torch.cuda.mem_get_info()[0]
    with_dense = not a.no_dense and R * K * B * 4 + (1 << 30) < free
    changed = None
    if with_dense:
        hist = torch.zeros((R, K, B), dtype=torch.int32, device=dev)
        dense(hist, score=False)
        changed = int((hist.view(R * K, B // 4, 4) != 0).any(2).sum())  # 16-byte vectors an update writes
        legs["dense_score"] = lambda: dense(hist, update=False, out=outs["dense_score"])
        legs["dense_update"] = lambda: dense(hist, score=False)
        legs["dense_fused"] = lambda: dense(hist, out=outs["dense_fused"])
        # what is timed is right: while nothing folds the two give the same bits
        legs["compact_score"]()
        legs["dense_score"]()
        if folded_first == 0:
            for n in ("score", "tail_ns", "total_ns", "base_tail_ns", "base_total_ns", "strag"):
                x, y = getattr(outs["compact_score"], n), getattr(outs["dense_score"], n)
                assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), n
    times = {k: [] for k in legs}
    folded_total = 0
    for it in range(a.warmup + a.reps):
        for name, fn in legs.items():  # interleaved: every leg sees the same drift
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
        folded_total = max(folded_total, int(folded.sum()))

    res = {k: _summary(v) for k, v in times.items()}
    med = {k: res[k]["median_ms"] for k in times}
    seg_bytes = 4 * samples + 12 * R * K
    nbytes = dict(compact_score=CB * nonempty + seg_bytes, compact_update=2 * CB * nonempty + seg_bytes,
                  compact_fused=2 * CB * nonempty + seg_bytes)
    if with_dense:
        nbytes.update(dense_score=960 * nonempty + seg_bytes, dense_update=seg_bytes + 2 * 16 * changed,
                      dense_fused=960 * nonempty + seg_bytes + 16 * changed)
    line = dict(
        tool="bench_compact_history", device=torch.cuda.get_device_name(0),
        shape=dict(R=R, K=K, cap=cap, permille=pm, records=R * N, retained_samples=samples,
                   nonempty_elements=nonempty, longest_bucket=max_len, records_bytes=8 * R * N,
                   compact_history_bytes=R * K * CB, dense_history_bytes=R * K * B * 4,
                   dense_changed_vectors=changed,
                   entries_mean=float(entries[seg_len.view(R, K) > 0].float().mean()),
                   entries_max=int(entries.max())),
        folded_first_interval=folded_first, folded_per_call_max=folded_total,
        dense_legs=with_dense, warmup=a.warmup, reps=a.reps, **res, bytes=nbytes,
        bytes_per_nonempty_element={k: v / nonempty for k, v in nbytes.items()},
        floor_ms={k: v / (COPY_TB_S * 1e12) * 1e3 for k, v in nbytes.items()},
        fraction_of_copy_rate={k: v / (COPY_TB_S * 1e12) * 1e3 / med[k] for k, v in nbytes.items()},
    )
    if with_dense:
        line["ratio_compact_over_dense"] = {m: med["compact_" + m] / med["dense_" + m]
                                            for m in ("score", "update", "fused")}
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
