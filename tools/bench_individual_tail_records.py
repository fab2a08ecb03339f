#!/usr/bin/env python3
"""Cost of the individual tail scores of record streams (segment_history.hip: the bucketed samples
against the dense history, no [R, K, 240] counts of the interval) against the dense chain they
replace and against the bytes they move.

Streams: synth.synth_records over a Zipf push order (synth.zipf_counts / zipf_order: 47,482
records per rank at K = 2,048), R ranks, bucketed once by ops.records_bucket (every bucket written
out).  The history is one such interval (the same buckets absorbed once); the update legs keep
absorbing, which changes no byte count.  In one process, interleaved, timed with HIP events:
  score        ops.segment_history_scores_ragged, SCORE
  update       the same, UPDATE
  fused        the same, SCORE | UPDATE
  fused_calls  the same with tail_calls
  row_pass     ops.segment_tail_scores_ragged (DESIGN 3.14's row pass) on the same buckets, for scale
  dense_hist / dense_history   (--dense) ops.segment_histogram_ragged into the counts, then
               ops.histogram_history_scores SCORE | UPDATE on a history of its own: the chain on
               the same buckets (R * K * 960 B of counts next to the history)
Bytes of the new entry: 960 B of history per non-empty element, 4 B per retained sample, 12 B per
segment, 16 B per changed vector written (counted on the device from the buckets).  Prints one
JSON line (and writes it to --out).  Needs a GPU: no fallback.
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
    ap.add_argument("--dense", action="store_true",
                    help="also time the dense chain (R * K * 960 B of counts and a second history)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nvidia_resiliency_ext.straggler import histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_individual_tail_records: no HIP device")
    dev = torch.device("cuda:0")
    R, K, cap, pm, B = a.R, a.K, a.cap, a.permille, histograms.BINS
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
    assert int(seg_len.min()) >= 0
    max_len = int(seg_len.max())
    samples = int(seg_len.sum(dtype=torch.int64))
    nonempty = int((seg_len > 0).sum())

    def seg(hist, **kw):
        return ops.segment_history_scores_ragged(out_ns, seg_off, seg_len, K, max_len, hist,
                                                 permille=pm, aligned16=True, **kw)

    # the history: one such interval
    hist = torch.zeros((R, K, B), dtype=torch.int32, device=dev)
    seg(hist, score=False)
    changed = int((hist.view(R * K, B // 4, 4) != 0).any(2).sum())  # 16-byte vectors an update writes
    outs = {k: ops.HistoryTailScores.empty(R, dev) for k in ("score", "fused", "fused_calls", "dense")}
    calls = torch.empty((R, K), dtype=torch.int32, device=dev)
    legs = {
        "score": lambda: seg(hist, update=False, out=outs["score"]),
        "update": lambda: seg(hist, score=False),
        "fused": lambda: seg(hist, out=outs["fused"]),
        "fused_calls": lambda: seg(hist, out=outs["fused_calls"], tail_calls=calls),
    }
    if a.dense:
        counts = torch.zeros((R * K, B), dtype=torch.int32, device=dev)
        dhist = hist.clone()
        legs["dense_hist"] = lambda: ops.segment_histogram_ragged(out_ns, seg_off, seg_len, max_len,
                                                                  aligned16=True, out=counts)
        legs["dense_history"] = lambda: ops.histogram_history_scores(counts.view(R, K, B), dhist,
                                                                     permille=pm, out=outs["dense"])
        # what is timed is right: from the same history the two give the same bits
        legs["dense_hist"]()
        legs["dense_history"]()
        legs["fused"]()
        for n in ("score", "tail_ns", "total_ns", "base_tail_ns", "base_total_ns", "strag"):
            x, y = getattr(outs["fused"], n), getattr(outs["dense"], n)
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), n
        assert torch.equal(hist, dhist)
    # the row pass of DESIGN 3.14 on the same buckets, for scale
    fleet = ops.segment_fleet_histogram_ragged(out_ns, seg_off, seg_len, K, max_len, aligned16=True)
    thr, sums = ops.histogram_tail_threshold(fleet, pm)
    row = ops.TailScores(torch.empty(R, dtype=torch.float64, device=dev),
                         torch.empty(R, dtype=torch.int64, device=dev),
                         torch.empty(R, dtype=torch.int64, device=dev),
                         torch.empty(R, dtype=torch.uint8, device=dev))
    legs["row_pass"] = lambda: ops.segment_tail_scores_ragged(out_ns, seg_off, seg_len, K, max_len, thr,
                                                              sums, aligned16=True, out=row)
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

    res = {k: _summary(v) for k, v in times.items()}
    med = {k: res[k]["median_ms"] for k in times}
    read = 960 * nonempty + 4 * samples + 12 * R * K
    write = 16 * changed
    nbytes = dict(score=read, update=4 * samples + 12 * R * K + 2 * write, fused=read + write,
                  fused_calls=read + write + 4 * R * K)
    dense_bytes = 4 * samples + 12 * R * K + 960 * R * K + (1920 + 960) * R * K
    line = dict(
        tool="bench_individual_tail_records", device=torch.cuda.get_device_name(0),
        shape=dict(R=R, K=K, cap=cap, permille=pm, records=R * N, retained_samples=samples,
                   nonempty_elements=nonempty, changed_vectors=changed, longest_bucket=max_len,
                   records_bytes=8 * R * N, history_bytes=R * K * B * 4,
                   dense_counts_bytes=R * K * B * 4),
        warmup=a.warmup, reps=a.reps, **res, bytes=nbytes, dense_chain_bytes=dense_bytes,
        floor_ms={k: v / (COPY_TB_S * 1e12) * 1e3 for k, v in nbytes.items()},
        fraction_of_copy_rate={k: v / (COPY_TB_S * 1e12) * 1e3 / med[k] for k, v in nbytes.items()},
    )
    if a.dense:
        line["dense_ms"] = med["dense_hist"] + med["dense_history"]
        line["ratio_fused_over_dense"] = med["fused"] / line["dense_ms"]
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
