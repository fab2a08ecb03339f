#!/usr/bin/env python3
"""Cost of the individual tail score attribution of record streams
(segment_history_attribution.hip: the bucketed samples against the dense history, no [R, K, 240]
counts of the interval) against the dense chain it replaces, against the score pass over nearly
the same bytes, and against the bytes it moves.

Streams: synth.synth_records over a Zipf push order (synth.zipf_counts / zipf_order: 47,482
records per rank at K = 2,048), R ranks, bucketed once by ops.records_bucket (every bucket written
out).  The history is one such interval (the same buckets absorbed once).  In one process,
interleaved, timed with HIP events:
  attribution   ops.segment_history_attribution_ragged, top 8: the loss kernel and the select
                kernel together (they are not timed separately)
  score         ops.segment_history_scores_ragged, SCORE (DESIGN 3.16's SCORE leg), for scale
  dense_hist / dense_attribution   (--dense) ops.segment_histogram_ragged into the counts, then
                ops.histogram_tail_attribution(kind="individual"): the chain on the same buckets
                (R * K * 960 B of counts next to the history)
  reporter / reporter_attr   (--reporter) MatrixReporter.individual_tail_scores_records(absorb=
                "never") without and with attribute=8 on the records themselves: bucketing, the
                launches and the device-to-host copy, timed on the host clock around the call
Bytes of the new entry: 960 B of history per taken element, 4 B per retained sample and 12 B per
segment in the loss kernel, 8 B per (row, kernel) written and read back; the winners' re-read is
left out (top per row).  Prints one JSON line (and writes it to --out).  Needs a GPU: no fallback.
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
    ap.add_argument("--R", type=int, default=1024)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--permille", type=int, default=990)
    ap.add_argument("--top", type=int, default=8)
    ap.add_argument("--dense", action="store_true",
                    help="also time the dense chain (R * K * 960 B of counts next to the history)")
    ap.add_argument("--reporter", action="store_true",
                    help="also time the reporter call with and without attribute (a second history)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nvidia_resiliency_ext.straggler import batch, histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_individual_tail_records_attribution: no HIP device")
    dev = torch.device("cuda:0")
    R, K, cap, pm, top, B = a.R, a.K, a.cap, a.permille, a.top, histograms.BINS
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
    if not a.reporter:
        del recs
    assert int(seg_len.min()) >= 0
    max_len = int(seg_len.max())
    samples = int(seg_len.sum(dtype=torch.int64))
    nonempty = int((seg_len > 0).sum())

    # the history: one such interval
    hist = torch.zeros((R, K, B), dtype=torch.int32, device=dev)
    ops.segment_history_scores_ragged(out_ns, seg_off, seg_len, K, max_len, hist, permille=pm,
                                      aligned16=True, score=False)
    attr = ops.TailAttribution.empty(R, K, top, dev)
    sc = ops.HistoryTailScores.empty(R, dev)
    legs = {
        "attribution": lambda: ops.segment_history_attribution_ragged(
            out_ns, seg_off, seg_len, K, max_len, hist, permille=pm, top=top, aligned16=True, out=attr),
        "score": lambda: ops.segment_history_scores_ragged(
            out_ns, seg_off, seg_len, K, max_len, hist, permille=pm, aligned16=True, update=False, out=sc),
    }
    if a.dense:
        counts = torch.zeros((R * K, B), dtype=torch.int32, device=dev)
        dattr = ops.TailAttribution.empty(R, K, top, dev)
        legs["dense_hist"] = lambda: ops.segment_histogram_ragged(out_ns, seg_off, seg_len, max_len,
                                                                  aligned16=True, out=counts)
        legs["dense_attribution"] = lambda: ops.histogram_tail_attribution(
            counts.view(R, K, B), top=top, kind="individual", hist=hist, permille=pm, out=dattr)
        # what is timed is right: the two give the same bits
        for n in ("dense_hist", "dense_attribution", "attribution"):
            legs[n]()
        for n in ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share"):
            assert torch.equal(getattr(attr, n).view(torch.uint8), getattr(dattr, n).view(torch.uint8)), n
        x, y = attr.loss_all, dattr.loss_all
        assert torch.equal(x.isnan(), y.isnan()) and torch.equal(x[~x.isnan()], y[~y.isnan()])
    host_legs = {}
    if a.reporter:
        rep = batch.MatrixReporter(R, K, cap=cap)
        rep.individual_tail_scores_records(recs, rec_off, permille=pm, absorb="always")  # its history
        host_legs["reporter"] = lambda: rep.individual_tail_scores_records(
            recs, rec_off, permille=pm, absorb="never")
        host_legs["reporter_attr"] = lambda: rep.individual_tail_scores_records(
            recs, rec_off, permille=pm, absorb="never", attribute=top)
    times = {k: [] for k in list(legs) + list(host_legs)}
    for it in range(a.warmup + a.reps):
        for name, fn in legs.items():  # interleaved: every leg sees the same drift
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
        for name, fn in host_legs.items():  # the call ends with its device-to-host copy
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if it >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    taken = int((~attr.loss_all.isnan()).sum())

    res = {k: _summary(v) for k, v in times.items()}
    med = {k: res[k]["median_ms"] for k in times}
    nbytes = dict(attribution=960 * taken + 4 * samples + 12 * R * K + 2 * 8 * R * K,
                  score=960 * nonempty + 4 * samples + 12 * R * K)
    dense_bytes = 4 * samples + 12 * R * K + 960 * R * K + 1920 * R * K + 2 * 8 * R * K
    line = dict(
        tool="bench_individual_tail_records_attribution", device=torch.cuda.get_device_name(0),
        shape=dict(R=R, K=K, cap=cap, permille=pm, top=top, records=R * N, retained_samples=samples,
                   nonempty_elements=nonempty, taken_elements=taken, longest_bucket=max_len,
                   records_bytes=8 * R * N, history_bytes=R * K * B * 4,
                   dense_counts_bytes=R * K * B * 4),
        warmup=a.warmup, reps=a.reps, **res, bytes=nbytes, dense_chain_bytes=dense_bytes,
        loss_and_select_timed_separately=False,
        floor_ms={k: v / (COPY_TB_S * 1e12) * 1e3 for k, v in nbytes.items()},
        fraction_of_copy_rate={k: v / (COPY_TB_S * 1e12) * 1e3 / med[k] for k, v in nbytes.items()},
        ratio_attribution_over_score=med["attribution"] / med["score"],
    )
    if a.dense:
        line["dense_ms"] = med["dense_hist"] + med["dense_attribution"]
        line["ratio_attribution_over_dense"] = med["attribution"] / line["dense_ms"]
    if a.reporter:
        line["reporter_attribute_adds_ms"] = med["reporter_attr"] - med["reporter"]
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
