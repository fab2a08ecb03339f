#!/usr/bin/env python3
"""Cost of the individual tail score attribution of record streams against the compact history
(segment_history_compact_attribution.hip: 64 B per (rank, kernel)) next to the dense-history entry
(segment_history_attribution.hip: 960 B) on the same inputs and the compact SCORE leg, in the same
process.

Streams: synth.synth_records over a Zipf push order (synth.zipf_counts / zipf_order: 47,482
records per rank at K = 2,048), R ranks, bucketed once by ops.records_bucket (every bucket written
out).  Each history is one such interval (the same buckets absorbed once by the compact and by the
dense update); nothing may fold there, so the dense history is the expansion of the compact one.
Before anything is timed the new entry's outputs are compared with the dense entry's, byte for
byte.  Interleaved, timed with HIP events:
  compact_attribution   ops.segment_history_attribution_compact_ragged, top --top
  dense_attribution     ops.segment_history_attribution_ragged on the expanded history
  compact_score         ops.segment_history_scores_compact_ragged(update=False)
The dense leg runs only if its history fits in free device memory (--no-dense leaves it out, and
with it the comparison).  Bytes of an attribution: the history of every non-empty element (64 B /
960 B), 4 B per retained sample, 12 B per segment, loss_all written by the loss kernel and read by
the select kernel (16 B per element); the winners' second read is left out (top per row).  Prints
one JSON line (and writes it to --out).  Needs a GPU: no fallback.
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
    ap.add_argument("--no-dense", action="store_true", help="time the compact legs only")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nvidia_resiliency_ext.straggler import histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_compact_attribution: no HIP device")
    dev = torch.device("cuda:0")
    R, K, cap, pm, top = a.R, a.K, a.cap, a.permille, a.top
    B, CB = histograms.BINS, histograms.CHIST_BYTES
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
    seg = (out_ns, seg_off, seg_len, K, max_len)

    chist = torch.zeros((R, K, CB), dtype=torch.uint8, device=dev)
    folded = torch.zeros(R, dtype=torch.int64, device=dev)
    ops.segment_history_scores_compact_ragged(*seg, chist, permille=pm, aligned16=True, score=False,
                                              folded=folded)  # the history: one such interval
    folded_first = int(folded.sum())
    entries = chist.view(torch.int32)[:, :, -1]  # n of every element
    out_c = ops.TailAttribution.empty(R, K, top, dev)
    scores = ops.HistoryTailScores.empty(R, dev)
    legs = {
        "compact_attribution": lambda: ops.segment_history_attribution_compact_ragged(
            *seg, chist, permille=pm, top=top, aligned16=True, out=out_c),
        "compact_score": lambda: ops.segment_history_scores_compact_ragged(
            *seg, chist, permille=pm, aligned16=True, update=False, out=scores),
    }
    free = torch.cuda.mem_get_info()[0]
    with_dense = not a.no_dense and R * K * B * 4 + R * K * 8 + (1 << 30) < free
    if with_dense:
        if folded_first:
            raise SystemExit("bench_compact_attribution: the history interval folded; the dense "
                             "history would not be the expansion of the compact one")
        hist = torch.zeros((R, K, B), dtype=torch.int32, device=dev)
        ops.segment_history_scores_ragged(*seg, hist, permille=pm, aligned16=True, score=False)
        out_d = ops.TailAttribution.empty(R, K, top, dev)
        legs["dense_attribution"] = lambda: ops.segment_history_attribution_ragged(
            *seg, hist, permille=pm, top=top, aligned16=True, out=out_d)
        # what is timed is right: the two entries give the same bytes
        for f in FIELDS:
            getattr(out_c, f).view(torch.uint8).fill_(0x5A)
            getattr(out_d, f).view(torch.uint8).fill_(0xA5)
        legs["compact_attribution"]()
        legs["dense_attribution"]()
        for f in FIELDS:
            x, y = getattr(out_c, f), getattr(out_d, f)
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f
    taken = int((out_c.idx >= 0).sum()) if with_dense else None
    order = [n for n in ("compact_attribution", "dense_attribution", "compact_score") if n in legs]
    times = {k: [] for k in order}
    for it in range(a.warmup + a.reps):
        for name in order:  # interleaved: every leg sees the same drift
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            legs[name]()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))

    res = {k: _summary(v) for k, v in times.items()}
    med = {k: res[k]["median_ms"] for k in times}
    seg_bytes = 4 * samples + 12 * R * K
    nbytes = dict(compact_attribution=CB * nonempty + seg_bytes + 16 * R * K,
                  compact_score=CB * nonempty + seg_bytes)
    if with_dense:
        nbytes["dense_attribution"] = 4 * B * nonempty + seg_bytes + 16 * R * K
    line = dict(
        tool="bench_compact_attribution", device=torch.cuda.get_device_name(0),
        shape=dict(R=R, K=K, cap=cap, permille=pm, top=top, records=R * N, retained_samples=samples,
                   nonempty_elements=nonempty, longest_bucket=max_len,
                   compact_history_bytes=R * K * CB, dense_history_bytes=R * K * B * 4,
                   entries_mean=float(entries[seg_len.view(R, K) > 0].float().mean()),
                   entries_max=int(entries.max()), winners_taken=taken),
        folded_first_interval=folded_first, dense_leg=with_dense, outputs_equal_dense=with_dense,
        warmup=a.warmup, reps=a.reps, **res, bytes=nbytes,
        bytes_per_nonempty_element={k: v / nonempty for k, v in nbytes.items()},
        floor_ms={k: v / (COPY_TB_S * 1e12) * 1e3 for k, v in nbytes.items()},
        fraction_of_copy_rate={k: v / (COPY_TB_S * 1e12) * 1e3 / med[k] for k, v in nbytes.items()},
        ratio_attribution_over_compact_score=med["compact_attribution"] / med["compact_score"],
    )
    if with_dense:
        line["ratio_compact_over_dense_attribution"] = med["compact_attribution"] / med["dense_attribution"]
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
