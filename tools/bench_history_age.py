#!/usr/bin/env python3
"""Cost of aging the tail histories (history_age.hip) next to two yardsticks measured in the same
process: a device copy of the same tensor, which reads and writes the same bytes, and the compact
SCORE | UPDATE pass (segment_history_compact.hip) that a ``half_life`` call runs after the aging.

Streams as tools/bench_compact_history.py: synth.synth_records over a Zipf push order (47,482
records per rank at K = 2,048), R ranks, bucketed once by ops.records_bucket.  Each history is one
such interval and is restored from a copy before every timed call (the restore is not timed), so
every repetition ages the same bytes.  Interleaved, timed with HIP events:
  compact_age / compact_age_counts   ops.compact_history_age without / with the row outputs
  compact_age_full12                 the same pass on a synthetic history whose every element
                                     holds 12 entries, every second one evicted by the shift
  compact_copy                       Tensor.copy_ of the compact history into a second tensor
  compact_fused                      ops.segment_history_scores_compact_ragged, SCORE | UPDATE
  dense_age / dense_copy             ops.histogram_history_age / Tensor.copy_ of the dense history
The dense legs run only if three dense histories fit in free device memory (--no-dense leaves
them out).  Bytes of the compact pass: 64 B read per element, 64 B written per non-empty element;
of the dense pass: 960 B read per element, 16 B written per vector that held a count.  Prints one
JSON line (and writes it to --out).  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nvidia-resiliency-ext-x_amd"))


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
    ap.add_argument("--shift", type=int, default=1)
    ap.add_argument("--no-dense", action="store_true", help="time the compact legs only")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from nvidia_resiliency_ext.straggler import histograms, ops, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench_history_age: no HIP device")
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
    max_len = int(seg_len.max())

    chist0 = torch.zeros((R, K, CB), dtype=torch.uint8, device=dev)
    folded = torch.zeros(R, dtype=torch.int64, device=dev)
    ops.segment_history_scores_compact_ragged(out_ns, seg_off, seg_len, K, max_len, chist0,
                                              permille=pm, aligned16=True, score=False, folded=folded)
    n0 = chist0.view(torch.int32)[:, :, -1]
    nonempty = int((n0 > 0).sum())
    chist, ccopy = chist0.clone(), torch.empty_like(chist0)
    evicted, full = torch.zeros(R, dtype=torch.int64, device=dev), torch.zeros(R, dtype=torch.int64, device=dev)
    ops.compact_history_age(chist, a.shift, evicted=evicted, full=full)
    evicted_total, stores = int(evicted.sum()), nonempty
    # every element full, every second entry evicted: counts 1, 2^20, 1, ...; buckets 0, 16, ..., 176
    one = np.zeros(CB, np.uint8)
    one[:48] = np.asarray([1 if i % 2 == 0 else 1 << 20 for i in range(12)], "<u4").view(np.uint8)
    one[48:60] = 16 * np.arange(12)
    one[60:] = np.asarray([12], "<u4").view(np.uint8)
    full0 = torch.from_numpy(one).to(dev).expand(R, K, CB).contiguous()
    out = ops.HistoryTailScores.empty(R, dev)

    legs = {
        "compact_age": (chist0, chist, lambda: ops.compact_history_age(chist, a.shift, counts=False)),
        "compact_age_counts": (chist0, chist, lambda: ops.compact_history_age(
            chist, a.shift, evicted=evicted, full=full)),
        "compact_age_full12": (full0, chist, lambda: ops.compact_history_age(chist, a.shift, counts=False)),
        "compact_copy": (chist0, chist, lambda: ccopy.copy_(chist)),
        "compact_fused": (chist0, chist, lambda: ops.segment_history_scores_compact_ragged(
            out_ns, seg_off, seg_len, K, max_len, chist, permille=pm, aligned16=True, out=out,
            folded=folded)),
    }
    dense_bytes = R * K * B * 4
    with_dense = not a.no_dense and 3 * dense_bytes + (2 << 30) < torch.cuda.mem_get_info()[0]
    changed = None
    if with_dense:
        hist0 = torch.zeros((R, K, B), dtype=torch.int32, device=dev)
        ops.segment_history_scores_ragged(out_ns, seg_off, seg_len, K, max_len, hist0, permille=pm,
                                          aligned16=True, score=False)
        changed = int((hist0.view(R * K, B // 4, 4) != 0).any(2).sum())  # vectors the pass stores
        hist, hcopy = hist0.clone(), torch.empty_like(hist0)
        legs["dense_age"] = (hist0, hist, lambda: ops.histogram_history_age(hist, a.shift))
        legs["dense_copy"] = (hist0, hist, lambda: hcopy.copy_(hist))
    times = {k: [] for k in legs}
    for it in range(a.warmup + a.reps):
        for name, (src, dst, fn) in legs.items():  # interleaved: every leg sees the same drift
            dst.copy_(src)  # the restore, not timed
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))

    res = {k: _summary(v) for k, v in times.items()}
    med = {k: res[k]["median_ms"] for k in times}
    nbytes = dict(compact_age=CB * (R * K + stores), compact_age_counts=CB * (R * K + stores),
                  compact_age_full12=2 * CB * R * K, compact_copy=2 * CB * R * K)
    if with_dense:
        nbytes.update(dense_age=dense_bytes + 16 * changed, dense_copy=2 * dense_bytes)
    line = dict(
        tool="bench_history_age", device=torch.cuda.get_device_name(0),
        shape=dict(R=R, K=K, cap=cap, permille=pm, shift=a.shift, records=R * N,
                   nonempty_elements=nonempty, entries_mean=float(n0[n0 > 0].float().mean()),
                   entries_max=int(n0.max()), evicted_by_one_pass=evicted_total,
                   compact_history_bytes=R * K * CB, dense_history_bytes=dense_bytes,
                   dense_changed_vectors=changed),
        dense_legs=with_dense, warmup=a.warmup, reps=a.reps, **res, bytes=nbytes,
        gb_per_s={k: v / med[k] / 1e6 for k, v in nbytes.items()},
        age_over_copy=dict(compact=med["compact_age"] / med["compact_copy"],
                           compact_counts=med["compact_age_counts"] / med["compact_copy"],
                           compact_full12=med["compact_age_full12"] / med["compact_copy"],
                           **({"dense": med["dense_age"] / med["dense_copy"]} if with_dense else {})),
        age_over_fused=dict(compact=med["compact_age"] / med["compact_fused"],
                            **({"dense": med["dense_age"] / med["compact_fused"]} if with_dense else {})),
    )
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
