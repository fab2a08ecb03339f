"""CPU: ``histograms.segment_tail_scores`` -- the host twin of the tail scores straight from ragged
segments -- equals, integer for integer and f64 bit for bit, the plain-Python definition
(``_tail_ref``) applied to counts built with ``bucket_of`` + ``np.bincount`` over the retained
windows; and a scenario: a rank slow on every 16th call of its hottest kernel is the one rank the
tail score singles out, while its median-based score stays at 1."""
import numpy as np
import pytest

import _segment_tail_cases as C
import _tail_ref as ref
from nvidia_resiliency_ext.straggler import histograms
from nvidia_resiliency_ext.straggler.synth import zipf_counts

CASES = [c for c in C.cases() if c.thr_index is None]


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_twin_equals_the_definition_over_the_windows(c):
    counts = [[np.bincount(histograms.bucket_of(w), minlength=ref.BINS).tolist()
               for w in C.windows(c)[r * c.K:(r + 1) * c.K]] for r in range(c.R)]
    valid = None if c.col_valid is None else c.col_valid.tolist()
    F, T, sums, rows = ref.full(counts, c.pm, col_valid=valid)
    assert histograms.segment_counts(c.keys, c.off, c.lens, c.K, c.cap).tolist() == counts
    got = histograms.segment_tail_scores(c.keys, c.off, c.lens, c.K, c.pm, c.cap, c.col_valid)
    assert got.threshold_bucket.tolist() == T
    assert (got.fleet_tail, got.fleet_total) == sums
    assert got.tail_ns.tolist() == [r["tail_ns"] for r in rows]
    assert got.total_ns.tolist() == [r["total_ns"] for r in rows]
    assert [ref.bits(s) for s in got.score] == [ref.bits(r["score"]) for r in rows]
    assert got.tail_calls.tolist() == [r["calls"] for r in rows]


def test_offsets_without_lengths_and_bad_shapes():
    keys = np.arange(10, dtype=np.uint32)
    off = np.array([0, 3, 3, 7, 10])
    a = histograms.segment_counts(keys, off, None, 2)
    b = histograms.segment_counts(keys, off[:4], [3, 0, 4, 3], 2)
    assert a.shape == (2, 2, 240) and (a == b).all() and a.sum() == 10
    with pytest.raises(ValueError):
        histograms.segment_counts(keys, off, None, 3)
    assert histograms.segment_counts(keys, off[:0], [], 0).shape == (0, 0, 240)


def test_all_zero_world_scores_nan():
    c = next(c for c in C.cases() if c.name == "all_zero_world")
    got = histograms.segment_tail_scores(c.keys, c.off, c.lens, c.K, c.pm)
    assert np.isnan(got.score).all() and got.fleet_total == 0


def test_intermittent_straggler_scenario():
    """64 ranks x 16 kernels, Zipf call counts (zipf_counts(16, top=256)), 2 % jitter; rank 37 is
    2x slower on every 16th call of kernel 0 (256 of its 753 calls; every kernel takes 10 us), pm =
    990.  The slow calls are 16 x 20 us of the rank's 7.7 ms, so its tail share is 4.2 % and the
    margin asked for first (below 0.95) is not what this scenario gives: the host twin gives
    0.95976 for the slow rank and 1.00065 for every other rank (none of their samples lies above a
    threshold bucket).  The bounds are therefore 0.97 for the slow rank and 0.01 around 1 for the
    others.  16 slow calls of 256 sit above the median, so the rank's median of kernel 0 and with
    it its median-based score stay where a healthy rank's are."""
    R, K, slow = 64, 16, 37
    calls = zipf_counts(K, top=256)
    rng = np.random.default_rng(2024)
    base = np.full(K, 10_000)
    keys, lens, med = [], [], np.zeros((R, K))
    for r in range(R):
        for k in range(K):
            x = base[k] * (1.0 + 0.02 * rng.standard_normal(calls[k]))
            if r == slow and k == 0:
                x[15::16] *= 2.0
            x = x.astype(np.uint32)
            med[r, k] = np.median(x)
            keys.append(x)
            lens.append(x.size)
    off = np.cumsum([0] + lens[:-1])
    got = histograms.segment_tail_scores(np.concatenate(keys), off, lens, K, 990)
    others = np.delete(got.score, slow)
    print("slow rank", got.score[slow], "others", others.min(), others.max())
    assert got.score[slow] < 0.97
    assert (np.abs(others - 1.0) < 0.01).all()
    assert int(np.argmin(got.score)) == slow and (got.score < 0.97).sum() == 1
    # what the report sees: ref / MED per kernel with ref = min over ranks, within the jitter of 1
    # for every rank; the slow rank is no lower than the others on its slow kernel
    rel = med.min(0) / med
    assert rel[slow, 0] >= np.delete(rel[:, 0], slow).min()
    healthy = base[0] * (1.0 + 0.02 * np.random.default_rng(1).standard_normal(256))
    slowed = healthy.copy()
    slowed[15::16] *= 2.0
    # 16 slow calls of 256 sit above the median and move it by at most the 16 ranks they displace
    assert abs(np.median(slowed) / np.median(healthy) - 1.0) < 0.005
