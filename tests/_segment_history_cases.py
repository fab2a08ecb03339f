"""The cases of the segment history-score tests (CPU twin and GPU kernel): a case is a sequence of
2-3 intervals of ragged segments over one (R, K) -- each interval a ``_segment_tail_cases.layout``
with its own lengths -- plus the history arguments (starting history, permille, col_valid,
hist_index / hist_stride, skip_rows).  Each case is aimed at a boundary of segment_history.hip: a
sample trip of 64 and of 256, the trimmed window, the four starts inside a 16-byte vector, empty
and negative lengths, the bucket rule's ends, an element that gains or loses its samples between
intervals, slots that are not the columns, skipped rows, a bin that saturates, a tail of nothing
and of everything, the split rule.  Built once per process and never written to."""
import functools
from collections import namedtuple

import numpy as np

import _segment_tail_cases as ST
from nvidia_resiliency_ext.straggler import histograms

BINS = 240
SENTINEL = 0xABCD0123  # in every bin of a slot no column uses
NEAR_FULL = 2 ** 32 - 2
KEY_WIDE = ST.KEY_WIDE

HCase = namedtuple("HCase", "name R K intervals pm col_valid hist_index stride skip_rows hist0")


def bucket(x):
    return int(histograms.bucket_of(np.asarray([x], np.uint32))[0])


def _kernel_fill(K):
    return lambda rng, g, n: ST.durations(rng, n, 3_000 * (1 + g % K))


def _rot(R, K, base, shift=0):
    return [base[(k + r + shift) % len(base)] for r in range(R) for k in range(K)]


def _special_fill(rng, g, n):
    k = g % 8
    if k in (0, 3):
        return np.zeros(n, np.uint32)                      # wholly in bucket 0: weight 0
    if k == 1:
        return rng.choice(np.array([7, 8], np.uint32), n)   # the bucket rule's two branches
    if k == 2:                                             # buckets 237 / 238 / 239
        return rng.choice(np.array([KEY_WIDE - 1, KEY_WIDE, 2 ** 32 - 1], np.uint32), n)
    if k == 4:
        return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return ST.durations(rng, n, 1 << (4 + 3 * k))


def make(name, R, K, lens_per_interval, fill, *, cap=0, aligned16=False, pm=990, col_valid=None,
         hist_index=None, stride=0, skip_rows=None, hist0=None, seed=0):
    ivs = tuple(ST.layout(f"{name}#{i}", R, K, lens, fill[i] if isinstance(fill, (list, tuple)) else fill,
                          cap=cap, aligned16=aligned16, pm=pm, seed=1000 * seed + i)
                for i, lens in enumerate(lens_per_interval))
    assert 2 <= len(ivs) <= 3
    if hist0 is None:
        hist0 = np.zeros((R, stride or K, BINS), np.uint32)
    assert hist0.shape == (R, stride or K, BINS) and hist0.dtype == np.uint32
    return HCase(name, R, K, ivs, pm, col_valid, hist_index, stride, skip_rows, hist0)


def _const(v):
    return lambda rng, g, n: np.full(n, v, np.uint32)


def _by_column(*fills):
    return lambda rng, g, n: fills[g % len(fills)](rng, g, n)


@functools.lru_cache(maxsize=None)
def cases():
    L = ST.LENGTHS
    K13 = len(L)
    out = [
        make("lengths_unaligned", 3, K13, [_rot(3, K13, L, i) for i in range(3)], _kernel_fill(K13), seed=1),
        make("lengths_aligned16", 3, K13, [_rot(3, K13, L, i) for i in range(3)], _kernel_fill(K13),
             aligned16=True, seed=2),
        make("cap_trims", 3, 5, [_rot(3, 5, [100, 101, 250, 7, 0], i) for i in range(3)], _kernel_fill(5),
             cap=100, seed=3),
        make("cap_trims_aligned16", 3, 5, [_rot(3, 5, [100, 101, 250, 7, 0], i) for i in range(2)],
             _kernel_fill(5), cap=100, aligned16=True, seed=4),
        make("negative_lengths", 4, 6, [_rot(4, 6, [5, -1, 40, -7, 0, 12, 300], i) for i in range(3)],
             _kernel_fill(6), seed=5),
        make("special_keys", 3, 8, [_rot(3, 8, [3, 20, 9, 70, 16, 17, 1], i) for i in range(3)],
             _special_fill, pm=900, seed=6),
        # (0, 1): empty, then filled -- no history yet when its first samples come;
        # (0, 2): filled, then empty -- a history but no samples; (1, *): the same one interval later
        make("empty_and_filled", 2, 4, [[30, 0, 70, 5, 9, 9, 0, 300],
                                        [30, 40, 0, 5, 9, 0, 80, 300],
                                        [30, 40, 0, 0, 9, 33, 80, -2]], _kernel_fill(4), seed=7),
    ]
    rng = np.random.default_rng(9)
    for K in (1, 5, 17, 300):
        valid = (rng.random(K) < 0.7).astype(np.uint8)
        if K == 1:
            valid[:] = 0
        lens = [rng.choice([0, 1, 2, 3, 5, 8, 16, 17, 40, 70], 3 * K) for _ in range(2)]
        out.append(make(f"col_valid_K{K}", 3, K, lens, _kernel_fill(K), pm=950, col_valid=valid, seed=10 + K))
    # slots that are not the columns: a permutation into 20 slots, two columns without one; the
    # five slots no column uses hold a sentinel
    S = 20
    index = rng.permutation(S)[:17].astype(np.int32)
    index[[2, 11]] = -1
    h0 = np.zeros((3, S, BINS), np.uint32)
    h0[:, sorted(set(range(S)) - {int(s) for s in index if s >= 0})] = SENTINEL
    out.append(make("hist_index_permuted", 3, 17, [rng.choice([0, 1, 4, 16, 17, 90], 3 * 17) for _ in range(3)],
                    lambda r, g, n: ST.durations(r, n, 8_000), pm=950, hist_index=index, stride=S,
                    hist0=h0, seed=40))
    h0 = np.zeros((2, 9, BINS), np.uint32)
    h0[:, 5:] = SENTINEL
    out.append(make("stride_above_K", 2, 5, [rng.choice([0, 3, 20, 65], 10) for _ in range(2)],
                    _kernel_fill(5), stride=9, hist0=h0, seed=44))
    out.append(make("skip_rows", 4, 6, [rng.choice([0, 2, 17, 64, 100], 24) for _ in range(3)],
                    _kernel_fill(6), skip_rows=np.array([0, 1, 0, 1], np.uint8), seed=45))
    # a history bin at 2^32 - 2 that receives 1 sample (2^32 - 1 exactly), then 5 (saturates)
    h0 = np.zeros((1, 2, BINS), np.uint32)
    h0[0, 0, bucket(20_000)] = NEAR_FULL
    h0[0, 0, bucket(20_000) - 1] = 7
    out.append(make("saturation", 1, 2, [[1, 30], [5, 30]], _by_column(_const(20_000), _kernel_fill(2)),
                    hist0=h0, seed=46))
    # column 0: every sample below the history's T; column 1: every sample above it
    h0 = np.zeros((1, 2, BINS), np.uint32)
    h0[0, 0, bucket(20_000)] = 100_000
    h0[0, 1, bucket(1_000)] = 100_000
    out.append(make("tail_of_nothing_and_everything", 1, 2, [[70, 300], [5, 17]],
                    _by_column(_const(1_000), _const(1_000_000)), hist0=h0, seed=47))
    # rows and splits, lengths as in _segment_tail_cases
    few = [0, 1, 1, 2, 3, 5, 8, 13]
    out.append(make("R1_K2048", 1, 2048,
                    [np.where(rng.random(2048) < 0.01, 70, rng.choice(few, 2048)) for _ in range(2)],
                    _kernel_fill(2048), seed=41))
    out.append(make("R70_K33", 70, 33,
                    [np.where(rng.random(70 * 33) < 0.02, 300, rng.choice(few, 70 * 33)) for _ in range(2)],
                    _kernel_fill(33), seed=42))
    out.append(make("R2049_K1", 2049, 1,
                    [np.where(rng.random(2049) < 0.01, 40, rng.choice(few, 2049)) for _ in range(2)],
                    lambda r, g, n: ST.durations(r, n, 50_000), seed=43))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def history_kwargs(c):
    """The history keywords of a case for the host twins (hist_stride is the history's shape there)."""
    return dict(hist_index=c.hist_index, col_valid=c.col_valid, skip_rows=c.skip_rows)


@functools.lru_cache(maxsize=None)
def walk(name):
    """Per interval of a case (counts of the retained windows, the history before, the twin's
    fused result): the reference every test shares, computed once and never written to."""
    c = case(name)
    h, out = c.hist0, []
    for iv in c.intervals:
        counts = histograms.segment_counts(iv.keys, iv.off, iv.lens, c.K, iv.cap)
        res = histograms.history_scores(counts, h, c.pm, score_thr=0.9, **history_kwargs(c))
        out.append((counts, h, res))
        h = res.hist
    return tuple(out)
