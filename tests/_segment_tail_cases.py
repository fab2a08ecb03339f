"""The cases of the segment tail-score tests (CPU twin and GPU kernels): ragged segments laid out
in one key array, each case aimed at a boundary of segment_tail.hip -- the lane class (<= 16
samples) against the wave class, a wave trip of 256 samples, the trimmed window, the four starts
inside a 16-byte vector, skipped segments, the bucket rule's ends, skipped columns, the split
rules of both kernels.  Built once per process and never written to."""
import functools
from collections import namedtuple

import numpy as np

KEY_WIDE = 0xE0000000
LENGTHS = [0, 1, 8, 9, 16, 17, 63, 64, 65, 255, 256, 257, 1025]

Case = namedtuple("Case", "name keys off lens R K cap aligned16 pm col_valid thr_index max_len")


def durations(rng, n, base=20_000):
    """A kernel's durations: a tight body (1 to 3 buckets) and a few slow calls."""
    x = base * (1.0 + 0.03 * rng.standard_normal(n))
    slow = rng.random(n) < 0.03
    return np.where(slow, x * rng.uniform(1.5, 6.0, n), x).clip(1, 2 ** 32 - 1).astype(np.uint32)


def layout(name, R, K, lens, fill, *, cap=0, aligned16=False, pm=990, col_valid=None,
           thr_index=None, seed=0):
    """lens [R * K] (<= 0: nothing laid out); fill(rng, g, n) -> n keys of segment g.  Starts:
    aligned16 puts every retained run on a 16-byte boundary, otherwise segment g starts at
    offset g % 4 inside its vector."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int32)
    assert lens.size == R * K
    off = np.zeros(R * K, np.int64)
    parts, pos = [], 0
    for g in range(R * K):
        n = max(int(lens[g]), 0)
        keep = cap if 0 < cap < n else n
        want = 0 if aligned16 else g % 4
        pad = (want - (pos + n - keep)) % 4  # the retained run starts at pos + pad + n - keep
        parts.append(np.full(pad, 0xDEAD, np.uint32))  # never inside a window
        pos += pad
        off[g] = pos
        if n:
            parts.append(np.asarray(fill(rng, g, n), np.uint32))
            assert parts[-1].size == n
        pos += n
    parts.append(np.full(8 - pos % 4, 0xDEAD, np.uint32))  # whole vectors past the last sample
    keys = np.concatenate(parts)
    max_len = max(int(lens.max(initial=0)), 0)
    return Case(name, keys, off, lens, R, K, cap, aligned16, pm, col_valid, thr_index, max_len)


def _kernel_fill(K):
    return lambda rng, g, n: durations(rng, n, 3_000 * (1 + g % K))


def _rot_lens(R, K, base):
    return [base[(k + r) % len(base)] for r in range(R) for k in range(K)]


def _special_fill(rng, g, n):
    k = g % 8
    if k in (0, 3):
        return np.zeros(n, np.uint32)                     # wholly in bucket 0: weight 0
    if k == 1:
        return rng.choice(np.array([7, 8], np.uint32), n)  # the bucket rule's two branches
    if k == 2:                                            # buckets 237 / 238 / 239
        return rng.choice(np.array([KEY_WIDE - 1, KEY_WIDE, 2 ** 32 - 1], np.uint32), n)
    if k == 4:
        return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return durations(rng, n, 1 << (4 + 3 * k))


def _spread_fill(rng, g, n):
    if g == 0:  # every sample in one bucket: the same LDS address for the whole wave
        return np.full(n, 20_000, np.uint32)
    if g == 1:  # 160 buckets in one segment
        b = np.arange(n) % 160 + 40
        return ((8 + b % 8) << (b // 8 - 1)).astype(np.uint32)
    return durations(rng, n)


@functools.lru_cache(maxsize=None)
def cases():
    K13 = len(LENGTHS)
    out = [
        layout("lengths_unaligned", 3, K13, _rot_lens(3, K13, LENGTHS), _kernel_fill(K13), seed=1),
        layout("lengths_aligned16", 3, K13, _rot_lens(3, K13, LENGTHS), _kernel_fill(K13),
               aligned16=True, seed=2),
        layout("cap_trims", 3, 5, _rot_lens(3, 5, [100, 101, 250, 7, 0]), _kernel_fill(5), cap=100, seed=3),
        layout("cap_trims_aligned16", 3, 5, _rot_lens(3, 5, [100, 101, 250, 7, 0]), _kernel_fill(5),
               cap=100, aligned16=True, seed=4),
        layout("negative_lengths", 4, 6, _rot_lens(4, 6, [5, -1, 40, -7, 0, 12, 300]), _kernel_fill(6),
               seed=5),
        layout("special_keys", 3, 8, _rot_lens(3, 8, [3, 20, 9, 70, 16, 17, 1]), _special_fill, pm=900,
               seed=6),
        layout("all_zero_world", 2, 3, [4, 20, 1, 0, 300, 2], lambda rng, g, n: np.zeros(n, np.uint32),
               seed=7),
        layout("clustered_and_spread", 2, 2, [1025, 320, 30, 1025], _spread_fill, pm=950, seed=8),
    ]
    rng = np.random.default_rng(9)
    for K in (1, 5, 17, 300):
        valid = (rng.random(K) < 0.7).astype(np.uint8)
        lens = rng.choice([0, 1, 2, 3, 5, 8, 16, 17, 40], 3 * K)
        out.append(layout(f"col_valid_K{K}", 3, K, lens, _kernel_fill(K), pm=950, col_valid=valid,
                          seed=10 + K))
    perm = rng.permutation(17).astype(np.int32)
    perm[[2, 11]] = -1
    out.append(layout("thr_index_permuted", 3, 17, rng.choice([0, 1, 4, 16, 17, 90], 3 * 17),
                      lambda r, g, n: durations(r, n, 8_000), pm=950, thr_index=perm, seed=40))
    # rows and splits: many splits of one row; more rows than either split rule's pivot
    few = [0, 1, 1, 2, 3, 5, 8, 13]
    out.append(layout("R1_K2048", 1, 2048, np.where(rng.random(2048) < 0.01, 70, rng.choice(few, 2048)),
                      _kernel_fill(2048), seed=41))
    out.append(layout("R70_K33", 70, 33, np.where(rng.random(70 * 33) < 0.02, 300, rng.choice(few, 70 * 33)),
                      _kernel_fill(33), seed=42))
    out.append(layout("R2049_K1", 2049, 1, np.where(rng.random(2049) < 0.01, 40, rng.choice(few, 2049)),
                      lambda r, g, n: durations(r, n, 50_000), seed=43))
    return tuple(out)


def windows(c):
    """The retained window of every segment, as arrays of keys."""
    w = []
    for g in range(c.R * c.K):
        n = int(c.lens[g])
        if n <= 0:
            w.append(c.keys[:0])
            continue
        e = int(c.off[g]) + n
        keep = c.cap if 0 < c.cap < n else n
        w.append(c.keys[e - keep:e])
    return w
