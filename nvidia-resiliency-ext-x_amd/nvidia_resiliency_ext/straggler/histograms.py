"""The fixed buckets of the duration histograms, on the host (numpy only, no native library).

``ops.segment_histogram_*``, ``KernelProfiler.get_histograms``, ``Detector.kernel_histograms``
and ``MatrixReporter.histograms`` count duration keys (``_native.duration_keys``: plain ns below
3.76 s) into ``BINS`` = 240 log-linear buckets with 3 mantissa bits, each at most 12.5 % wide::

    bucket(x) = x                                  x < 8
              = 8*(e-2) + ((x >> (e-3)) & 7)       otherwise, e = x.bit_length() - 1
    edge(b)   = b                                  b < 8      (lower edge, a key)
              = (8 + b%8) << (b//8 - 1)            otherwise; edge(240) = 2**32

``bucket`` is monotone in the duration, ``edge(bucket(x)) <= x < edge(bucket(x) + 1)``, and
``edge(238) == KEY_WIDE``: buckets 238 and 239 hold exactly the durations of 3.76 s and more.
The edges are the same for every kernel, rank and report (they are part of the C ABI), so
counts add: ``merge`` over ranks gives the fleet-wide distribution of a kernel, over reports a
whole run's, and ``quantile_bounds`` brackets any quantile of the merged samples by one bucket.
"""
from __future__ import annotations

import numpy as np

BINS = 240
KEY_WIDE = 0xE0000000
_KEY_WIDE_F32BITS = 0x4F600000


def bucket_of(keys) -> np.ndarray:
    """Bucket (int64, 0..239) of every u32 duration key."""
    x = np.asarray(keys).astype(np.uint64)
    if x.size and int(x.max()) >= 1 << 32:
        raise ValueError("keys must be u32 duration keys")
    # e - 3 for x >= 8 (0 below): the exponent of x | 8, exact in f64 for a 32-bit integer
    sh = np.frexp((x | np.uint64(8)).astype(np.float64))[1].astype(np.int64) - 4
    return 8 * sh + (x >> sh.astype(np.uint64)).astype(np.int64)


def edges_keys() -> np.ndarray:
    """The 241 bucket edges as duration keys (u64): bucket b is [edges[b], edges[b + 1])."""
    b = np.arange(BINS + 1, dtype=np.uint64)
    hi = (np.uint64(8) + b % np.uint64(8)) << np.maximum(b // np.uint64(8), np.uint64(1)) - np.uint64(1)
    return np.where(b < 8, b, hi)


def _keys_to_us(keys: np.ndarray) -> np.ndarray:
    # key_to_f32(key) / 1000.0f, as every sample is converted (include/nvrx_straggler.h)
    k = keys.astype(np.uint32)
    wide = (k.astype(np.int64) - KEY_WIDE + _KEY_WIDE_F32BITS).astype(np.uint32).view(np.float32)
    return np.where(k < KEY_WIDE, k.astype(np.float32), wide) / np.float32(1000.0)


def edges_us() -> np.ndarray:
    """The 241 bucket edges in microseconds (f32), converted like every sample; the last is +inf."""
    e = edges_keys()
    us = np.empty(BINS + 1, np.float32)
    us[:BINS] = _keys_to_us(e[:BINS])
    us[BINS] = np.inf
    return us


def merge(*counts) -> np.ndarray:
    """Sum of histograms (arrays of equal shape [..., 240]; torch tensors on the host are taken
    too) as int64: counts of the same buckets add, over ranks and over reports."""
    if not counts:
        raise ValueError("merge needs at least one histogram")
    total = None
    for c in counts:
        a = np.asarray(c)
        if a.dtype == np.int32:  # device counts are u32 in an int32 tensor
            a = a.view(np.uint32)
        a = a.astype(np.int64)
        if a.shape[-1:] != (BINS,):
            raise ValueError(f"a histogram has {BINS} bins in its last dimension, got shape {a.shape}")
        total = a if total is None else total + a
    return total


def quantile_bounds(counts, permille: int):
    """``(lo_us, hi_us)`` of the bucket that holds the quantile ``permille`` (an int in
    [0, 1000]) of the n samples counted in ``counts`` ([240]): the sample of 0-based rank
    ``(permille * (n - 1)) // 1000``, the rank rule of the quantile calls, lies in
    ``[lo_us, hi_us)`` (``hi_us`` is +inf for the last bucket).  (NaN, NaN) for n = 0."""
    if isinstance(permille, bool) or int(permille) != permille or not 0 <= permille <= 1000:
        raise ValueError(f"permille must be an int in [0, 1000], got {permille!r}")
    c = merge(counts)
    if c.shape != (BINS,):
        raise ValueError(f"counts must have shape [{BINS}]")
    n = int(c.sum())
    if n == 0:
        return float("nan"), float("nan")
    k = (int(permille) * (n - 1)) // 1000
    b = int(np.searchsorted(np.cumsum(c), k, side="right"))
    us = edges_us()
    return float(us[b]), float(us[b + 1])
