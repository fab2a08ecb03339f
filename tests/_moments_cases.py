"""Seeded input segments of the FAST AVG / STD tests (numpy, no GPU): tests/test_moments_ref_cpu.py
proves from the keys alone which branch of lean_core each one takes, the GPU tests run them."""
from fractions import Fraction

import numpy as np

KEY_WIDE = 0xE0000000


FAST_WAVE_SLOTS = 8192  # 64 lanes * PL 128: what one FAST wave holds


def sent_to_exact(keep, aligned16):
    """The FAST dispatch rule (segment_stats.hip, segment_ragged_kernels.h seg_class): a retained
    run of `keep` > 128 samples that does not start on a 16-byte boundary needs up to 3 more
    slots; beyond 8192 slots it runs the EXACT kernel, whose AVG / STD are the oracle's bits."""
    return keep + (0 if aligned16 else 3) > FAST_WAVE_SLOTS


def edge_segments(n):
    rng = np.random.default_rng(7)
    segs = [
        np.full(n, 12345, np.uint32),                                   # all equal
        np.where(rng.random(n) < 0.5, 10, 20).astype(np.uint32),       # two values
        rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32),  # full 32-bit range
        (2**24 + rng.integers(-3, 4, size=n)).astype(np.uint32),       # u32->f32 rounding edge
        np.sort(rng.integers(100, 200, size=n).astype(np.uint32)),     # sorted, narrow
        np.sort(rng.integers(100, 2**31, size=n).astype(np.uint32))[::-1].copy(),  # reverse
        # one huge bucket: most values clustered, few outliers (forces deeper levels)
        np.concatenate([np.full(n - min(n, 3), 1_000_000, np.uint32) +
                        rng.integers(0, 7, size=n - min(n, 3)).astype(np.uint32),
                        np.array([1, 4_000_000_000, 7][:min(n, 3)], np.uint32)]),
        (rng.integers(0, 2**20, size=n) * 4096 + 5).astype(np.uint32),  # sparse keys
        np.zeros(n, np.uint32),                                          # 0-ns durations
        # tight cluster + one low outlier: variance far below mean^2 (cancellation-prone)
        np.where(np.arange(n) == n - 1, 10, 100_000 + rng.integers(0, 20, size=n)).astype(np.uint32),
    ]
    return segs


def outlier_family(n, seed=0):
    """The pivot-outlier family at length n >= 8, name -> keys: a cluster 100 000 + U[0, 20) ns
    with one outlier (10 ns or 8 ms) at the first, middle or last retained sample; a three-call
    warm-up (samples 0..2 = 5 ms over 300 000 + U[0, 4000)); two of the three pivot probes
    outliers (first and last: the pivot is an outlier, the general bound still holds); and the
    all-equal segment (STD exactly 0)."""
    assert n >= 8
    rng = np.random.default_rng(1000 * n + seed)
    fam = {}
    for name, val in (("lo", 10), ("hi", 8_000_000)):
        for where, at in (("first", 0), ("mid", n // 2), ("last", n - 1)):
            k = (100_000 + rng.integers(0, 20, size=n)).astype(np.uint32)
            k[at] = val
            fam[f"{name}@{where}"] = k
    k = (300_000 + rng.integers(0, 4000, size=n)).astype(np.uint32)
    k[:3] = 5_000_000
    fam["warmup3"] = k
    k = (100_000 + rng.integers(0, 20, size=n)).astype(np.uint32)
    k[0] = k[n - 1] = 8_000_000
    fam["two_probes"] = k
    fam["equal"] = np.full(n, 123_456, np.uint32)
    return fam


# names of the family members whose pivot (median of first / middle / last) is in the cluster
FAMILY_PIVOT_IN_CLUSTER = ("lo@first", "lo@mid", "lo@last", "hi@first", "hi@mid", "hi@last", "warmup3")


def branch_family(n, seed=0):
    """One segment per sum branch, name = the branch (tests/_moments_ref.py `branch`)."""
    rng = np.random.default_rng(77 * n + seed)
    return {
        "r23": (5_000_000 + rng.integers(0, (1 << 23) - 1, size=n)).astype(np.uint32),
        "r24": np.concatenate([[1000, 1000 + (1 << 23) + 12345],
                               1000 + rng.integers(0, (1 << 23) + 12345, size=n - 2)]).astype(np.uint32),
        "r31": np.concatenate([[7, 7 + (1 << 24) + 99_999],
                               7 + rng.integers(0, (1 << 24) + 99_999, size=n - 2)]).astype(np.uint32),
        "r32": np.concatenate([[3, 3 + (1 << 31) + 5],
                               3 + rng.integers(0, (1 << 31) + 5, size=n - 2)]).astype(np.uint32),
        "wide": np.concatenate([[KEY_WIDE + 17, 2_000_000_000],
                                rng.integers(1_000_000_000, 0xE8000000, size=n - 2)]).astype(np.uint32),
    }


def midpoint_segment(n, seed=0):
    """A segment (range < 2^23, keys near 3.0e9 ns) whose exact mean in us lies one unit of the
    integer sum away from the midpoint of two adjacent float32 values: about 4e-14 relative at
    n = 1000 -- inside 2^-40, far outside the 2^-52 of the kernel's quotient.  The sum sits on
    the side of the midpoint away from the even neighbour, so a kernel that lands on the midpoint
    itself (ties to even) rounds the wrong way."""
    rng = np.random.default_rng(4242 + n + seed)
    lo = np.float32(3.0e6)  # us
    hi = np.nextafter(lo, np.float32(np.inf))
    mid = (Fraction(float(lo)) + Fraction(float(hi))) / 2
    target = mid * 1000 * n  # the integer sum of keys that would hit the midpoint
    assert target.denominator == 1
    odd_is_hi = bool(int(hi.view(np.uint32)) & 1)
    s1 = int(target) + (1 if odd_is_hi else -1)
    base = int(target) // n
    k = base + rng.integers(-1000, 1000, size=n).astype(np.int64)
    diff = s1 - int(k.sum())
    k += diff // n
    k[: diff % n] += 1
    assert int(k.sum()) == s1 and k.max() < KEY_WIDE and k.min() > 0
    return k.astype(np.uint32)
