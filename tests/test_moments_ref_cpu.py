"""The exact FAST-moments reference (tests/_moments_ref.py) against numpy, the C oracle and closed
forms, and the input conditions the GPU tests (tests/test_gpu_fast_moments.py) rely on: which sum
branch of lean_core every case takes, where its pivot lies, and the crafted AVG midpoint segment.
No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _moments_cases as C
import _moments_ref as M
import oracle as O

U32 = 2.0 ** -24
GPU_FAMILY_N = (100, 200, 255, 256, 300, 400, 1000, 1024, 1100, 8189, 8191, 8192)  # lengths the GPU file uses
GPU_BRANCH_N = (64, 1000, 8192)


@pytest.mark.parametrize("n", [1, 2, 7, 1000, 8192])
def test_against_numpy_f64(n):
    rng = np.random.default_rng(n)
    k = rng.integers(1000, 3_000_000, size=n, dtype=np.uint32)
    m = M.moments(k)
    assert abs(float(m.avg) - k.astype(np.float64).mean() / 1000) <= 1e-13 * float(m.avg)
    assert abs(m.std - k.astype(np.float64).std() / 1000) <= 1e-12 * max(m.std, 1e-300)
    assert m.avg_f32 == np.float32(float(m.avg))  # no double-rounding case in these draws
    lo, hi = M.f32_bracket(m.avg)
    assert Fraction(float(lo)) <= m.avg <= Fraction(float(hi)) and hi <= np.nextafter(lo, np.float32(np.inf))
    b = M.batch(k[None, :])
    assert abs(b.avg[0] - float(m.avg)) <= 4 * M.U64 * float(m.avg)
    assert abs(b.std[0] - m.std) <= 4 * M.U64 * m.std
    if n > 2:
        assert abs(b.z2[0] - m.z2) <= 1e-12 * max(m.z2, 1e-300)
        assert abs(b.bound[0] - M.std_bound(m)) <= 1e-15


@pytest.mark.parametrize("n", [5, 100, 1000, 8192])
def test_against_oracle_compute_stats(n):
    """computeStats sums f32 us values one after another: its AVG is within gamma_(n+2)(2^-24) of
    exact (two roundings per converted sample, n - 1 additions, the divide), its STD within
    (n + 5) 2^-24 max|x| / sigma (the deviations inherit the mean's and the samples' absolute
    error) + (n + 4) 2^-24 (the sum of squares, the divide, the root)."""
    rng = np.random.default_rng(100 + n)
    k = rng.integers(1000, 3_000_000, size=n, dtype=np.uint32)
    m = M.moments(k)
    r = O.compute_stats(O.key_to_us(k))
    assert abs(r.avg - float(m.avg)) <= M.gamma(n + 2, U32) * float(m.avg)
    bound = (n + 5) * U32 * (int(k.max()) / 1000 / m.std) + (n + 4) * U32
    assert abs(r.stddev - m.std) <= bound * m.std


def test_closed_forms():
    for n in (1, 2, 64, 1000, 8192):
        m = M.moments(np.full(n, 12345, np.uint32))
        assert m.sigma2 == 0 and m.std == 0.0 and m.avg == Fraction(12345, 1000) and m.z2 == 0.0
        assert M.std_err(np.float32(0.0), m) == 0.0
        assert M.std_err(np.float32(-0.0), m) == math.inf and M.std_err(np.float32(1e-30), m) == math.inf
    for a, b, n in ((10, 20, 64), (7, 4_000_000_000, 1000), (0, 1, 8192)):
        k = np.where(np.arange(n) % 2 == 0, a, b).astype(np.uint32)
        m = M.moments(k)
        if m.branch != "wide":
            assert m.var == Fraction((a - b) ** 2, 4 * 10 ** 6) and m.avg == Fraction(a + b, 2000)
            assert m.std == abs(a - b) / 2 / 1000
    # wide keys are averaged over their decoded f32(ns) values
    k = np.array([M.KEY_WIDE + 5, 1 << 24 | 1], np.uint32)
    vals = O.key_to_f32(k).astype(np.float64)
    m = M.moments(k)
    assert m.branch == "wide" and float(m.avg) == vals.mean() / 1000 and m.std == vals.std() / 1000


def test_round_f32_rules():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2))
    mid = (Fraction(float(one)) + Fraction(float(up))) / 2
    assert M.round_f32(Fraction(1))[:2] == (one, one)
    near, far, dist = M.round_f32(mid)                      # tie: to even (1.0)
    assert near == one and far == up and dist == 0.0
    near, far, dist = M.round_f32(mid + Fraction(1, 2 ** 70))
    assert near == up and far == one and 0 < dist < 2.0 ** -69
    m = M.moments(np.array([1000, 1000], np.uint32))
    assert M.avg_ok(one, m) and not M.avg_ok(up, m)


def test_bound_shape():
    """The bound stays under the former flat 1e-6 for |z| <= 1.3 and grows as 1 + z^2."""
    assert M.std_bound_terms("r23", 8192, 0.0) < 4.0e-7
    assert M.std_bound_terms("r23", 8192, 1.3 ** 2) < 1e-6 < M.std_bound_terms("r23", 8192, 4.0)
    assert M.std_bound_terms("r31", 8192, 0.0) < 4.6e-7
    assert M.std_bound_terms("r32", 8192, 0.0, zmin2=3.0) < 1.6e-7
    assert M.std_bound_terms("wide", 8192, 0.0, mean_over_sigma2=100.0) < 6.1e-8
    big = M.std_bound_terms("r23", 8192, 8192.0)
    assert abs(big / (M.gamma(8, U32) * 8193 / 2) - 1) < 1e-2


@pytest.mark.parametrize("n", GPU_FAMILY_N)
def test_outlier_family_conditions(n):
    fam = C.outlier_family(n)
    for name, k in fam.items():
        assert k.size == n and M.branch(k) == "r23", name   # packed f32 squares, registers as floats
        m = M.moments(k)
        m0 = M.moments(k, c=int(k[0]))                       # the first retained sample as the pivot
        if name == "equal":
            assert m.sigma2 == 0 and m.z2 == 0.0
        elif name in C.FAMILY_PIVOT_IN_CLUSTER:
            # the median of the three probes is a cluster sample: the bound is the z ~ 0 one
            assert 90_000 <= m.c <= 400_000 and m.z2 < 0.3, (name, m.c, m.z2)
            assert M.std_bound(m) < 5.2e-7, (name, M.std_bound(m))
        else:
            # two probes are outliers, so is the pivot: only the general bound holds
            assert name == "two_probes" and m.c == 8_000_000 and m.z2 > n / 4
            assert M.std_bound(m) > 1e-6
        if name.endswith("@first") or name == "warmup3":
            # with sample 0 as the pivot these are the cases whose squares cancel
            assert m0.z2 > n / 8 and (n < 1000 or M.std_bound(m0) > 1e-5), (name, m0.z2)


@pytest.mark.parametrize("n", GPU_BRANCH_N)
def test_branch_family_conditions(n):
    for name, k in C.branch_family(n).items():
        assert k.size == n and M.branch(k) == name
        rng_ = int(k.max()) - int(k.min())
        want = {"r23": rng_ < 1 << 23, "r24": 1 << 23 <= rng_ < 1 << 24, "r31": 1 << 24 <= rng_ < 1 << 31,
                "r32": rng_ >= 1 << 31 and int(k.max()) < M.KEY_WIDE, "wide": int(k.max()) >= M.KEY_WIDE}
        assert want[name], (name, rng_)
        m = M.moments(k)
        # uniform draws with the minimum first: |z| is of order 1, the bound of order 1e-6
        assert m.sigma2 > 0 and m.z2 < 4.0 and M.std_bound(m) < 2e-6, (name, m.z2, M.std_bound(m))
    seen = {M.branch(k) for k in C.edge_segments(n)}
    assert {"r23", "r31", "wide"} <= seen <= set(M.BRANCHES)
    assert M.moments(C.edge_segments(n)[0]).sigma2 == 0 and M.moments(C.edge_segments(n)[8]).sigma2 == 0


@pytest.mark.parametrize("n", [1000, 1024])
def test_midpoint_segment(n):
    k = C.midpoint_segment(n)
    m = M.moments(k)
    assert k.size == n and m.branch == "r23"
    assert 4 * M.QUOT_REL < m.mid_dist < 2.0 ** -40, m.mid_dist
    assert m.mid_dist > 4 * M.avg_rel(m)
    assert int(m.avg_f32.view(np.uint32)) & 1          # the exact mean is on the odd neighbour's side
    assert not M.avg_ok(m.avg_other, m) and M.avg_ok(m.avg_f32, m)
    assert np.float32(k.astype(np.float64).mean() / 1000) in (m.avg_f32, m.avg_other)


def test_dispatch_rule():
    assert not C.sent_to_exact(8192, True) and C.sent_to_exact(8192, False)
    assert not C.sent_to_exact(8189, False) and C.sent_to_exact(8190, False) and C.sent_to_exact(8193, True)
