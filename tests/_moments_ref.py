"""The plain exact reference of the FAST-mode AVG / STD (numpy / Python integers, no GPU) and
the error bound of the kernel's arithmetic, branch by branch.

A segment is the retained u32 duration keys of one ring, in push order.  Below KEY_WIDE a key is
the duration in ns; the sum S1 and the sum of squares S2 are Python integers and

    AVG = S1 / (1000 n)                     VAR = (n S2 - S1^2) / (1000 n)^2      (us, us^2)

are exact rationals.  A segment with a key at or above KEY_WIDE is averaged over the decoded
f32(ns) values (integers as well), as `wide_moments` (csrc/segment_emit.h) does.

The pivot c of the kernel's f32 squares is a sample: the median of the first, middle and last
retained sample (`pivot`), or the sample the caller names.  With z = (c - mean) / sigma the sum
of squares about c is n sigma^2 (1 + z^2), and its f32 rounding is relative to that sum, not to
sigma^2: the bound carries the factor (1 + z^2).

    branch   keys                          squares
    r23      range < 2^23                  packed f32 about c, the registers taken as floats
    r24      2^23 <= range < 2^24          packed f32 about c, exact conversions
    r31      2^24 <= range < 2^31          f32 about c, (float)(int)(d - c) rounds
    r32      2^31 <= range, below KEY_WIDE f64 about MIN (c plays no part)
    wide     a key >= KEY_WIDE             two-pass f64 over the decoded values
"""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

KEY_WIDE = 0xE0000000
KEY_WIDE_F32BITS = 0x4F600000
U32 = 2.0 ** -24   # unit roundoff of float32
U64 = 2.0 ** -53   # unit roundoff of float64
BRANCHES = ("r23", "r24", "r31", "r32", "wide")
# quot_f64 (segment_emit.h): the reciprocal after two Newton steps is within ~2^-52, the quotient
# num * rc is corrected by its own exactly computed residual, and the last fma rounds once: the
# result is within 2^-53 (1 + O(2^-50)) of num / dd.  2^-52 is stated.
QUOT_REL = 2.0 ** -52


def gamma(m, u):
    """Higham's gamma_m: the relative error bound of m successive roundings."""
    return m * u / (1.0 - m * u)


def key_ints(keys):
    """The values behind u32 duration keys as Python integers (ns): the keys themselves below
    KEY_WIDE, else every key decoded to its f32(ns) value (an integer, too)."""
    k = np.asarray(keys, np.uint32)
    if k.size and int(k.max()) >= KEY_WIDE:
        wide = (k.astype(np.uint64) - KEY_WIDE + KEY_WIDE_F32BITS).astype(np.uint32).view(np.float32)
        f = np.where(k < KEY_WIDE, k.astype(np.float32), wide).astype(np.float32)
        return [int(x) for x in f.astype(np.float64)]
    return [int(x) for x in k]


def branch(keys):
    """Which sum branch of lean_core (or wide_moments) a segment takes, from its keys alone."""
    k = np.asarray(keys, np.uint32)
    if int(k.max()) >= KEY_WIDE:
        return "wide"
    r = int(k.max()) - int(k.min())
    return "r23" if r < 1 << 23 else "r24" if r < 1 << 24 else "r31" if r < 1 << 31 else "r32"


def pivot_index(n):
    """Indices of the three probes of the pivot rule: first, middle, last retained sample."""
    return 0, n // 2, n - 1


def pivot(keys):
    """The kernel's pivot: the median of the three probes (a sample of the segment)."""
    k = np.asarray(keys, np.uint32)
    return sorted(int(k[i]) for i in pivot_index(k.size))[1]


def f32_bracket(q):
    """(lo, hi): the float32 neighbours of the rational q, lo <= q <= hi (equal when q is one)."""
    q = Fraction(q)
    f = np.float32(float(q))
    while Fraction(float(f)) > q:
        f = np.nextafter(f, np.float32(-np.inf))
    while Fraction(float(np.nextafter(f, np.float32(np.inf)))) <= q:
        f = np.nextafter(f, np.float32(np.inf))
    if Fraction(float(f)) == q:
        return f, f
    return f, np.nextafter(f, np.float32(np.inf))


def round_f32(q):
    """(the correctly rounded float32 of the rational q -- nearest, ties to even --, the other
    neighbour, the relative distance of q from the midpoint of the two)."""
    q = Fraction(q)
    lo, hi = f32_bracket(q)
    if lo == hi:
        return lo, lo, 1.0
    L, H = Fraction(float(lo)), Fraction(float(hi))
    mid = (L + H) / 2
    if q < mid or (q == mid and not (int(lo.view(np.uint32)) & 1)):
        near, far = lo, hi
    else:
        near, far = hi, lo
    return near, far, float(abs(q - mid) / abs(q)) if q else 1.0


def moments(keys, c=None):
    """Exact moments of one segment.  c: the pivot sample (default: `pivot(keys)`).

    avg, var      Fractions (us, us^2);  avg_f32 the correctly rounded f32 of avg, avg_other its
                  other f32 neighbour (avg_f32 itself when avg is a float32), mid_dist the
                  relative distance of avg from their midpoint
    std           the exact std (us) to f64 accuracy: sqrt of the correctly rounded f64 variance
    sigma2, dev2  sigma^2 and (c - mean)^2 in ns^2 (Fractions); z2 = dev2 / sigma2 (float, inf
                  when sigma is 0 and c is not the mean); zmin2 the same for c = MIN
    """
    k = np.asarray(keys, np.uint32)
    n = int(k.size)
    assert n >= 1
    x = key_ints(k)
    s1 = sum(x)
    s2 = sum(v * v for v in x)
    br = branch(k)
    if c is None:
        c = pivot(k)
    cv = key_ints(np.array([c, int(k.max())], np.uint32))[0] if br == "wide" else int(c)
    mean = Fraction(s1, n)
    sigma2 = Fraction(n * s2 - s1 * s1, n * n)
    avg = mean / 1000
    var = sigma2 / 1000000
    near, far, dist = round_f32(avg)
    dev2 = (cv - mean) ** 2
    devmin2 = (min(x) - mean) ** 2
    z2 = float(dev2 / sigma2) if sigma2 else (0.0 if dev2 == 0 else math.inf)
    zmin2 = float(devmin2 / sigma2) if sigma2 else (0.0 if devmin2 == 0 else math.inf)
    # Fraction -> float is correctly rounded; sqrt is correctly rounded: 2^-53 (1/2 + 1) relative
    std = math.sqrt(float(var))
    return SimpleNamespace(n=n, branch=br, c=int(c), avg=avg, var=var, avg_f32=near, avg_other=far,
                           mid_dist=dist, std=std, sigma2=sigma2, dev2=dev2, z2=z2, zmin2=zmin2,
                           mean_over_sigma2=float(mean * mean / sigma2) if sigma2 else math.inf)


def _std_from_var_rel(R, root_rel):
    """Relative error of the root of a variance that is off by at most R (relative), the root
    itself off by root_rel: |sqrt(1 - R) - 1| = R / (1 + sqrt(1 - R)) <= R / (2 - R) is the
    larger side; beyond R = 1 the variance may have been clamped to 0 (error 1)."""
    a = R / (2.0 - R) if R < 1.0 else max(1.0, math.sqrt(1.0 + R) - 1.0)
    return (1.0 + a) * (1.0 + root_rel) - 1.0


def std_bound_terms(br, n, z2, zmin2=0.0, mean_over_sigma2=0.0):
    """The bound on |STD_kernel - STD| / STD from the kernel's arithmetic (not its output).

    r23 / r24: a lane sums its squares in packed-f32 groups of 16 registers, two accumulators of
    8 fused multiply-adds each (fewer for PL < 16), (d - c) exact in f32: each accumulator is
    within gamma_8(2^-24) of its exact non-negative sum, hence so is the segment's
    sq = sum (d - c)^2 = n sigma^2 (1 + z^2); the groups and lanes are added in f64.
    r31: (float)(int)(d - c) rounds once before squaring, two more roundings per term: gamma_10.
    The epilogue forms n sq - se^2 in f64 (se exact; se * se rounds, the fma rounds, quot_f64 is
    within 2^-52): 2^-50 (1 + z^2) covers them and the f64 additions of sq.  The quotient is
    rounded to f32 (2^-24) and v_sqrt_f32 is within 1 ulp (2^-23 relative).
    r32: f64 squares about MIN, at most 64 fused multiply-adds per accumulator and the wave sum:
    80 * 2^-53 relative to n sigma^2 (1 + zmin^2), then as above.
    wide: two f64 passes (n / 64 additions per lane, the wave sums, the divide): the mean is within
    e = (n / 64 + 8) 2^-53, the squares about it within 2 e, the shifted mean adds
    (mean / sigma)^2 e^2; f64 sqrt, the divide by 1000 and one f32 rounding (2^-24)."""
    if br in ("r23", "r24"):
        R = (gamma(8, U32) + 2.0 ** -50) * (1.0 + z2) + U32
        return _std_from_var_rel(R, 2.0 * U32)
    if br == "r31":
        R = (gamma(10, U32) + 2.0 ** -50) * (1.0 + z2) + U32
        return _std_from_var_rel(R, 2.0 * U32)
    if br == "r32":
        R = (80 * U64 + 2.0 ** -50) * (1.0 + zmin2) + U32
        return _std_from_var_rel(R, 2.0 * U32)
    assert br == "wide", br
    e = (n / 64 + 8) * U64
    R = 2 * e + mean_over_sigma2 * e * e + 4 * U64
    return _std_from_var_rel(R, U32 + 4 * U64)


def std_bound(m):
    """`std_bound_terms` of the segment `moments` describes (sigma > 0)."""
    return std_bound_terms(m.branch, m.n, m.z2, m.zmin2, m.mean_over_sigma2)


def avg_rel(m):
    """How far the f64 quotient the kernel rounds to f32 may be from the exact AVG (relative):
    numerator and denominator are exact integers below 2^53 (n MIN + sd, 1000 n), so quot_f64's
    2^-52; wide segments sum n / 64 values per lane and the wave in f64, divide by n and by
    1000 -- (n / 64 + 8) 2^-53 (sums of integers below 2^53 are exact, the stated bound still
    holds)."""
    return (m.n / 64 + 8) * U64 if m.branch == "wide" else QUOT_REL


def avg_ok(got, m):
    """AVG must be the correctly rounded f32 of the exact rational; the other neighbour only
    where the exact value lies within `avg_rel` of their midpoint."""
    got = np.float32(got)
    if got.view(np.uint32) == m.avg_f32.view(np.uint32):
        return True
    return bool(got.view(np.uint32) == m.avg_other.view(np.uint32) and m.mid_dist <= avg_rel(m))


def std_err(got, m):
    """Relative error of a kernel STD (0 / inf for a zero-variance segment: exact 0.0 demanded)."""
    got = float(np.float32(got))
    if m.sigma2 == 0:
        return 0.0 if (got == 0.0 and not math.copysign(1.0, got) < 0) else math.inf
    return abs(got - m.std) / m.std


def check(got_avg, got_std, keys, c=None, tag=""):
    """Assert one segment's FAST AVG / STD against the exact moments; returns (relative STD
    error, its bound) so that callers can report the worst case."""
    m = moments(keys, c)
    assert avg_ok(got_avg, m), (tag, "avg", float(got_avg), float(m.avg_f32), float(m.avg_other),
                                m.mid_dist)
    err = std_err(got_std, m)
    if m.sigma2 == 0:
        assert err == 0.0, (tag, "std of a constant segment must be +0.0", float(got_std))
        return 0.0, 0.0
    bound = std_bound(m)
    assert err <= bound, (tag, "std", float(got_std), m.std, f"err {err:.3e} > bound {bound:.3e}",
                          m.branch, f"z2 {m.z2:.3e}")
    return err, bound


# ---------------------------------------------------------------- many equal-length segments
def batch(x, c=None):
    """Vectorised exact moments of the rows of x (u32 keys below KEY_WIDE, small enough for the
    integer sums to stay below 2^63: asserted).  c: pivot per row (default: the rule's).
    Returns avg, std (f64, us, within 4 * 2^-53), z2 and the STD bound per row; rows whose
    variance is 0 get bound 0."""
    x = np.ascontiguousarray(x, np.uint32)
    nseg, n = x.shape
    mx = int(x.max())
    assert mx < KEY_WIDE and n * mx * mx < 2 ** 63
    xi = x.astype(np.int64)
    s1 = xi.sum(axis=1)
    s2 = (xi * xi).sum(axis=1)
    if c is None:
        i0, i1, i2 = pivot_index(n)
        c = np.sort(np.stack([xi[:, i0], xi[:, i1], xi[:, i2]]), axis=0)[1]
    # the products leave 64 bits: Python integers per row, each converted to f64 once
    s1o, s2o = s1.astype(object), s2.astype(object)
    vo = n * s2o - s1o * s1o                                  # n^2 sigma^2, exact
    devo = n * np.asarray(c, np.int64).astype(object) - s1o   # n (c - mean), exact
    v = np.array([float(t) for t in vo], np.float64)
    dev2 = np.array([float(t * t) for t in devo], np.float64)
    rng = xi.max(axis=1) - xi.min(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        z2 = np.where(v > 0, dev2 / v, 0.0)
    avg = s1.astype(np.float64) / (1000.0 * n)
    std = np.sqrt(v) / (1000.0 * n)
    g = np.where(rng < (1 << 24), gamma(8, U32), gamma(10, U32))
    assert int(rng.max()) < 1 << 31
    R = (g + 2.0 ** -50) * (1.0 + z2) + U32
    assert float(R.max()) < 1.0
    bound = (1.0 + R / (2.0 - R)) * (1.0 + 2.0 * U32) - 1.0
    return SimpleNamespace(n=n, s1=s1, avg=avg, std=std, z2=z2, bound=np.where(v > 0, bound, 0.0),
                           zero=v == 0)


def check_batch(got_avg, got_std, x, c=None, tag=""):
    """`check` for the rows of x (see `batch`): AVG by the rounding rule (rows whose f64 quotient
    is too close to an f32 midpoint to decide take the exact path), STD at the per-row bound."""
    b = batch(x, c)
    ga = np.asarray(got_avg, np.float32)
    gs = np.asarray(got_std, np.float32)
    want = b.avg.astype(np.float32)
    # b.avg is within 2^-52 of exact: rows where it is nowhere near a midpoint are decided
    side = np.where(want.astype(np.float64) > b.avg, -np.inf, np.inf).astype(np.float32)
    other = np.nextafter(want, side).astype(np.float64)       # the neighbour on the exact value's side
    close = np.abs(b.avg - (want.astype(np.float64) + other) / 2) <= 8 * U64 * np.abs(b.avg)
    bad = np.flatnonzero((ga.view(np.uint32) != want.view(np.uint32)) | close)
    for s in bad:
        assert avg_ok(ga[s], moments(x[s], None if c is None else int(np.asarray(c)[s]))), (tag, "avg", int(s))
    assert np.all(gs[b.zero].view(np.uint32) == 0), (tag, "std of constant segments must be +0.0")
    nz = ~b.zero
    err = np.zeros(len(gs))
    err[nz] = np.abs(gs[nz].astype(np.float64) - b.std[nz]) / b.std[nz]
    worst = int(np.argmax(err - b.bound))
    assert np.all(err <= b.bound + 4 * U64), (tag, "std", worst, float(err[worst]), float(b.bound[worst]))
    return err, b.bound
