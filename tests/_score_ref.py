"""The plain reference of the scoring half of a report (numpy / Python, no GPU), written from
reporting.py's arithmetic as csrc/scores.hip's header cites it, and the seeded inputs the
scoring and attribution tests share.

Every per-element value is one numpy operation in the stated type: rounded once, never fused.
Sums are math.fsum (the correctly rounded sum), so a kernel's sum in any order is compared to
the exact one; counts are exact.  Only `finalize` adds in a fixed order (the ABI fixes it: shards
in shard order starting from 0.0), so that one is bit for bit.

    eligible      col_valid != 0 and num > 0
    w             f64(num) * f64(avg)
    individual    h = min(hist, med) in the value type; s = f64(h) / f64(med); t = s * w
    relative      s = f64(ref[ri]) / f64(med); t = s * w, where ref[ri] >= 0 (-1 and NaN: no
                  reference) and not ref_missing[ri]
    score         sum t / sum w when n > 0, else NaN; optional float32 rounding; mask = score < thr
    error bits    1: an eligible term of a computed kind has med == 0
                  2: n > 0 and sum w == 0 (set where scores are finished)
"""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

EPS = 2.0 ** -53  # unit roundoff of float64


# ------------------------------------------------------------------ shared seeded inputs
def inputs(R, K, dt, seed, nonneg_avg=False):
    """Seeded statistics with absent kernels, filtered columns and references of every kind.
    nonneg_avg: the caller relies on avg >= 0 throughout (every weight >= 0); the draws are
    the same, the property is checked."""
    g = np.random.default_rng(seed)
    num = g.integers(0, 40, (R, K)).astype(np.int32)
    num[g.random((R, K)) < 0.1] = 0            # absent on that rank
    num[g.random((R, K)) < 0.02] = -3          # <= 0 is absent too
    med = g.uniform(1.0, 100.0, (R, K)).astype(dt)
    avg = (med * g.uniform(0.9, 1.4, (R, K))).astype(dt)
    col_valid = (g.random(K) > 0.1).astype(np.uint8)
    perm = g.permutation(K).astype(np.int32)   # ref_index: the column's id in the reference
    ref = np.empty(K, np.float32)
    ref[perm] = (np.where(num > 0, med, np.inf).min(0) * g.uniform(0.4, 1.0, K)).astype(np.float32)
    bad = g.random(K)
    ref[perm[bad < 0.06]] = -1.0
    ref[perm[(bad >= 0.06) & (bad < 0.12)]] = np.nan
    ref[~np.isfinite(ref) & ~np.isnan(ref)] = np.nan  # a column absent everywhere
    missing = (g.random(K) < 0.08).astype(np.uint32)
    stride = K + 5                              # history rows longer than K, slots permuted
    slot = g.permutation(stride)[:K].astype(np.int32)
    hist = g.uniform(0.5, 200.0, (R, stride)).astype(dt)
    hist[:, slot] = np.minimum(hist[:, slot], med)  # as the report's scores call leaves it
    if nonneg_avg:
        assert (avg >= 0).all()
    return dict(num=num, med=med, avg=avg, col_valid=col_valid, perm=perm, ref=ref, missing=missing,
                stride=stride, slot=slot, hist=hist)


def score_inputs(R, K, dt, seed):
    """`inputs` for the score tests: the history is raised again in places (a stored value above
    MED, +inf where nothing was stored yet), so the update has something to do."""
    x = inputs(R, K, dt, seed, nonneg_avg=True)
    g = np.random.default_rng(seed + 7919)
    h = x["hist"]
    up = g.random(h.shape)
    h[up < 0.3] *= dt(3.0)
    h[up > 0.9] = np.inf
    return x


def two_term_inputs():
    """The "no FMA" inputs: 256 rows, K = 2304, float64, two present kernels per row (c0, c1),
    64 rows per column pair.  Kernel c0: med 1, num 1, ref 0.5 and history 0.5, avg A an odd
    multiple of 2^-52 in [1, 1.1): t0 = A / 2 exactly, an odd multiple of 2^-53.  Kernel c1: t1 in
    [1, 1.4), one ulp 2^-52.  So round(s1 * w1) + t0 lies exactly halfway between two doubles
    below 2, and wherever s1 * w1 is inexact a fused multiply-add rounds the other way in about
    half the rows."""
    R, K = 256, 2304
    pairs = [(0, 256), (0, 1), (0, 64), (5, 2053)]
    g = np.random.default_rng(2024)
    num = np.zeros((R, K), np.int32)
    med = np.ones((R, K))
    avg = np.zeros((R, K))
    hist = np.full((R, K), np.inf)
    ref = np.full(K, -1.0, np.float32)      # one reference per column: the same for every row
    ref[[0, 5]] = 0.5
    for _, c1 in pairs:
        ref[c1] = g.uniform(10.0, 50.0)
    for r in range(R):
        c0, c1 = pairs[r // 64]
        num[r, c0] = num[r, c1] = 1
        avg[r, c0] = 1.0 + (2 * int(g.integers(0, 2 ** 47)) + 1) * 2.0 ** -52
        hist[r, c0] = 0.5
        med[r, c1] = float(ref[c1]) / g.uniform(0.8, 1.0)   # s1 = ref / med in [0.8, 1]
        hist[r, c1] = med[r, c1] * g.uniform(0.8, 1.0)      # and so is hist / med
        avg[r, c1] = g.uniform(1.25, 1.4)                   # t1 = s1 * avg in [1, 1.4]
    return dict(num=num, med=med, avg=avg, ref=ref, hist=hist, pairs=pairs)


def rounding_order_row():
    """round_f32 and the mask: the f64 score is below the threshold, its float32 rounding is not."""
    return dict(num=np.ones((1, 1), np.int32), med=np.ones((1, 1)), avg=np.ones((1, 1)),
                hist=np.full((1, 1), 0.75 - 2.0 ** -30), thr=0.75)


# ------------------------------------------------------------------ scores
def _fsum(v):
    v = np.asarray(v, np.float64)
    return math.fsum(v) if np.isfinite(v).all() else float(np.sum(v))  # inf / NaN: no order to fix


def score_terms(num, med, avg, *, col_valid=None, ref=None, ref_index=None, ref_missing=None,
                hist=None, hist_index=None, hist_stride=0):
    """Per-element terms, partials [R][6] = [sum t, sum w, n] relative then individual, bit 1 of
    the error word, and the new history (hist itself is left unchanged)."""
    R, K = med.shape
    cols = np.arange(K)
    w = num.astype(np.float64) * avg.astype(np.float64)
    m = med.astype(np.float64)
    elig = num > 0
    if col_valid is not None:
        elig = elig & (col_valid != 0)[None, :]
    out = SimpleNamespace(w=w, elig=elig, partials=np.zeros((R, 6)), zero_med=False, new_hist=None,
                          t_rel=None, t_ind=None, in_rel=None, in_ind=None)
    with np.errstate(all="ignore"):
        if ref is not None:
            ri = cols if ref_index is None else ref_index
            b = ref[ri]
            usable = b >= 0  # -1 and NaN: no reference
            if ref_missing is not None:
                usable = usable & (ref_missing[ri] == 0)
            out.in_rel = elig & usable[None, :]
            s = b.astype(np.float64)[None, :] / m
            out.t_rel = s * w
            out.zero_med |= bool((out.in_rel & (m == 0)).any())
        if hist is not None:
            hi = cols if hist_index is None else hist_index
            flat = hist.reshape(R, -1)
            assert flat.shape[1] == (hist_stride or K)
            old = flat[:, hi]
            h = np.where(med < old, med, old)  # Python's min(hist, MED), in the value type
            out.in_ind = elig
            s = h.astype(np.float64) / m
            out.t_ind = s * w
            new = flat.copy()
            rr, cc = np.nonzero(elig)
            new[rr, np.asarray(hi)[cc]] = h[rr, cc]
            out.new_hist = new.reshape(hist.shape)
            out.zero_med |= bool((elig & (m == 0)).any())
    for r in range(R):
        for base, t, take in ((0, out.t_rel, out.in_rel), (3, out.t_ind, out.in_ind)):
            if t is None:
                continue
            out.partials[r, base:base + 3] = (_fsum(t[r][take[r]]), _fsum(w[r][take[r]]),
                                              int(take[r].sum()))
    return out


def finish(partials, *, round_f32=False, thr_rel=0.75, thr_ind=0.75):
    """[R][6] partials -> (score_rel, score_ind, mask_rel, mask_ind, zero_weight)."""
    p = np.asarray(partials, np.float64)
    res = []
    zero_w = False
    for base in (0, 3):
        sw, w, n = p[:, base], p[:, base + 1], p[:, base + 2]
        with np.errstate(all="ignore"):
            s = np.where(n > 0, sw / w, np.nan)
        zero_w |= bool(((n > 0) & (w == 0)).any())
        if round_f32:
            s = s.astype(np.float32).astype(np.float64)
        res.append(s)
    with np.errstate(invalid="ignore"):
        return res[0], res[1], res[0] < thr_rel, res[1] < thr_ind, zero_w


def finalize(partials, nshards, **kw):
    """[nshards][R][6] -> finish() of the shards added in shard order starting from 0.0."""
    q = np.asarray(partials, np.float64).reshape(nshards, -1, 6)
    p = np.zeros(q.shape[1:])
    for g in range(nshards):
        p = p + q[g]
    return finish(p, **kw)


def sum_bound(n, exact):
    """|sum in any order - exact sum| for n non-negative float64 terms: n * 2^-53 * sum."""
    return n * EPS * exact


def score_rel_bound(n):
    """Relative error of (sum t) / (sum w) against the exact sums' quotient: (2n + 2) * 2^-53."""
    return (2 * n + 2) * EPS


def stragglers(score, thr):
    with np.errstate(invalid="ignore"):
        return np.asarray(score, np.float64) < thr


# ------------------------------------------------------------------ column reference
def kernel_ref(num, med):
    """(ref, minbits, missing): the min over rows with num > 0 of the float32 MED bit pattern
    (starting from +inf's), NaN where a row has num <= 0 or R == 0."""
    R, K = med.shape
    med = np.ascontiguousarray(med, np.float32)
    present = num > 0
    bits = np.where(present, med.view(np.uint32), np.uint32(0x7F800000))
    minbits = np.minimum(bits.min(0, initial=0x7F800000), np.uint32(0x7F800000)).astype(np.uint32)
    missing = (~present).any(0).astype(np.uint32)
    ref = minbits.view(np.float32).copy()
    ref[(missing != 0) | (R == 0)] = np.nan
    return ref, minbits, missing


def pack_min_times(med, ids, total):
    out = np.full(total, -1.0, np.float32)
    out[ids] = med.astype(np.float32)  # round to nearest even
    return out


# ------------------------------------------------------------------ sections
def section_scores(med, present, *, ref_in=None, ref_index=None, hist=None, round_f32=False,
                   rel=True, ind=True):
    """(rel [R][S], ind [R][S], new history, bit 1): elementwise float64, no sums."""
    R, S = med.shape
    pres = present != 0
    out_rel = out_ind = new_hist = None
    with np.errstate(all="ignore"):
        if rel:
            if ref_in is None:  # min over ranks of the float32 MED if every rank has it
                m32 = np.where(pres, med.astype(np.float32), np.float32(np.inf))
                r32 = np.where(pres.all(0) & (R > 0), m32.min(0, initial=np.inf), np.nan)
                r32 = r32.astype(np.float32)
            else:
                r32 = ref_in[np.arange(S) if ref_index is None else ref_index]
            rd = np.where(r32 >= 0, r32.astype(np.float64), np.nan)  # -1 => NaN
            out_rel = np.where(pres, rd[None, :] / med, np.nan)
        if ind:
            h = np.where(med < hist, med, hist)
            new_hist = np.where(pres, h, hist)
            out_ind = np.where(pres, h / med, np.nan)
        if round_f32:
            out_rel = None if out_rel is None else out_rel.astype(np.float32).astype(np.float64)
            out_ind = None if out_ind is None else out_ind.astype(np.float32).astype(np.float64)
    zero = bool((rel or ind) and (pres & (med == 0)).any())
    return out_rel, out_ind, new_hist, zero


def section_stats(values):
    """dict(num, min, max, med, avg, std) of one section: sorted values, the lower median
    s[(n - 1) // 2], mean = fsum / n, unbiased standard deviation from exact rationals."""
    v = np.sort(np.asarray(values, np.float64))
    n = len(v)
    nan = float("nan")
    if n == 0:
        return dict(num=0, min=nan, max=nan, med=nan, avg=nan, std=nan)
    std = nan
    if n > 1:
        ratios = [float(x).as_integer_ratio() for x in v]
        Q = max(q for _, q in ratios)          # denominators are powers of two
        xs = [p * (Q // q) for p, q in ratios]
        s1, s2 = sum(xs), sum(x * x for x in xs)
        var = Fraction(n * s2 - s1 * s1, n * (n - 1) * Q * Q)  # exact sum (x - mean)^2 / (n - 1)
        std = math.sqrt(var)
    return dict(num=n, min=float(v[0]), max=float(v[-1]), med=float(v[(n - 1) // 2]),
                avg=math.fsum(v) / n, std=std)


WELL_CONDITIONED = ("uniform", "equal", "two", "sorted", "reverse", "ties_outlier", "negative",
                    "zeros")
ABSOLUTE_BOUND = ("cluster", "mixed")  # mean far from the spread, or cancelling signs


def section_patterns(n, seed):
    """name -> n float64 section timings of one value pattern."""
    g = np.random.default_rng(seed)
    u = g.random(n) * 10
    ties = np.full(n, 2.5)
    ties[-1] = 1e4
    zeros = np.zeros(n)
    zeros[::2] = -0.0
    zeros[n // 2] = 3.0  # MIN, MAX and MED compare by value: -0.0 == 0.0
    return dict(uniform=u, equal=np.full(n, 7.25), two=g.choice([1.5, 4.0], n), sorted=np.sort(u),
                reverse=np.sort(u)[::-1].copy(), ties_outlier=ties, negative=-u - 1.0,
                zeros=zeros, cluster=1e6 + g.random(n) * 1e-3, mixed=g.uniform(-10, 10, n))


# ------------------------------------------------------------------ comparisons
def same_bits(got, want):
    """Equal bit for bit, any NaN matching any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got[~nan].view(u), want[~nan].view(u)))
