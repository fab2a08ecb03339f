"""GPU: ops.section_stats and ops.section_scores against the plain reference of
tests/_score_ref.py.

section_stats: NUM, MIN, MAX and the lower median are exact.  AVG and STD are held to the
project's own bars for these kernels (rel 1e-14 and rel 1e-12, test_gpu_detector.py) on the
well-conditioned value patterns.  For the tight cluster and the mixed-sign pattern a relative bar
means nothing (the spread is tiny against the values, or the mean cancels), so the bounds are the
absolute ones of a float64 sum of n values:
    |avg - ref| <= n * 2^-53 * max|x|
    |std - ref| <= 4 * n * 2^-53 * max|x|
A mean off by d moves the sum of squared deviations by n * d^2, so it moves the standard
deviation by at most about |d| <= n * 2^-53 * max|x|; summing the n squares adds a relative
n * 2^-53 to the variance, half of that to its root, and the root is below 2 * max|x|: together
under 4 * n * 2^-53 * max|x|.

section_scores: elementwise float64 operations with no sums, so every output and history
element is bit for bit."""
import time

import numpy as np
import pytest
import torch

import _score_ref as R
from nvidia_resiliency_ext.straggler import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stats(secs, max_len):
    off = np.zeros(len(secs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in secs])
    vals = np.concatenate(secs) if off[-1] else np.zeros(1)
    num, out = ops.section_stats(dev(vals), dev(off), max_len)
    return num.cpu().numpy(), out.cpu().numpy()


def check_section(v, num, out, i, absolute=False, tag=None):
    want = R.section_stats(v)
    n = len(v)
    assert num[i] == n, tag
    mn, mx, med, avg, std = out[:, i]
    if n == 0:
        assert np.isnan(out[:, i]).all(), tag
        return
    assert mn == want["min"] and mx == want["max"] and med == want["med"], tag  # by value
    if absolute:
        amax = np.abs(v).max()
        assert abs(avg - want["avg"]) <= n * R.EPS * amax, tag
        assert n == 1 or abs(std - want["std"]) <= 4 * n * R.EPS * amax, tag
    else:
        assert avg == pytest.approx(want["avg"], rel=1e-14), tag
        assert n == 1 or std == pytest.approx(want["std"], rel=1e-12), tag
    assert n > 1 or np.isnan(std), tag


# every template boundary, grouped so max_len selects each code path; the kernel is chosen by
# max_len, the padding by each section's own n
GROUPS = {
    "lds1024": ([1, 2, 3, 255, 256, 257, 1023, 1024, 0], 1024),
    "lds8192": ([1025, 8191, 0, 8192, 5], 8192),
    "lds16384": ([8193, 16383, 16384, 3], 16384),
    "global": ([16385, 32768, 0, 32769, 2, 1025], 32769),
    "short_in_lds16384": ([1, 2, 3, 255, 0, 257, 1000], 16384),
    "short_in_global": ([1, 2, 3, 255, 0, 257, 1000], 40000),
}


@pytest.mark.parametrize("group", list(GROUPS))
def test_section_stats_lengths(group):
    lengths, max_len = GROUPS[group]
    g = np.random.default_rng(len(group))
    secs = [g.random(n) * 10 for n in lengths]
    num, out = stats(secs, max_len)
    assert num.dtype == np.int32
    for i, v in enumerate(secs):
        check_section(v, num, out, i, tag=(group, len(v)))


@pytest.mark.parametrize("n", [5, 1000, 8193, 16385])
def test_section_stats_value_patterns(n):
    pats = R.section_patterns(n, seed=n)
    assert set(pats) == set(R.WELL_CONDITIONED) | set(R.ABSOLUTE_BOUND)
    names = list(pats)
    num, out = stats([pats[k] for k in names], n)
    for i, k in enumerate(names):
        check_section(pats[k], num, out, i, absolute=k in R.ABSOLUTE_BOUND, tag=(k, n))
    z = names.index("zeros")
    assert out[0, z] == 0.0 and out[1, z] == 3.0 and out[2, z] == 0.0  # -0.0 among zeros


def test_section_stats_second_chunk_of_the_scratch_path():
    """max_len 16385 -> 32768 doubles of scratch per section -> 1024 sections per 256 MiB chunk:
    sections 1024..1029 go through a second launch at off + c0 / num + c0."""
    g = np.random.default_rng(1030)
    lengths = g.integers(0, 41, 1030)
    lengths[1027] = 16385
    secs = [g.random(int(n)) * 10 for n in lengths]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    num, out = stats(secs, 16385)
    print(f"chunked scratch call: {time.perf_counter() - t0:.3f} s")
    assert np.array_equal(num, lengths)
    for i, v in enumerate(secs):
        check_section(v, num, out, i, tag=i)


# ------------------------------------------------------------------ section_scores
def _sections(rows, S, seed, zero_med):
    g = np.random.default_rng(seed)
    med = g.uniform(0.5, 50.0, (rows, S))
    present = (g.random((rows, S)) < 0.8).astype(np.uint8)
    if S >= 3:
        present[:, 0] = 1                    # present everywhere
        present[:, 1] = 1
        present[g.integers(0, rows), 1] = 0  # absent on one rank
        present[:, 2] = 0                    # absent on all ranks
    kind = g.integers(0, 3, (rows, S))       # history: +inf, above MED, below MED
    hist = np.where(kind == 0, np.inf, np.where(kind == 1, med * 1.5, med * 0.5))
    if zero_med:
        r, s = int(g.integers(0, rows)), 0
        med[r, s], present[r, s] = 0.0, 1
    ref_in = g.uniform(0.1, 60.0, S).astype(np.float32)
    bad = g.random(S)
    ref_in[bad < 0.2] = -1.0
    ref_in[bad > 0.85] = np.nan
    if S >= 5:
        ref_in[:4] = (3.0, -1.0, np.nan, 0.0)
    return med, present, hist, ref_in, g.permutation(S).astype(np.int32)


@pytest.mark.parametrize("zero_med", [False, True])
@pytest.mark.parametrize("rows,S", [(1, 1), (1, 5), (3, 300), (70, 7)])
def test_section_scores_bit_exact(rows, S, zero_med):
    med, present, hist, ref_in, perm = _sections(rows, S, 100 * rows + S, zero_med)
    if zero_med:
        assert (present.astype(bool) & (med == 0)).any()
    for given in (False, True):
        ref_kw = dict(ref_in=ref_in, ref_index=perm) if given else {}
        for rel, ind in ((True, False), (False, True), (True, True)):
            for round_f32 in (False, True):
                wr, wi, wh, zero = R.section_scores(med, present, hist=hist, round_f32=round_f32,
                                                    rel=rel, ind=ind, **ref_kw)
                d_hist = dev(hist)
                err = torch.full((1,), 4, dtype=torch.int32, device=DEV)
                gr, gi = ops.section_scores(dev(med), dev(present), hist=d_hist, round_f32=round_f32,
                                            rel=rel, ind=ind, err=err,
                                            **{k: dev(v) for k, v in ref_kw.items()})
                tag = (given, rel, ind, round_f32)
                assert (gr is None) == (not rel) and (gi is None) == (not ind), tag
                if rel:
                    assert R.same_bits(gr.cpu().numpy(), wr), tag
                if ind:
                    assert R.same_bits(gi.cpu().numpy(), wi), tag
                # absent sections and a call without the individual kind leave the history alone
                assert R.same_bits(d_hist.cpu().numpy(), wh if ind else hist), tag
                assert zero == zero_med
                assert int(err.item()) == (4 | 1 if zero_med else 4), tag
