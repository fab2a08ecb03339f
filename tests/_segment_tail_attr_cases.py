"""The cases of the segment tail-attribution tests (CPU twin and GPU kernels): every case of
``_segment_tail_cases`` unchanged (top 16), plus cases laid out with its ``layout`` for what those
do not reach in segment_tail_attribution.hip -- the select kernel's second batch of loads
(K > 2,048), a winner longer than one wave trip of 256 * 4 samples, rows with only negative
losses, exactly ``top`` / ``top - 1`` / fewer elements taken, two columns whose losses tie at a
non-zero value, a column present in one row only, and every instantiation of ``top``.  ``planted``
states where a case's aim must show: {(row, position): column} of the twin's ``idx``.  Built once
per process and never written to; the twin's result per case is computed once and shared."""
import functools
from collections import namedtuple

import numpy as np

import _segment_tail_cases as S
from nvidia_resiliency_ext.straggler import histograms

AttrCase = namedtuple("AttrCase", "name seg top planted")


def _slow_tail(base, n, slow):
    """n durations of exactly `base`, the last `slow` of them 8x as long: no noise, so the loss
    of the element is known to grow with base * slow."""
    x = np.full(n, base, np.uint32)
    if slow:
        x[n - slow:] = 8 * base
    return x


def _k2100():
    """R 2, K 2,100, lengths mostly 0..3.  Row 0's winners, largest first, sit in columns 2099,
    0, 256, 2050, 255 (the second batch of the select kernel's loads, and both sides of the first
    256-column boundary); row 1's single planted winner in column 2070."""
    R, K = 2, 2100
    rng = np.random.default_rng(50)
    lens = rng.choice([0, 0, 1, 2, 3], R * K)
    row0 = {2099: 5_000_000, 0: 4_000_000, 256: 3_000_000, 2050: 2_000_000, 255: 1_000_000}
    for k in row0:
        lens[k], lens[K + k] = 40, 60          # 4 of 100 samples slow: the fleet's T stays in the body
    lens[2070], lens[K + 2070] = 60, 40

    def fill(rng, g, n):
        r, k = divmod(g, K)
        if k in row0:
            return _slow_tail(row0[k], n, 4 if r == 0 else 0)
        if k == 2070:
            return _slow_tail(500_000, n, 4 if r == 1 else 0)
        return S.durations(rng, n, 2_000)      # a 6x slow call costs 10 us: far below the planted

    planted = {(0, j): k for j, k in enumerate(row0)}
    planted[(1, 0)] = 2070
    return AttrCase("K2100_second_batch", S.layout("K2100_second_batch", R, K, lens, fill, pm=950, seed=50),
                    8, planted)


def _long_winner(cap, top):
    """(0, 1) holds 4,100 samples, the last 100 of them 8x slow: four wave trips and a partial
    one (three with cap 3,000, which keeps the slow calls)."""
    lens = [5, 4100, 300, 7, 2000, 16]

    def fill(rng, g, n):
        if g == 1:
            x = S.durations(rng, n, 20_000)
            x[n - 100:] = 160_000
            return x
        return S.durations(rng, n, 20_000 if g == 4 else 2_000)

    name = f"long_winner_cap{cap}"
    return AttrCase(name, S.layout(name, 2, 3, lens, fill, cap=cap, pm=950, seed=51), top, {(0, 0): 1})


def _only_negative():
    """Row 0 has no sample above any T while the fleet has: every loss of the row is negative.
    K 4 with top 5: the fifth slot is a pad."""
    base = [30_000, 50_000, 70_000, 90_000]

    def fill(rng, g, n):
        r, k = divmod(g, 4)
        return _slow_tail(base[k], n, r)       # row 1: one slow call in 20, 39 of 40 in the body

    return AttrCase("only_negative_losses", S.layout("only_negative_losses", 2, 4, [20] * 8, fill,
                                                    pm=950, seed=52), 5, {})


def _exactly_top():
    """Row 0 has exactly top = 9 columns with samples, row 1 top - 1 = 8."""
    K = 12
    lens = np.zeros(2 * K, np.int32)
    lens[[0, 1, 3, 4, 6, 7, 9, 10, 11]] = [3, 17, 1, 40, 16, 2, 5, 300, 9]
    lens[K + np.array([0, 2, 3, 5, 6, 8, 9, 11])] = [4, 1, 18, 2, 64, 7, 3, 12]
    return AttrCase("exactly_top_and_one_less", S.layout("exactly_top_and_one_less", 2, K, lens,
                                                        lambda rng, g, n: S.durations(rng, n, 9_000 * (1 + g % K)),
                                                        pm=900, seed=53), 9, {})


def _few_taken():
    """Three and one column taken under top 16."""
    lens = [6, 0, 20, 0, 2, 0, 0, 0, 9, 0]
    return AttrCase("fewer_than_top16", S.layout("fewer_than_top16", 2, 5, lens,
                                                lambda rng, g, n: S.durations(rng, n, 40_000),
                                                pm=900, seed=54), 16, {})


def _duplicated_columns():
    """Columns 2 and 4 hold the same samples in every row, so their losses tie exactly; row 0's
    are the largest of the row and not zero: the lower column comes first."""
    R, K = 3, 6
    rng = np.random.default_rng(55)
    twin_data = [S.durations(rng, 30, 900_000) for _ in range(R)]
    twin_data[0][-3:] = 7_200_000
    lens = [30 if k in (2, 4) else (4, 17, 9, 0)[(r + k) % 4] for r in range(R) for k in range(K)]

    def fill(rng, g, n):
        r, k = divmod(g, K)
        return twin_data[r] if k in (2, 4) else S.durations(rng, n, 3_000)

    return AttrCase("duplicated_columns", S.layout("duplicated_columns", R, K, lens, fill, pm=950,
                                                  seed=55), 4, {(0, 0): 2, (0, 1): 4})


def _one_row_column():
    """Column 2 has samples in row 1 only: taken there, absent in rows 0 and 2."""
    lens = [5, 20, 0, 3, 8, 2, 25, 17, 1, 40, 0, 6]
    return AttrCase("column_in_one_row", S.layout("column_in_one_row", 3, 4, lens,
                                                 lambda rng, g, n: S.durations(rng, n, 60_000),
                                                 pm=900, seed=56), 1, {})


@functools.lru_cache(maxsize=None)
def cases():
    out = [AttrCase(c.name, c, 16, {}) for c in S.cases()]
    out += [_k2100(), _long_winner(0, 3), _long_winner(3000, 4), _only_negative(), _exactly_top(),
            _few_taken(), _duplicated_columns(), _one_row_column()]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def twin(name):
    """``histograms.segment_tail_attribution`` of a case: computed once, never written to."""
    c = case(name)
    s = c.seg
    res = histograms.segment_tail_attribution(s.keys, s.off, s.lens, s.K, s.pm, c.top, s.cap,
                                              s.col_valid, s.thr_index)
    for f in vars(res).values():
        f.setflags(write=False)
    return res
