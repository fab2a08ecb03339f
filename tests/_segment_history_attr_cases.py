"""The cases of the segment history-attribution tests (CPU twin and GPU kernels): every ``HCase`` of
``_segment_history_cases`` unchanged, attributed on every interval against the history before that
interval (``walk()``), with ``top`` cycling through 1, 2, 4, 16, 5, 8, 9 -- plus cases built with
its ``make`` for the boundaries of segment_history_attribution.hip itself: a winner order that is
not the order of ``tail_calls``, exact ties in loss (a row of zeros among them), fewer elements
taken than ``top``, a row with none, a history wholly in bucket 0 (NaN loss, left out) whose tail
would rank first, negative losses below positive ones, K = 2,049 and K = 4,100 (the select kernel's
second and third batch of loads, a split of one element), winners with a retained run of 1, 64, 65,
256, 257 samples and a trimmed one.  ``planted`` states where a case's aim must show: {(interval,
row, position): column} of the twin's ``idx``.  Built once per process and never written to; the
twin's result per case and interval is computed once and shared."""
import functools
from collections import namedtuple

import numpy as np

import _segment_history_cases as H
import _segment_tail_cases as ST
from nvidia_resiliency_ext.straggler import histograms

BINS = 240
TOPS = (1, 2, 4, 16, 5, 8, 9)
WINNER_LENGTHS = (1, 64, 65, 256, 257)

AttrCase = namedtuple("AttrCase", "name h top planted")


def _counts_of(x):
    return np.bincount(histograms.bucket_of(np.asarray(x, np.uint32)), minlength=BINS).astype(np.uint32)


def _hist0(R, K, sampler):
    """hist0[r][k] = the histogram of sampler(r, k) (None: no history)."""
    h = np.zeros((R, K, BINS), np.uint32)
    for r in range(R):
        for k in range(K):
            x = sampler(r, k)
            if x is not None:
                h[r, k] = _counts_of(x)
    return h


def _slow_tail(base, n, slow):
    """n durations of exactly `base`, the last `slow` of them 8x as long."""
    x = np.full(n, base, np.uint32)
    if slow:
        x[n - slow:] = 8 * base
    return x


def _count_is_not_cost():
    """Kernel 0 is cheap, jittery and called 2,048 times; kernel 2 costs 2 ms and row 1 runs it 2x
    slower on every 16th call: by tail calls kernel 0 leads row 1, by excess tail time kernel 2."""
    R, K = 2, 4
    bases, calls, jitter = [5_000, 200_000, 2_000_000, 200_000], [2048, 128, 64, 128], [.10, .02, .02, .02]

    def draw(rng, k, slow):
        d = bases[k] * (1.0 + jitter[k] * rng.standard_normal(calls[k]))
        if slow:
            d[::16] *= 2
        return d.astype(np.uint32)

    hr = np.random.default_rng(60)
    h0 = _hist0(R, K, lambda r, k: draw(hr, k, False))

    def fill(rng, g, n):
        r, k = divmod(g, K)
        return draw(rng, k, r == 1 and k == 2)

    lens = [calls * R] * 2
    return AttrCase("count_is_not_cost", H.make("count_is_not_cost", R, K, lens, fill, pm=950, hist0=h0,
                                                seed=60), 2, {(0, 1, 0): 2, (1, 1, 0): 2})


def _ties():
    """Row 0: every history and every sample of a column in one bucket -- every loss is +0.0, the
    winners are columns 0..3.  Row 1: columns 2 and 4 hold the same history and the same samples,
    the largest loss of the row and not zero: the lower column first."""
    R, K = 3, 6
    rng = np.random.default_rng(61)
    pair_hist = ST.durations(rng, 200, 900_000)
    pair = []
    for _ in range(2):
        x = ST.durations(rng, 30, 900_000)
        x[-3:] = 7_200_000
        pair.append(x)

    def sampler(r, k):
        if r == 0:
            return np.full(50, 1_000 * (k + 1), np.uint32)
        if r == 1 and k in (2, 4):
            return pair_hist
        return ST.durations(rng, 100, 3_000 * (k + 1))

    def fill(i):
        def f(rng, g, n):
            r, k = divmod(g, K)
            if r == 0:
                return np.full(n, 1_000 * (k + 1), np.uint32)
            if r == 1 and k in (2, 4):
                return pair[i]
            return ST.durations(rng, n, 3_000 * (k + 1))
        return f

    lens = [[7, 20, 64, 3, 1, 9] + [30 if k in (2, 4) else (4, 17, 9)[k % 3] for k in range(K)] +
            [5, 0, 12, 40, 2, 8]] * 2
    planted = {(i, 0, j): j for i in range(2) for j in range(4)}
    planted.update({(0, 1, 0): 2, (0, 1, 1): 4, (1, 1, 0): 2, (1, 1, 1): 4})
    return AttrCase("ties", H.make("ties", R, K, lens, [fill(0), fill(1)], pm=950,
                                   hist0=_hist0(R, K, sampler), seed=61), 4, planted)


def _few_and_none():
    """Under top 16: row 0 has three columns with a history, row 1 neither history nor (at first)
    samples -- none taken in either interval --, row 2 three columns with samples."""
    R, K = 3, 5
    rng = np.random.default_rng(62)
    h0 = _hist0(R, K, lambda r, k: ST.durations(rng, 80, 40_000) if r == 2 or (r == 0 and k % 2 == 0) else None)
    lens = [[6] * 5 + [0] * 5 + [5, 0, 7, 0, 9], [6, 3, 70, 1, 2] + [4, 9, 1, 17, 2] + [5, 2, 7, 0, 9]]
    return AttrCase("few_and_none", H.make("few_and_none", R, K, lens,
                                           lambda rng, g, n: ST.durations(rng, n, 40_000), pm=900,
                                           hist0=h0, seed=62), 16, {})


def _bucket0_history():
    """(0, 1): a history of 100 samples wholly in bucket 0 (weight 0: btotal == 0, a NaN loss) under
    the costliest samples of the row: left out, although its tail would rank first."""
    R, K = 2, 5
    rng = np.random.default_rng(63)
    h0 = _hist0(R, K, lambda r, k: np.zeros(100, np.uint32) if (r, k) == (0, 1)
                else ST.durations(rng, 100, 20_000))

    def fill(rng, g, n):
        return np.full(n, 100_000_000, np.uint32) if g == 1 else ST.durations(rng, n, 20_000)

    return AttrCase("bucket0_history", H.make("bucket0_history", R, K, [[20] * (R * K)] * 2, fill, pm=950,
                                              hist0=h0, seed=63), 5, {})


def _negative_below_positive():
    """Columns 0..2: a history with a fifth of its samples 8x slow and an interval without a slow
    call -- negative losses; columns 3..5: a clean history and 4 slow calls -- positive ones."""
    R, K = 2, 6
    base = [30_000, 50_000, 70_000, 90_000, 110_000, 130_000]
    h0 = _hist0(R, K, lambda r, k: _slow_tail(base[k], 100, 20 if k < 3 else 0))

    def fill(rng, g, n):
        k = g % K
        return _slow_tail(base[k], n, 0 if k < 3 else 4)

    return AttrCase("negative_below_positive",
                    H.make("negative_below_positive", R, K, [[40] * (R * K)] * 2, fill, pm=700, hist0=h0,
                           seed=64), 8, {})


def _wide(name, R, K, top, winners, seed):
    """R x K with lengths mostly 0..3 over a one-bucket history; ``winners`` {(row, column): base}
    hold 40 samples of `base`, 4 of them 8x slow over a history at `base`: by loss they lead their
    row in the order of their bases."""
    rng = np.random.default_rng(seed)
    lens = rng.choice([0, 0, 1, 2, 3], R * K)
    h0 = np.zeros((R, K, BINS), np.uint32)
    h0[:, :, H.bucket(2_000)] = 100
    for (r, k), b in winners.items():
        lens[r * K + k] = 40
        h0[r, k] = 0
        h0[r, k, H.bucket(b)] = 100

    def fill(rng, g, n):
        b = winners.get(divmod(g, K))
        return _slow_tail(b, n, 4) if b else ST.durations(rng, n, 2_000)

    planted = {}
    for r in range(R):
        mine = sorted(((b, k) for (rr, k), b in winners.items() if rr == r), reverse=True)
        planted.update({(0, r, j): k for j, (_, k) in enumerate(mine)})
    return AttrCase(name, H.make(name, R, K, [lens, lens], fill, pm=950, hist0=h0, seed=seed), top, planted)


def _winner_lengths():
    """Every column is a winner (top 8 over K 6): retained runs of 1, 64, 65, 256, 257 and 1,025."""
    K = 6
    lens = list(WINNER_LENGTHS) + [1025]
    h0 = _hist0(1, K, lambda r, k: np.full(100, 10_000 * (k + 1), np.uint32))
    return AttrCase("winner_lengths",
                    H.make("winner_lengths", 1, K, [lens, lens[1:] + lens[:1]],
                           lambda rng, g, n: ST.durations(rng, n, 10_000 * (g % K + 1)), pm=950, hist0=h0,
                           seed=67), 8, {})


def _winner_cap_trimmed():
    """(0, 0) holds 250 samples under cap 100: the 150 trimmed ones are all slow, of the retained
    100 the last 10 are."""
    h0 = _hist0(1, 3, lambda r, k: np.full(100, 1_000_000 if k == 0 else 5_000, np.uint32))

    def fill(rng, g, n):
        if g != 0:
            return ST.durations(rng, n, 5_000)
        x = np.full(n, 8_000_000, np.uint32)
        x[n - 100:n - 10] = 1_000_000
        return x

    return AttrCase("winner_cap_trimmed",
                    H.make("winner_cap_trimmed", 1, 3, [[250, 7, 100]] * 2, fill, cap=100, pm=950, hist0=h0,
                           seed=68), 1, {(0, 0, 0): 0, (1, 0, 0): 0})


@functools.lru_cache(maxsize=None)
def cases():
    out = [AttrCase(c.name, c, TOPS[i % len(TOPS)], {}) for i, c in enumerate(H.cases())]
    out += [_count_is_not_cost(), _ties(), _few_and_none(), _bucket0_history(), _negative_below_positive(),
            _wide("K2049", 1, 2049, 8, {(0, 2048): 5_000_000, (0, 0): 4_000_000, (0, 2047): 3_000_000,
                                        (0, 256): 2_000_000}, 65),
            _wide("K4100", 2, 4100, 9, {(0, 4099): 5_000_000, (0, 4096): 4_000_000, (0, 2048): 3_000_000,
                                        (0, 5): 2_000_000, (1, 4097): 5_000_000}, 66),
            _winner_lengths(), _winner_cap_trimmed()]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def attr_kwargs(h):
    return dict(hist_index=h.hist_index, col_valid=h.col_valid)


@functools.lru_cache(maxsize=None)
def walk(name):
    """Per interval of a case (counts of the retained windows, the history before, the twin's score
    result): ``_segment_history_cases.walk`` for its own cases, the same walk for the added ones."""
    h = case(name).h
    if any(c.name == name for c in H.cases()):
        return H.walk(name)
    hist, out = h.hist0, []
    for iv in h.intervals:
        counts = histograms.segment_counts(iv.keys, iv.off, iv.lens, h.K, iv.cap)
        res = histograms.history_scores(counts, hist, h.pm, score_thr=0.9, **H.history_kwargs(h))
        out.append((counts, hist, res))
        hist = res.hist
    return tuple(out)


@functools.lru_cache(maxsize=None)
def twin(name):
    """``histograms.segment_history_attribution`` of every interval of a case against the history
    before it: computed once, never written to."""
    c = case(name)
    h = c.h
    out = []
    for iv, (_, before, _) in zip(h.intervals, walk(name)):
        res = histograms.segment_history_attribution(iv.keys, iv.off, iv.lens, h.K, before, h.pm, c.top,
                                                     iv.cap, **attr_kwargs(h))
        for f in vars(res).values():
            f.setflags(write=False)
        out.append(res)
    return tuple(out)


def retained(iv, g):
    n = int(iv.lens[g])
    return 0 if n <= 0 else (min(n, iv.cap) if iv.cap else n)
