"""The cases of the tests of nvrx_histogram_history_attribution_compact (CPU twin and GPU kernels):
every case of ``_histogram_compact_cases.cases()`` (read only), ``top`` cycling through 1, 4, 8,
16, and behind them what that table lacks for an attribution -- an element that has a history and
samples but whose history weighs nothing (bucket 0 alone: ``btotal == 0``, the share 0 / 0, a NaN
loss that is left out).  ``skip_rows`` of a case belongs to the score's update and is not used.

``twin`` (the compact host twin) and ``oracle`` (the dense host twin on the expansion) are computed
once per case and never written to."""
import functools

import numpy as np

import _histogram_compact_cases as HC
from nvidia_resiliency_ext.straggler import histograms

BINS = HC.BINS
TOPS = (1, 4, 8, 16)
FIELDS = ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share", "loss_all")


def _weightless_history():
    """R = 2, K = 6.  Column 1: the history holds bucket 0 alone (weight 0), the interval has
    samples: eligible, btotal == 0, NaN, left out.  Column 4: the same history, the interval in
    bucket 0 alone: total == 0 as well.  The other columns are ordinary, so the row still has
    winners, fewer than ``top`` = 8."""
    R, K = 2, 6
    counts = np.zeros((R, K, BINS), np.uint32)
    chist = np.zeros((R, K, HC.CB), np.uint8)
    for r in range(R):
        for k in range(K):
            if k in (1, 4):
                chist[r, k] = HC.element({0: 9 + r})
                counts[r, k] = HC.dense({0: 3} if k == 4 else {0: 1, 5: 2, 90: 1 + r})
            else:
                b = 30 + 7 * k
                chist[r, k] = HC.element({b: 50, b + 1: 20, b + 9: 2})
                counts[r, k] = HC.dense({b: 10, b + 1: 3 + r, b + 9: 1 + k})
    counts.setflags(write=False)
    chist.setflags(write=False)
    return HC.HCase("weightless_history", R, K, counts, chist, 950, None, None, 0, None)


@functools.lru_cache(maxsize=None)
def cases():
    out = HC.cases() + (_weightless_history(),)
    assert len({c.name for c in out}) == len(out)
    return out


def table_size():
    return len(HC.cases())


def top_of(name):
    return TOPS[[c.name for c in cases()].index(name) % len(TOPS)]


def case(name):
    return next(c for c in cases() if c.name == name)


def attr_kwargs(c):
    return dict(hist_index=c.hist_index, col_valid=c.col_valid)


def dense_of(c, chist=None):
    """The dense expansion (u32 [R, S, 240]) of the slots a case uses; the others (sentinels, which
    no call may look at) expand to zeros."""
    chist = c.chist0 if chist is None else chist
    used = HC.used_slots(c)
    d = np.zeros(chist.shape[:2] + (BINS,), np.uint32)
    d[:, used] = histograms.compact_to_dense(chist[:, used])
    return d


def _frozen(res):
    for f in vars(res).values():
        f.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def twin(name):
    c = case(name)
    return _frozen(histograms.compact_history_attribution(c.counts, c.chist0, c.pm, top_of(name),
                                                          **attr_kwargs(c)))


@functools.lru_cache(maxsize=None)
def oracle(name):
    c = case(name)
    return _frozen(histograms.history_attribution(c.counts, dense_of(c), c.pm, top_of(name),
                                                  **attr_kwargs(c)))


def base_total(c, r, k):
    """btotal of element (r, k), or None where the element has no slot or is not valid."""
    s = k if c.hist_index is None else int(c.hist_index[k])
    if s < 0 or (c.col_valid is not None and not c.col_valid[k]):
        return None
    count, bucket, _ = histograms._chist_fields(c.chist0[r:r + 1, s:s + 1])
    w = histograms.weights()
    return sum(int(v) * int(w[b]) for v, b in zip(count[0, 0], bucket[0, 0]))
