"""The cases of the compact-history attribution tests (CPU twin and GPU kernels).  Three sets share
one shape (``XCase``: per step an interval of ragged segments and the compact history it is
attributed against):

* ``hist/...``: every case and interval of ``_compact_history_cases.cases()`` against ``walk``'s
  history before that interval, ``top`` cycling through 1, 2, 4, 16, 5, 8, 9: full 12-entry
  elements, sentinel slots, hist_index, stride, col_valid, the edge buckets, the sample trips, cap.
* ``attr/...``: every ``AttrCase`` of ``_segment_history_attr_cases``, the dense history before
  each interval (``hist0`` first) passed through ``histograms.compact_from_dense``; whatever that
  yields is the history: ties, a row of zeros, fewer than ``top`` taken, an empty row, the
  bucket-0-only history, negative losses, K = 2,049 and 4,100, the winner lengths.
* ``new/...``: small cases (R <= 3, K <= 17) for what is new in
  segment_history_compact_attribution.hip: T in the first and in the twelfth entry of a full
  element, a rank exactly on an entry boundary, N past 2^32, K = 1, 3, 5, 17 (the trailing rows of
  a four-element load past K), the four rows of one load holding {eligible, empty history, empty
  segment, col_valid 0} in all four rotations, a reversed hist_index with a -1 under a stride above
  K.  The builder asserts that each aim shows in the twin's result.

The imported case modules are read only.  ``twin`` (the compact host twin) and ``oracle`` (the
dense host twin on the expansion) are computed once per case and never written to."""
import functools
from collections import namedtuple

import numpy as np

import _compact_history_cases as CH
import _segment_history_attr_cases as AC
import _segment_history_cases as H
from nvidia_resiliency_ext.straggler import histograms

BINS = 240
E = histograms.CHIST_ENTRIES
CB = histograms.CHIST_BYTES
TOPS = AC.TOPS
assert TOPS == (1, 2, 4, 16, 5, 8, 9)

XCase = namedtuple("XCase", "name R K pm top hist_index stride col_valid steps planted")
Step = namedtuple("Step", "iv chist")


def used_slots(c):
    """The history slots some column of a case uses (with or without col_valid)."""
    index = range(c.K) if c.hist_index is None else [int(s) for s in c.hist_index]
    return sorted({s for s in index if s >= 0})


def dense_of(c, chist):
    """The dense expansion (u32 [R, S, 240]) of the slots a case uses; the others (sentinels, which
    no call may look at) expand to zeros."""
    used = used_slots(c)
    d = np.zeros(chist.shape[:2] + (BINS,), np.uint32)
    d[:, used] = histograms.compact_to_dense(chist[:, used])
    return d


def _from_compact():
    out = []
    for i, c in enumerate(CH.cases()):
        steps = tuple(Step(iv, before) for iv, (_, before, _) in zip(c.intervals, CH.walk(c.name)))
        out.append(XCase("hist/" + c.name, c.R, c.K, c.pm, TOPS[i % len(TOPS)], c.hist_index, c.stride,
                         c.col_valid, steps, {}))
    return out


def _from_dense():
    out = []
    for c in AC.cases():
        h = c.h
        S = h.stride or h.K
        used = used_slots(h)
        spare = sorted(set(range(S)) - set(used))
        steps = []
        for iv, (_, before, _) in zip(h.intervals, AC.walk(c.name)):
            dense = np.zeros_like(before)
            dense[:, used] = before[:, used]
            ch, _ = histograms.compact_from_dense(dense)
            ch[:, spare] = CH.SENTINEL
            steps.append(Step(iv, ch))
        out.append(XCase("attr/" + c.name, h.R, h.K, h.pm, c.top, h.hist_index, h.stride, h.col_valid,
                         tuple(steps), dict(c.planted)))
    return out


def _new(name, R, K, spec, chist0, *, pm, top, col_valid=None, seed=0):
    """One interval through ``_compact_history_cases.make``: spec {segment: [(bucket, count), ...]},
    chist0 {(row, slot): {bucket: count}}."""
    c = CH.make(name, R, K, [spec], chist0, pm=pm, col_valid=col_valid, seed=100 + seed)
    return XCase("new/" + name, R, K, pm, top, None, 0, col_valid, (Step(c.intervals[0], c.chist0),), {})


FULL_B = [10 * (i + 1) for i in range(E)]  # buckets 10, 20, ..., 120


def _directed():
    out = []
    # (0, 0): 1,000 of the 1,011 history samples in the FIRST entry, rank 505: T = 10;
    # (0, 1): 1,000 of them in the TWELFTH, rank 959: T = 120
    first = {b: (1000 if b == FULL_B[0] else 1) for b in FULL_B}
    last = {b: (1000 if b == FULL_B[-1] else 1) for b in FULL_B}
    c = _new("T_first_and_twelfth", 1, 2, {0: [(5, 3), (10, 20), (15, 4), (130, 2)],
                                           1: [(100, 9), (120, 30), (121, 2), (200, 1)]},
             {(0, 0): first, (0, 1): last}, pm=500, top=2, seed=1)
    out.append(c._replace(planted={"T": {(0, 0): 10, (0, 1): 120}}))
    # N = 21, pm 500: rank 10.  (0, 0): 10 samples below the boundary, incl == rank: the NEXT entry
    # holds the rank, T = 30; (0, 1): 11 below, incl == rank + 1: T = 20
    c = _new("rank_on_entry_boundary", 1, 2, {0: [(20, 5), (30, 5), (40, 2)], 1: [(20, 5), (30, 5), (40, 2)]},
             {(0, 0): {20: 10, 30: 11}, (0, 1): {20: 11, 30: 10}}, pm=500, top=2, seed=2)
    out.append(c._replace(planted={"T": {(0, 0): 30, (0, 1): 20}}))
    # twelve counts of 2^32 - 1: N = 12 (2^32 - 1) passes 2^32; rank (990 (N - 1)) // 1000 lies in
    # the twelfth entry
    c = _new("N_past_2_32", 1, 1, {0: [(60, 9), (120, 5), (125, 3)]},
             {(0, 0): {b: 2 ** 32 - 1 for b in FULL_B}}, pm=990, top=1, seed=3)
    out.append(c._replace(planted={"T": {(0, 0): 120}}))
    # K = 1, 3, 5, 17: the trailing rows of the last four-element load lie past K
    for K in (1, 3, 5, 17):
        spec, hist = {}, {}
        for r in range(2):
            for k in range(K):
                b = 60 + k
                spec[r * K + k] = [(b, 10), (b + 1, 3), (b + 8, 1 + (r + k) % 3)]
                hist[(r, k)] = {b: 50, b + 1: 20, b + 8: 2}
        out.append(_new(f"K{K}_rows_past_K", 2, K, spec, hist, pm=950, top=4, seed=4 + K))
    # one row of 16 kernels = four loads; the load of wave v holds {eligible, empty history, empty
    # segment, col_valid 0} rotated by v
    K = 16
    spec, hist, valid, eligible = {}, {}, np.ones(K, np.uint8), []
    for k in range(K):
        state = (k + k // 4) % 4
        b = 40 + 3 * k
        if state != 2:
            spec[k] = [(b, 12), (b + 9, 1 + k % 4)]
        if state != 1:
            hist[(0, k)] = {b: 90, b + 1: 8, b + 9: 2}
        if state == 3:
            valid[k] = 0
        if state == 0:
            eligible.append(k)
    c = _new("four_rows_four_rotations", 1, K, spec, hist, pm=950, top=8, col_valid=valid, seed=30)
    assert sorted(k % 4 for k in eligible) == [0, 1, 2, 3]  # the eligible element sits in every row once
    out.append(c._replace(planted={"taken": {0: eligible}}))
    # slots that are not the columns: the reversed order into 8 slots with one column left out;
    # the slots no column uses hold the sentinel
    R, K, S = 2, 5, 8
    index = np.array([S - 1 - k for k in range(K)], np.int32)
    index[2] = -1
    spec = {r * K + k: [(70 + 2 * k, 8), (90 + k, 1 + r)] for r in range(R) for k in range(K)}
    base = CH.make("hist_index_reversed", R, K, [spec], {}, pm=950, seed=131)
    ch = np.zeros((R, S, CB), np.uint8)
    ch[:] = CH.SENTINEL
    for r in range(R):
        for k in range(K):
            if index[k] >= 0:
                ch[r, index[k]] = CH.element({70 + 2 * k: 40 + r, 71 + 2 * k: 3, 90 + k: 1})
    out.append(XCase("new/hist_index_reversed", R, K, 950, 5, index, S, None, (Step(base.intervals[0], ch),),
                     {"taken": {0: [0, 1, 3, 4], 1: [0, 1, 3, 4]}}))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _from_compact() + _from_dense() + _directed()
    assert len({c.name for c in out}) == len(out)
    for c in out:
        assert all(s.chist.shape == (c.R, c.stride or c.K, CB) and s.chist.dtype == np.uint8 for s in c.steps)
        for s in c.steps:
            s.chist.setflags(write=False)
    return tuple(out)


def directed():
    return tuple(c for c in cases() if c.name.startswith("new/"))


def case(name):
    return next(c for c in cases() if c.name == name)


def attr_kwargs(c):
    return dict(hist_index=c.hist_index, col_valid=c.col_valid)


def _frozen(res):
    for f in vars(res).values():
        f.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def twin(name):
    """``histograms.segment_compact_history_attribution`` of every step of a case."""
    c = case(name)
    out = tuple(_frozen(histograms.segment_compact_history_attribution(
        s.iv.keys, s.iv.off, s.iv.lens, c.K, s.chist, c.pm, c.top, s.iv.cap, **attr_kwargs(c)))
        for s in c.steps)
    _check_aims(c, out)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name):
    """``histograms.segment_history_attribution`` of every step on the dense expansion."""
    c = case(name)
    return tuple(_frozen(histograms.segment_history_attribution(
        s.iv.keys, s.iv.off, s.iv.lens, c.K, dense_of(c, s.chist), c.pm, c.top, s.iv.cap, **attr_kwargs(c)))
        for s in c.steps)


def _check_aims(c, res):
    """The aims of a case as they must show in the twin's result."""
    for key, want in c.planted.items():
        if key == "T":  # {(row, column): threshold bucket}, every named element a winner
            for (r, k), t in want.items():
                j = res[0].idx[r].tolist().index(k)
                assert res[0].thr_bucket[r, j] == t, (c.name, r, k)
        elif key == "taken":  # {row: the columns taken}
            for r, cols in want.items():
                assert sorted(np.flatnonzero(~np.isnan(res[0].loss_all[r])).tolist()) == cols, (c.name, r)
                assert sorted(k for k in res[0].idx[r].tolist() if k >= 0) == cols[:c.top], (c.name, r)
        else:  # _segment_history_attr_cases.planted: {(interval, row, position): column}
            i, r, j = key
            assert res[i].idx[r, j] == want, (c.name, key)
    if c.name == "new/N_past_2_32":
        count, _, _ = histograms._chist_fields(c.steps[0].chist)
        assert int(count[0, 0].sum()) > 2 ** 32 and (count[0, 0] == 2 ** 32 - 1).all()
    if c.name.endswith("_rows_past_K"):
        assert c.K % 4 != 0 and not np.isnan(res[0].loss_all).any()
