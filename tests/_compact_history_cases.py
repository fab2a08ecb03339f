"""The cases of the compact-history tests (CPU twin and GPU kernel).  Two sets share one shape
(``CCase``: the fields of ``_segment_history_cases.HCase`` with a compact starting history):

* ``converted()``: every case of ``_segment_history_cases`` (imported read-only), its ``hist0``
  converted with ``histograms.compact_from_dense``; the slots no column uses hold a 64-byte
  sentinel pattern instead, which no call may touch.
* ``directed()``: small cases (R <= 3, K <= 4) aimed at the fold rule of
  segment_history_compact.hip: a 13th bucket above / below a full element, admission in ascending
  order with two free entries, a full element hit only in used buckets, an empty element receiving
  20 buckets at once, a fold target that saturates, skip_rows / col_valid on a folding element, a
  fold scored in the same fused call, the bucket rule's ends as entries, the sample trips and the
  trimmed window.

``walk`` gives per interval the retained windows' counts, the history before and the host twin's
fused result: the reference every test shares, computed once and never written to."""
import functools
from collections import namedtuple

import numpy as np

import _segment_history_cases as H
import _segment_tail_cases as ST
from nvidia_resiliency_ext.straggler import histograms

BINS = 240
E = histograms.CHIST_ENTRIES
CB = histograms.CHIST_BYTES
SENTINEL = (np.arange(CB) * 7 + 0xA5).astype(np.uint8)  # not canonical: n is far above 12
NEAR_FULL = 2 ** 32 - 2
THR = 0.9

CCase = namedtuple("CCase", "name R K intervals pm col_valid hist_index stride skip_rows chist0")

EDGES = histograms.edges_keys()


def key(b):
    """A duration key of bucket b (its lower edge)."""
    return int(EDGES[b])


def used_slots(c):
    """The history slots some column of a case uses (with or without col_valid)."""
    index = range(c.K) if c.hist_index is None else [int(s) for s in c.hist_index]
    return sorted({s for s in index if s >= 0})


def element(entries):
    """A canonical element from {bucket: count}."""
    d = np.zeros(BINS, np.int64)
    for b, v in entries.items():
        d[b] = v
    ch, folded = histograms.compact_from_dense(d.reshape(1, 1, BINS))
    assert not folded.any()
    return ch[0, 0]


@functools.lru_cache(maxsize=None)
def converted():
    out = []
    for c in H.cases():
        S = c.stride or c.K
        used = used_slots(c)
        dense = np.zeros_like(c.hist0)
        dense[:, used] = c.hist0[:, used]
        ch, folded = histograms.compact_from_dense(dense)
        assert not folded.any()  # no starting history of those cases has more than 12 buckets
        ch[:, sorted(set(range(S)) - set(used))] = SENTINEL
        out.append(CCase(c.name, c.R, c.K, c.intervals, c.pm, c.col_valid, c.hist_index, c.stride,
                         c.skip_rows, ch))
    return tuple(out)


def make(name, R, K, specs, chist0, *, cap=0, aligned16=False, pm=950, col_valid=None,
         skip_rows=None, seed=0):
    """specs: per interval {segment g: [(bucket, count), ...] or an array of keys}; a segment not
    named is empty."""
    ivs = []
    for i, spec in enumerate(specs):
        runs = {}
        for g, v in spec.items():
            runs[g] = (np.asarray(v, np.uint32) if isinstance(v, np.ndarray) else
                       np.concatenate([np.full(n, key(b), np.uint32) for b, n in v]))
        lens = [runs[g].size if g in runs else 0 for g in range(R * K)]
        ivs.append(ST.layout(f"{name}#{i}", R, K, lens, lambda rng, g, n: rng.permutation(runs[g]),
                             cap=cap, aligned16=aligned16, pm=pm, seed=7000 + 10 * seed + i))
    ch = np.zeros((R, K, CB), np.uint8)
    for (r, k), entries in chist0.items():
        ch[r, k] = element(entries)
    return CCase(name, R, K, tuple(ivs), pm, col_valid, None, 0, skip_rows, ch)


FULL = {10 * (i + 1): 5 for i in range(E)}       # buckets 10, 20, ..., 120
TEN = {10 + 20 * i: 9 for i in range(E - 2)}     # buckets 10, 30, ..., 190: two entries free


@functools.lru_cache(maxsize=None)
def directed():
    rng = np.random.default_rng(77)
    out = [
        # (0, 0): a 13th bucket above all -> the highest entry; (0, 1): below all -> the lowest;
        # (0, 2): two free entries, new buckets 5, 20, 40, 60: 5 and 20 admitted, 40 -> 30, 60 -> 50,
        #         then a sample in bucket 0 below the now full element -> 5;
        # (0, 3): a full element hit only in used buckets: nothing folded;
        # (1, 0): an empty element, 20 buckets x 15 samples at once; (1, 1): never any sample
        make("fold_rule", 2, 4, [
            {0: [(200, 3), (20, 2)], 1: [(3, 4)], 2: [(60, 2), (5, 1), (40, 3), (20, 4), (30, 1)],
             3: [(10, 7), (120, 1), (60, 30)], 4: [(12 * i + 2, 15) for i in range(20)], 6: [(33, 3)]},
            {0: [(125, 4), (119, 1)], 1: [(15, 2), (9, 1)], 2: [(0, 2), (191, 1)], 3: [(20, 65)],
             4: [(12 * i + 3, 3) for i in range(20)], 6: [(34, 1), (32, 1)], 7: [(100, 70)]},
        ], {(0, 0): FULL, (0, 1): FULL, (0, 2): TEN, (0, 3): FULL}, seed=1),
        # the fold target sits at 2^32 - 2 and receives 1 sample (2^32 - 1 exactly), then 5
        make("fold_saturates", 1, 2, [{0: [(55, 1)], 1: [(40, 9)]}, {0: [(55, 5)], 1: [(41, 9)]}],
             {(0, 0): {**{50: NEAR_FULL, 60: 7}, **{70 + 10 * i: 1 for i in range(E - 2)}}}, seed=2),
        # every element full and hit in a new bucket: only (0, 0) may fold -- row 1 is skipped,
        # column 1 is not valid
        make("skip_and_invalid", 2, 2, [{g: [(200, 6), (20, 1)] for g in range(4)},
                                        {g: [(210, 2)] for g in range(4)}],
             {(r, k): FULL for r in range(2) for k in range(2)},
             col_valid=np.array([1, 0], np.uint8), skip_rows=np.array([0, 1], np.uint8), seed=3),
        # a full element whose tail samples (bucket 150) fold into its top entry (100): the fused
        # call scores them as tail against the history from before
        make("fused_fold_scores_before", 1, 1, [{0: [(100, 50), (150, 10)]}, {0: [(100, 50), (150, 10)]}],
             {(0, 0): {**{100: 1000}, **{8 * i + 1: 3 for i in range(E - 1)}}}, pm=990, seed=4),
        # the bucket rule's ends as entries: 0, 7 / 8, 237 / 238 / 239
        make("edge_buckets", 1, 3, [
            {0: np.array([0, 7, 8, 0, 7], np.uint32),
             1: np.array([H.KEY_WIDE - 1, H.KEY_WIDE, 2 ** 32 - 1, H.KEY_WIDE], np.uint32),
             2: np.array([0, 2 ** 32 - 1], np.uint32)},
            {0: np.array([8, 8, 7, 0, 1], np.uint32),
             1: np.array([2 ** 32 - 1, H.KEY_WIDE - 1, 5], np.uint32),
             2: np.array([7, 8, H.KEY_WIDE], np.uint32)},
        ], {(0, 0): {0: 4, 7: 2, 8: 9}, (0, 1): {237: 3, 238: 1, 239: 6},
            (0, 2): {0: 1, 7: 1, 8: 1, 237: 1, 238: 1, 239: 1}}, seed=5),
    ]
    # the sample trips (1, 63, 64, 65, 256, 257) at the four starts inside a 16-byte vector
    # (segment g starts at offset g % 4), unaligned and aligned; durations of 1-3 buckets and a few
    # slow calls, which over three intervals pass 12 buckets in some elements
    L = [1, 63, 64, 65, 256, 257]
    for name, al in (("trips_unaligned", False), ("trips_aligned16", True)):
        specs = [{g: ST.durations(rng, L[(g + i + g // 4) % 6], 3_000 * (1 + g % 4)) for g in range(12)}
                 for i in range(3)]
        out.append(make(name, 3, 4, specs, {}, aligned16=al, seed=6 + al))
    # the trimmed window: only the last 100 samples count
    specs = [{g: ST.durations(rng, [100, 101, 250, 7, 0, 300][(g + i) % 6], 9_000) for g in range(6)
              if (g + i) % 6 != 4} for i in range(2)]
    out.append(make("compact_cap_trims", 2, 3, specs, {(0, 0): FULL}, cap=100, seed=8))
    return tuple(out)


def cases():
    return converted() + directed()


def case(name):
    return next(c for c in cases() if c.name == name)


def history_kwargs(c):
    return dict(hist_index=c.hist_index, col_valid=c.col_valid, skip_rows=c.skip_rows)


@functools.lru_cache(maxsize=None)
def walk(name):
    """Per interval of a case: (counts of the retained windows, the compact history before, the
    twin's fused result)."""
    c = case(name)
    h, out = c.chist0, []
    for iv in c.intervals:
        counts = histograms.segment_counts(iv.keys, iv.off, iv.lens, c.K, iv.cap)
        res = histograms.compact_history_scores(counts, h, c.pm, score_thr=THR, **history_kwargs(c))
        out.append((counts, h, res))
        h = res.hist
    return tuple(out)
