"""The cases of the tests of nvrx_histogram_history_scores_compact and of the dense / compact
conversion.  Every element is built by hand (``SPECS``: a history as {bucket: count} and an
interval's counts as {bucket: count}), aimed at the kernel in histogram_history_compact.hip:

* ``element_cases()``: one case per spec, R = 1, K = 18, the spec at columns 0, 15, 16 and K - 1
  (the first and last element of a 16-element workgroup trip, the first of the next, the last of a
  short trip), the other columns filled with the other specs in rotation.
* ``geometry_cases()``: the specs in rotation over (R, K) = (1, 1), (1, 17), (3, 37), (2, 50) and
  (2049, 1) -- the trip remainder, several splits, a short last split, one split per row and rows
  beyond 2,048 -- and over (3, 37) with ``hist_stride > K`` and a permuted ``hist_index`` with
  negative entries (the slots no column uses hold a sentinel pattern), ``col_valid`` with zeros,
  ``skip_rows``; and over (1, 17) at permille 0, 500, 990 and 1000.

``expected(name)`` is the host twin's fused result, computed once and never written to."""
import functools
from collections import namedtuple

import numpy as np

from nvidia_resiliency_ext.straggler import histograms

BINS = 240
E = histograms.CHIST_ENTRIES
CB = histograms.CHIST_BYTES
SENTINEL = (np.arange(CB) * 7 + 0xA5).astype(np.uint8)  # not canonical: n is far above 12
U32 = 2 ** 32 - 1
THR = 0.9

Spec = namedtuple("Spec", "name hist cur pm")
HCase = namedtuple("HCase", "name R K counts chist0 pm col_valid hist_index stride skip_rows")

FULL = {10 * (i + 1): 5 for i in range(E)}       # buckets 10, 20, ..., 120
TEN = {10 + 20 * i: 9 for i in range(E - 2)}     # buckets 10, 30, ..., 190: two entries free
ELEVEN = {10 * i + 3: i + 1 for i in range(E - 1)}  # buckets 3, 13, ..., 103: one entry free

SPECS = (
    Spec("empty_history", {}, {5: 3, 100: 2}, 990),           # admitted, never scored
    Spec("no_samples", {10: 4, 20: 1}, {}, 990),              # the 64 bytes unchanged
    Spec("n1", {40: 7}, {40: 2, 41: 5}, 990),
    # one entry free, two new buckets: 2 is admitted, 200 folds into 103
    Spec("n11_one_more_than_fits", ELEVEN, {2: 1, 200: 4, 13: 2}, 950),
    Spec("n12_hit_in_used", FULL, {10: 7, 120: 1, 60: 30}, 950),
    Spec("full_new_below", FULL, {3: 4, 9: 1}, 950),          # folds to min S'
    Spec("full_new_between", FULL, {15: 2, 119: 1, 20: 3}, 950),
    Spec("full_new_above", FULL, {200: 3, 239: 1}, 950),
    # two entries free, three new buckets: 5 and 20 admitted, 40 folds into 30
    Spec("two_free_three_new", TEN, {5: 1, 20: 4, 40: 3, 30: 1}, 950),
    Spec("buckets_0_3_4", {0: 5, 3: 2, 4: 9}, {0: 1, 3: 1, 4: 1, 7: 2}, 500),  # T = 4: the next lane
    Spec("buckets_63_64", {63: 10, 64: 10}, {63: 3, 64: 4, 65: 1}, 500),        # T = 63: a row's end
    Spec("bucket_239", {0: 1, 239: 6}, {239: 2, 238: 1, 0: 1}, 100),            # T = 0, tail in 239
    Spec("wide_buckets", {237: 3, 238: 1, 239: 6}, {237: 1, 238: 5, 239: 5}, 350),  # T = 238
    Spec("T_inside_a_lane", {8: 10, 9: 10, 10: 10, 11: 10}, {8: 1, 9: 2, 10: 3, 11: 4}, 500),  # T = 9
    Spec("T_is_the_highest_bucket", {50: 1, 60: 1000}, {60: 3, 61: 2, 50: 1}, 990),  # no history tail
    # N = 12 (2^32 - 1): the rank needs 64 bits
    Spec("N_near_12_u32", {20 * i + 1: U32 for i in range(E)}, {1: 5, 221: 7, 230: 9}, 990),
    # three bins of 0xFFFFFFF0 fold into an entry that holds 0x10: 0xFFFFFFFF, and folded the
    # exact u64 sum; a u32 add of the bins wraps to 0xFFFFFFD0 and would give 0xFFFFFFE0
    Spec("fold_sum_needs_64_bits", {**FULL, 120: 0x10},
         {130: 0xFFFFFFF0, 140: 0xFFFFFFF0, 150: 0xFFFFFFF0}, 950),
    Spec("kept_entry_saturates", {40: U32 - 1, 50: 3}, {40: 5, 50: U32}, 950),
    Spec("empty_history_20_buckets", {}, {12 * i + 2: 15 + i for i in range(20)}, 950),
    Spec("all_240_bins", {7: 2}, {b: b + 1 for b in range(BINS)}, 950),
)
PERMILLES = (0, 500, 990, 1000)


def dense(entries):
    d = np.zeros(BINS, np.uint32)
    for b, v in entries.items():
        d[b] = v
    return d


def element(entries):
    """A canonical element from {bucket: count} (at most 12 buckets)."""
    ch, folded = histograms.compact_from_dense(dense(entries).reshape(1, 1, BINS))
    assert not folded.any()
    return ch[0, 0]


def used_slots(c):
    """The history slots some column of a case uses (with or without col_valid)."""
    index = range(c.K) if c.hist_index is None else [int(s) for s in c.hist_index]
    return sorted({s for s in index if s >= 0})


def build(name, R, K, spec_of, pm, *, col_valid=None, hist_index=None, stride=0, skip_rows=None):
    """A case whose element (r, k) is SPECS[spec_of(r, k)]."""
    S = stride or K
    index = list(range(K)) if hist_index is None else [int(s) for s in hist_index]
    counts = np.zeros((R, K, BINS), np.uint32)
    chist = np.zeros((R, S, CB), np.uint8)
    chist[:, sorted(set(range(S)) - {s for s in index if s >= 0})] = SENTINEL
    elems = [element(s.hist) for s in SPECS]
    curs = [dense(s.cur) for s in SPECS]
    for r in range(R):
        for k in range(K):
            i = spec_of(r, k) % len(SPECS)
            counts[r, k] = curs[i]
            if index[k] >= 0:
                chist[r, index[k]] = elems[i]
    return HCase(name, R, K, counts, chist, pm, col_valid, hist_index, stride, skip_rows)


@functools.lru_cache(maxsize=None)
def element_cases():
    out = []
    for i, s in enumerate(SPECS):
        at = lambda r, k, i=i: i if k in (0, 15, 16, 17) else i + k  # noqa: E731
        out.append(build("elem_" + s.name, 1, 18, at, s.pm))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def geometry_cases():
    rot = lambda r, k: 7 * r + k  # noqa: E731
    out = [build(f"R{R}_K{K}", R, K, rot, 950) for R, K in ((1, 1), (1, 17), (3, 37), (2, 50))]
    out.append(build("R2049_K1", 2049, 1, lambda r, k: r, 950))
    rng = np.random.default_rng(5)
    index = rng.permutation(45)[:37].astype(np.int32)
    index[[0, 16, 36, 20]] = (-1, -3, -1, -2)
    out.append(build("stride_and_index", 3, 37, rot, 950, hist_index=index, stride=45))
    valid = np.ones(37, np.uint8)
    valid[[0, 5, 15, 16, 36]] = 0
    out.append(build("col_valid", 3, 37, rot, 950, col_valid=valid))
    out.append(build("skip_rows", 3, 37, rot, 950, skip_rows=np.array([0, 1, 0], np.uint8)))
    out.append(build("all_three", 3, 37, rot, 990, hist_index=index, stride=45, col_valid=valid,
                     skip_rows=np.array([1, 0, 0], np.uint8)))
    out += [build(f"permille_{pm}", 1, 17, lambda r, k: 3 * k, pm) for pm in PERMILLES]
    return tuple(out)


def cases():
    return element_cases() + geometry_cases()


def case(name):
    return next(c for c in cases() if c.name == name)


def history_kwargs(c):
    return dict(hist_index=c.hist_index, col_valid=c.col_valid, skip_rows=c.skip_rows)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The host twin's fused result of a case (its score does not depend on the update)."""
    c = case(name)
    return histograms.compact_history_scores(c.counts, c.chist0, c.pm, score_thr=THR,
                                             **history_kwargs(c))


def clustered(rng, R, K, spread=3, peak=4000):
    """Random counts of real kernels: per element 1 to ``spread`` adjacent buckets from a start
    that depends on (r, k) alone, so chained intervals stay within ``spread`` buckets and nothing
    folds."""
    c = np.zeros((R, K, BINS), np.uint32)
    for r in range(R):
        for k in range(K):
            lo = 20 + (13 * k + 5 * r) % 200
            for b in range(lo, lo + int(rng.integers(1, spread + 1))):
                c[r, k, b] = rng.integers(1, peak)
    return c
