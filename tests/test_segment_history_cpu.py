"""CPU: ``histograms.segment_history_scores`` -- the host twin of the individual tail scores straight
from ragged segments -- equals ``history_scores(segment_counts(...))`` and the plain-Python
definition (``_history_tail_ref``) on every case, interval by interval; every case proves from its
own keys that it hits what it is aimed at; and a scenario through the twins: a rank slow on every
16th call of one kernel is the one rank its own history singles out."""
import numpy as np
import pytest

import _history_tail_ref as HREF
import _segment_history_cases as C
import _segment_tail_cases as ST
from nvidia_resiliency_ext.straggler import histograms

CASES = C.cases()
BOTH = HREF.SCORE | HREF.UPDATE


def lists(a):
    return np.ascontiguousarray(a).astype(np.uint32).tolist()


def assert_same(a, b):
    for f in ("hist", "score", "tail_ns", "total_ns", "base_tail_ns", "base_total_ns", "history_share",
              "stragglers", "threshold_bucket", "tail_calls"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_twin_equals_history_scores_of_the_segment_counts(c):
    kw = C.history_kwargs(c)
    for iv, (counts, h, fused) in zip(c.intervals, C.walk(c.name)):
        windows = [np.bincount(histograms.bucket_of(w), minlength=C.BINS) for w in ST.windows(iv)]
        assert np.array_equal(counts.reshape(-1, C.BINS), np.asarray(windows))
        for score, update in ((True, True), (True, False), (False, True)):
            got = histograms.segment_history_scores(iv.keys, iv.off, iv.lens, c.K, h, c.pm, iv.cap,
                                                    score=score, update=update, score_thr=0.9, **kw)
            assert_same(got, histograms.history_scores(counts, h, c.pm, score=score, update=update,
                                                       score_thr=0.9, **kw))
            if score and update:
                assert_same(got, fused)
        # the definition in plain integers
        rows, new = HREF.history_scores(
            lists(counts), lists(h), c.pm, BOTH, score_thr=0.9,
            hist_index=None if c.hist_index is None else c.hist_index.tolist(),
            col_valid=None if c.col_valid is None else c.col_valid.tolist(),
            skip_rows=None if c.skip_rows is None else c.skip_rows.tolist())
        assert fused.hist.tolist() == new
        assert fused.tail_ns.tolist() == [r["tail_ns"] for r in rows]
        assert fused.base_total_ns.tolist() == [r["base_total_ns"] for r in rows]
        assert [HREF.bits(s) for s in fused.score] == [HREF.bits(r["score"]) for r in rows]
        assert fused.tail_calls.tolist() == [r["calls"] for r in rows]


def test_offsets_without_lengths():
    keys = np.arange(1000, 1010, dtype=np.uint32)
    off = np.array([0, 3, 3, 7, 10])
    h = np.zeros((2, 2, C.BINS), np.uint32)
    h[:, :, 100] = 5
    a = histograms.segment_history_scores(keys, off, None, 2, h, 500)
    b = histograms.segment_history_scores(keys, off[:4], [3, 0, 4, 3], 2, h, 500)
    assert_same(a, b)
    assert int(a.hist.sum()) == 20 + 10 and np.array_equal(a.hist[0, 1], h[0, 1])


# ---------------------------------------------------------------- what each case claims of itself
def _lens(c, i):
    return np.asarray(c.intervals[i].lens).reshape(c.R, c.K)


@pytest.mark.parametrize("name", ["lengths_unaligned", "lengths_aligned16"])
def test_claim_length_ladder_and_starts(name):
    c = C.case(name)
    for r in range(c.R):  # every row meets every length of the ladder in some interval
        assert {int(v) for v in _lens(c, 0)[r]} == set(ST.LENGTHS)
    assert [int(v) for v in _lens(c, 0)[0]] != [int(v) for v in _lens(c, 1)[0]]
    for iv in c.intervals:
        starts = {int(o) % 4 for o, n in zip(iv.off, iv.lens) if n > 0}
        assert starts == ({0} if iv.aligned16 else {0, 1, 2, 3})
    # every (row, kernel) has a history by the last interval, and some had none at their first samples
    last = C.walk(name)[-1][2]
    assert (last.threshold_bucket >= 0).sum() > 0
    assert any((w[2].threshold_bucket < 0)[_lens(c, i) > 0].any() for i, w in enumerate(C.walk(name)))


@pytest.mark.parametrize("name", ["cap_trims", "cap_trims_aligned16"])
def test_claim_cap_trims(name):
    c = C.case(name)
    for i, (counts, _, _) in enumerate(C.walk(name)):
        n = counts.sum(2)
        L = _lens(c, i)
        assert np.array_equal(n, np.minimum(L, 100)) and (L > 100).any() and (L == 100).any()
        iv = c.intervals[i]
        g = int(np.argmax(iv.lens == 250))  # a trimmed run: the first 150 samples are not counted
        full = np.bincount(histograms.bucket_of(iv.keys[iv.off[g]:iv.off[g] + 250]), minlength=C.BINS)
        assert full.sum() == 250 and counts.reshape(-1, C.BINS)[g].sum() == 100


def test_claim_negative_lengths_are_empty():
    c = C.case("negative_lengths")
    seen = False
    for i, (counts, h, res) in enumerate(C.walk(c.name)):
        neg = _lens(c, i) < 0
        assert neg.any() and not counts[neg].any()
        assert np.array_equal(res.hist[neg], h[neg]) and (res.threshold_bucket[neg] == -1).all()
        seen |= bool(h[neg].any())
    assert seen  # a negative length over a non-zero history


def test_claim_special_keys():
    c = C.case("special_keys")
    total = sum(w[0] for w in C.walk(c.name)).sum(0)  # [K, 240]
    assert total[0, 1:].sum() == 0 and total[0, 0] > 0 and total[3, 1:].sum() == 0
    assert total[1, 7] > 0 and total[1, 8] > 0 and total[1].sum() == total[1, 7] + total[1, 8]
    assert (total[2, 237:] > 0).all() and total[2, :237].sum() == 0
    assert np.count_nonzero(total[4]) > 20
    # bucket 0 weighs nothing: a kernel wholly there is eligible and adds nothing
    last = C.walk(c.name)[-1][2]
    assert (last.threshold_bucket[:, 0] == 0).any()


def test_claim_empty_and_filled():
    c = C.case("empty_and_filled")
    w = C.walk(c.name)
    # (0, 1): no samples, then samples without a history (not eligible), then scored
    assert _lens(c, 0)[0, 1] == 0 and not w[1][1][0, 1].any() and w[1][0][0, 1].any()
    assert w[1][2].threshold_bucket[0, 1] == -1 and w[2][2].threshold_bucket[0, 1] >= 0
    # (0, 2): samples, then none over a non-zero history: the slot stays bit-identical
    assert _lens(c, 1)[0, 2] == 0 and w[1][1][0, 2].any()
    assert np.array_equal(w[1][2].hist[0, 2], w[1][1][0, 2]) and w[1][2].tail_calls[0, 2] == 0
    assert w[1][2].threshold_bucket[0, 2] == -1
    # (1, 3): a negative length in the last interval over a history of 600 samples
    assert _lens(c, 2)[1, 3] < 0 and w[2][1][1, 3].sum() == 600


@pytest.mark.parametrize("K", [1, 5, 17, 300])
def test_claim_col_valid(K):
    c = C.case(f"col_valid_K{K}")
    off = c.col_valid == 0
    assert off.any() and (K == 1 or (~off).any())
    for counts, h, res in C.walk(c.name):
        assert counts[:, off].any() and not res.hist[:, off].any()
        assert (res.threshold_bucket[:, off] == -1).all()


@pytest.mark.parametrize("name", ["hist_index_permuted", "stride_above_K"])
def test_claim_slots(name):
    c = C.case(name)
    S = c.stride
    index = np.arange(c.K) if c.hist_index is None else c.hist_index
    used = sorted(int(s) for s in index if s >= 0)
    free = sorted(set(range(S)) - set(used))
    assert S > c.K and free and len(set(used)) == len(used)
    if c.hist_index is not None:
        assert (c.hist_index < 0).sum() == 2 and not np.array_equal(c.hist_index, np.arange(c.K))
    for counts, h, res in C.walk(name):
        assert (res.hist[:, free] == C.SENTINEL).all()
    assert C.walk(name)[-1][2].hist[:, used].any()


def test_claim_skip_rows():
    c = C.case("skip_rows")
    for counts, h, res in C.walk(c.name):
        assert counts[1].any() and counts[3].any()
        assert not res.hist[[1, 3]].any() and res.hist[[0, 2]].any()
    assert np.isnan(C.walk(c.name)[-1][2].score[[1, 3]]).all()
    assert not np.isnan(C.walk(c.name)[-1][2].score[[0, 2]]).any()


def test_claim_saturation():
    c = C.case("saturation")
    b = C.bucket(20_000)
    (c0, h0, r0), (c1, h1, r1) = C.walk(c.name)
    assert h0[0, 0, b] == C.NEAR_FULL and c0[0, 0].sum() == c0[0, 0, b] == 1
    assert r0.hist[0, 0, b] == 2 ** 32 - 1                      # reached exactly
    assert c1[0, 0].sum() == c1[0, 0, b] == 5 and r1.hist[0, 0, b] == 2 ** 32 - 1  # saturated
    assert r1.hist[0, 0, b - 1] == 7 and r1.threshold_bucket[0, 0] == b


def test_claim_tail_of_nothing_and_everything():
    c = C.case("tail_of_nothing_and_everything")
    for counts, h, res in C.walk(c.name):
        T = res.threshold_bucket[0]
        nz0, nz1 = np.nonzero(counts[0, 0])[0], np.nonzero(counts[0, 1])[0]
        assert nz0.max() <= T[0] and nz1.min() > T[1]
        assert res.tail_calls[0].tolist() == [0, int(counts[0, 1].sum())]
        w = histograms.weights()
        assert int(res.tail_ns[0]) == sum(int(v) * w[b] for b, v in enumerate(counts[0, 1]))


@pytest.mark.parametrize("name,splits,last", [("R1_K2048", 128, 16), ("R70_K33", 3, 1), ("R2049_K1", 1, 1)])
def test_claim_split_rule(name, splits, last):
    """The split rule of histogram_history.hip: about 2,048 workgroups over rows x
    splits, a split a whole number of 16-kernel trips."""
    c = C.case(name)
    s = min(-(-2048 // c.R), -(-c.K // 16))
    kper = -(-(-(-c.K // s)) // 16) * 16
    s = -(-c.K // kper)
    assert (s, c.K - (s - 1) * kper) == (splits, last)
    assert any((w[2].threshold_bucket >= 0).any() for w in C.walk(name))


# ---------------------------------------------------------------- scenario
def test_intermittent_straggler_against_its_own_history():
    """4 ranks x 6 kernels, calls [512, 128, 64, 16, 4, 1] per interval, bases [5e3, 2e5, 2e5, 2e6,
    2e5, 5e4] ns with 2 % normal jitter (default_rng(0)), cap 100, pm 990, absorb="healthy"
    emulated by a score call and an update call with skip_rows.  Rank 2's kernel 1 is 2x slower on
    every 16th call from interval 5 on.  Interval 0 has no history: NaN.  No rank is flagged in
    intervals 1-4, exactly rank 2 in intervals 5-8, at score_thr = 0.97: with this generation order
    the lowest healthy score is 0.9962 and rank 2 scores 0.954-0.960 once slow."""
    R, K, thr = 4, 6, 0.97
    calls = [512, 128, 64, 16, 4, 1]
    base = [5e3, 2e5, 2e5, 2e6, 2e5, 5e4]
    rng = np.random.default_rng(0)
    hist = np.zeros((R, K, C.BINS), np.uint32)
    lens = np.tile(np.asarray(calls, np.int32), R)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    flagged, scores = [], []
    for i in range(9):
        keys = []
        for r in range(R):
            for k in range(K):
                x = base[k] * (1.0 + 0.02 * rng.standard_normal(calls[k]))
                if i >= 5 and r == 2 and k == 1:
                    x[15::16] *= 2.0
                keys.append(x.astype(np.uint32))
        keys = np.concatenate(keys)
        s = histograms.segment_history_scores(keys, off, lens, K, hist, 990, cap=100, update=False,
                                              score_thr=thr)
        hist = histograms.segment_history_scores(keys, off, lens, K, hist, 990, cap=100, score=False,
                                                 skip_rows=s.stragglers).hist
        scores.append(s.score)
        flagged.append(set(np.nonzero(s.stragglers)[0].tolist()))
    print("scores", np.asarray(scores))
    assert np.isnan(scores[0]).all()
    assert flagged[:5] == [set()] * 5
    assert flagged[5:] == [{2}] * 4
    # the history of rank 2 has absorbed none of its slow intervals: 5 intervals x 100 retained
    assert int(hist[2, 1].sum()) == 500 and int(hist[0, 1].sum()) == 900
