"""CPU: the host twins of the history aging, ``histograms.compact_age`` and ``history_age``, over
the shared elements of ``_history_age_cases`` at shifts 1, 2 and 31 -- canonical output, aging
commutes with the dense expansion, aging by s then t is aging by s + t, evicted / full equal a
direct count -- and the stale-entry scenario the feature exists for: a full element that folds a
new bucket in every call admits it once aging has evicted the stale entries."""
import numpy as np
import pytest

import _compact_history_cases as C
import _history_age_cases as A
from nvidia_resiliency_ext.straggler import histograms

N = len(A.elements())
SHAPE = (4, N // 4)  # the directed elements and 297 random ones, over four rows


def hist():
    return A.history(*SHAPE)


def test_the_shared_elements_are_canonical_and_cover_the_directed_cases():
    assert histograms.compact_is_canonical(hist()).all()
    n = A.elements()[:, 5 * A.E:].view("<u4")[:, 0]
    assert set(n.tolist()) == set(range(A.E + 1))  # every fill level
    assert len(A.NAMES) == len(set(A.NAMES)) >= 10


@pytest.mark.parametrize("shift", A.SHIFTS)
def test_compact_age_is_canonical_and_commutes_with_the_dense_expansion(shift):
    h = hist()
    before = h.copy()
    out, evicted, full = A.aged(*SHAPE, 0, shift)
    assert np.array_equal(h, before)  # the input is left unchanged
    assert out.dtype == np.uint8 and out.shape == h.shape
    assert histograms.compact_is_canonical(out).all()
    dense = histograms.compact_to_dense(h)
    assert np.array_equal(histograms.compact_to_dense(out), histograms.history_age(dense, shift))
    # evicted / full against a direct count on the bytes
    want, ev, fu = A.direct(h, shift)
    assert np.array_equal(out, want)
    assert evicted.dtype == full.dtype == np.uint64
    assert np.array_equal(evicted, ev) and np.array_equal(full, fu)
    n0 = h[..., 5 * A.E:].view("<u4")[..., 0].astype(np.int64)
    n1 = out[..., 5 * A.E:].view("<u4")[..., 0].astype(np.int64)
    assert np.array_equal(evicted, (n0 - n1).sum(1).astype(np.uint64))
    assert np.array_equal(full, (n1 == A.E).sum(1).astype(np.uint64))


@pytest.mark.parametrize("s,t", [(1, 1), (1, 2), (2, 1), (2, 29), (1, 30), (15, 16)])
def test_aging_by_s_then_t_is_aging_by_s_plus_t(s, t):
    h = hist()
    a, ev_a, _ = histograms.compact_age(h, s)
    b, ev_b, full_b = histograms.compact_age(a, t)
    want, ev, full = histograms.compact_age(h, s + t)
    assert np.array_equal(b, want)
    assert np.array_equal(ev_a + ev_b, ev) and np.array_equal(full_b, full)
    dense = histograms.compact_to_dense(h)
    assert np.array_equal(histograms.history_age(histograms.history_age(dense, s), t),
                          histograms.history_age(dense, s + t))


def test_directed_elements_age_as_stated():
    el = A.elements()
    by = {n: el[i].reshape(1, 1, A.CB) for i, n in enumerate(A.NAMES)}
    empty = np.zeros((1, 1, A.CB), np.uint8)
    for name in ("empty", "one_count_1", "full_to_empty"):
        out, ev, full = histograms.compact_age(by[name], 1)
        assert np.array_equal(out, empty) and full[0] == 0
        assert ev[0] == {"empty": 0, "one_count_1": 1, "full_to_empty": 12}[name]
    out, ev, full = histograms.compact_age(by["one_count_max"], 1)
    assert np.array_equal(out[0, 0], A.pack({50: 2 ** 31 - 1})) and ev[0] == 0
    out, ev, full = histograms.compact_age(by["full_all_survive"], 31)
    assert full[0] == 1 and ev[0] == 0
    assert np.array_equal(out[0, 0], A.pack({7 * i + 3: 1 for i in range(A.E)}))
    out, ev, full = histograms.compact_age(by["full_alternating"], 1)
    assert ev[0] == 6 and full[0] == 0
    assert np.array_equal(out[0, 0], A.pack({9 * i + 1: (A.BIG + i) >> 1 for i in range(1, A.E, 2)}))
    out, ev, _ = histograms.compact_age(by["full_last_survives"], 2)  # index 11 -> 0
    assert ev[0] == 11 and np.array_equal(out[0, 0], A.pack({11 * 11 + 4: A.MAXC >> 2}))
    out, ev, _ = histograms.compact_age(by["full_first_survives"], 2)
    assert ev[0] == 11 and np.array_equal(out[0, 0], A.pack({5: A.MAXC >> 2}))
    # bucket byte 0: only the count decides
    out, ev, _ = histograms.compact_age(by["bucket0_survives"], 1)
    assert ev[0] == 1 and np.array_equal(out[0, 0], A.pack({0: (A.BIG + 1) >> 1, 17: 1}))
    out, ev, _ = histograms.compact_age(by["bucket0_evicted"], 1)
    assert ev[0] == 1 and np.array_equal(out[0, 0], A.pack({9: A.MAXC >> 1}))
    out, ev, _ = histograms.compact_age(by["bucket239"], 1)
    assert ev[0] == 1 and np.array_equal(out[0, 0], A.pack({239: A.BIG >> 1}))


def test_history_age_reads_int32_as_u32_and_keeps_the_ends():
    d = np.zeros((1, 2, A.BINS), np.uint32)
    d[0, 0, 0], d[0, 0, 239], d[0, 1, 7] = 2 ** 32 - 1, 3, 1
    for src in (d, d.view(np.int32)):
        out = histograms.history_age(src, 1)
        assert out.dtype == np.uint32 and out[0, 0, 0] == 2 ** 31 - 1 and out[0, 0, 239] == 1
        assert out[0, 1].sum() == 0
    assert histograms.history_age(d, 31)[0, 0, 0] == 1


def test_bad_arguments():
    h = hist()
    for bad in (0, 32, -1, 1.5, True):
        with pytest.raises(ValueError, match="shift"):
            histograms.compact_age(h, bad)
        with pytest.raises(ValueError, match="shift"):
            histograms.history_age(np.zeros((1, 1, A.BINS), np.uint32), bad)
    with pytest.raises(ValueError, match="chist"):
        histograms.compact_age(np.zeros((1, 1, 60), np.uint8), 1)
    with pytest.raises(ValueError, match="hist"):
        histograms.history_age(np.zeros((1, 1, 239), np.uint32), 1)
    sent = np.broadcast_to(C.SENTINEL, (1, 1, A.CB)).copy()
    with pytest.raises(ValueError, match="canonical"):
        histograms.compact_age(sent, 1)


def test_aging_frees_the_stale_entries_of_a_full_element():
    """An element filled to 12 buckets by early intervals, then fed intervals in ONE new bucket
    above them.  Without aging every call folds; with aging at shifts that zero the old counts the
    new bucket is admitted and folded returns to 0."""
    K, pm, new = 1, 990, 200
    early = {10 * (i + 1): 5 for i in range(A.E)}  # counts of 5: gone after three halvings
    h0 = np.zeros((1, 1, A.CB), np.uint8)
    off = np.zeros(1, np.int64)
    for b in early:  # twelve early intervals, one bucket each
        keys = np.full(early[b], C.key(b), np.uint32)
        h0 = histograms.segment_compact_history_scores(keys, off, np.array([keys.size], np.int32),
                                                       K, h0, pm).hist
    assert np.array_equal(h0[0, 0], A.pack(early))
    keys = np.full(40, C.key(new), np.uint32)
    lens = np.array([keys.size], np.int32)

    h = h0
    for _ in range(4):  # without aging: stuck
        res = histograms.segment_compact_history_scores(keys, off, lens, K, h, pm)
        assert int(res.folded[0]) == keys.size
        h = res.hist
    assert new not in histograms._chist_entries(h[0, 0])

    h, folded, evicted = h0, [], []
    for _ in range(5):  # age, then score and update
        h, ev, _ = histograms.compact_age(h, 1)
        evicted.append(int(ev[0]))
        res = histograms.segment_compact_history_scores(keys, off, lens, K, h, pm)
        folded.append(int(res.folded[0]))
        h = res.hist
    # 5 -> 2 -> 1 -> 0: the third halving empties the eleven old entries that took no folds; the
    # top one (120) took the folded samples and outlives them by a few halvings
    assert folded[:2] == [40, 40] and evicted[:3] == [0, 0, 11]
    assert folded[2:] == [0, 0, 0]
    assert histograms._chist_entries(h[0, 0]).keys() >= {new}
    assert histograms.compact_is_canonical(h).all()
    # one pass at a shift that zeroes the old counts at once
    h, ev, full = histograms.compact_age(h0, 3)
    assert ev[0] == 12 and full[0] == 0 and not h.any()
    res = histograms.segment_compact_history_scores(keys, off, lens, K, h, pm)
    assert int(res.folded[0]) == 0 and histograms._chist_entries(res.hist[0, 0]) == {new: 40}
