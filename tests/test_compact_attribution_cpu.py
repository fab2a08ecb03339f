"""CPU: ``histograms.compact_history_attribution`` / ``segment_compact_history_attribution`` -- the
host twins of the attribution against the compact history -- equal, field for field and bit for
bit, ``histograms.history_attribution`` / ``segment_history_attribution`` on the dense expansion
(``compact_to_dense``) on every case of ``_compact_attr_cases``, although they work from the
element's entries and never expand; the sentinel slots no column uses are never looked at; bad
arguments are refused."""
import numpy as np
import pytest

import _compact_attr_cases as X
from nvidia_resiliency_ext.straggler import histograms

CASES = X.cases()
FIELDS = ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share", "loss_all")


def assert_same(got, want, what=""):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f)
        assert a.tobytes() == b.tobytes(), (what, f)  # NaN and the sign of zero count


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_segment_twin_equals_the_dense_twin_on_the_expansion(c):
    for s, twin, oracle in zip(c.steps, X.twin(c.name), X.oracle(c.name)):
        assert_same(twin, oracle, s.iv.name)


@pytest.mark.parametrize("c", [c for c in CASES if c.R * c.K <= 400], ids=lambda c: c.name)
def test_counts_twin_equals_the_dense_twin_on_the_expansion(c):
    for s, twin in zip(c.steps, X.twin(c.name)):
        counts = histograms.segment_counts(s.iv.keys, s.iv.off, s.iv.lens, c.K, s.iv.cap)
        got = histograms.compact_history_attribution(counts, s.chist, c.pm, c.top, **X.attr_kwargs(c))
        want = histograms.history_attribution(counts, X.dense_of(c, s.chist), c.pm, c.top, **X.attr_kwargs(c))
        assert_same(got, want, s.iv.name)
        assert_same(got, twin, s.iv.name)


def test_the_directed_cases_are_there():
    names = {c.name for c in X.directed()}
    assert {"new/T_first_and_twelfth", "new/rank_on_entry_boundary", "new/N_past_2_32",
            "new/four_rows_four_rotations", "new/hist_index_reversed"} <= names
    assert {f"new/K{K}_rows_past_K" for K in (1, 3, 5, 17)} <= names
    assert all(c.R <= 3 and c.K <= 17 for c in X.directed())
    for c in X.directed():
        X.twin(c.name)  # asserts the case's aims


def test_every_kind_of_case_takes_part():
    names = [c.name for c in CASES]
    for prefix in ("hist/", "attr/", "new/"):
        assert any(n.startswith(prefix) for n in names)
    assert {"attr/K2049", "attr/K4100", "attr/ties", "attr/bucket0_history", "hist/fold_rule",
            "hist/hist_index_permuted", "hist/stride_above_K", "hist/edge_buckets"} <= set(names)


@pytest.mark.parametrize("name", ["hist/hist_index_permuted", "hist/stride_above_K", "new/hist_index_reversed"])
def test_sentinel_slots_are_unused(name):
    """The slots no column uses hold a pattern that is not canonical: the twin neither refuses it
    nor lets it into a result -- with those slots zeroed the result is the same."""
    c = X.case(name)
    spare = sorted(set(range(c.stride or c.K)) - set(X.used_slots(c)))
    assert spare
    for s, twin in zip(c.steps, X.twin(name)):
        assert (s.chist[:, spare] == X.CH.SENTINEL).all()
        assert not histograms.compact_is_canonical(s.chist[:, spare]).any()
        cleared = s.chist.copy()
        cleared[:, spare] = 0
        got = histograms.segment_compact_history_attribution(s.iv.keys, s.iv.off, s.iv.lens, c.K, cleared,
                                                             c.pm, c.top, s.iv.cap, **X.attr_kwargs(c))
        assert_same(got, twin, s.iv.name)


def test_the_history_is_left_as_it_was():
    c = X.case("hist/fold_rule")
    s = c.steps[-1]
    ch = s.chist.copy()
    histograms.segment_compact_history_attribution(s.iv.keys, s.iv.off, s.iv.lens, c.K, ch, c.pm, c.top, s.iv.cap)
    assert ch.tobytes() == s.chist.tobytes()


def test_bad_arguments():
    c = X.case("new/rank_on_entry_boundary")
    s = c.steps[0]
    counts = histograms.segment_counts(s.iv.keys, s.iv.off, s.iv.lens, c.K, s.iv.cap)
    for top in (0, 17, True, 1.5):
        with pytest.raises(ValueError, match="top"):
            histograms.compact_history_attribution(counts, s.chist, 950, top)
    for pm in (-1, 1001, 0.5):
        with pytest.raises(ValueError, match="permille"):
            histograms.compact_history_attribution(counts, s.chist, pm, 4)
    with pytest.raises(ValueError, match="counts"):
        histograms.compact_history_attribution(counts[0], s.chist, 950, 4)
    with pytest.raises(ValueError, match="chist"):
        histograms.compact_history_attribution(counts, np.zeros((2, 2, 64), np.uint8), 950, 4)
    with pytest.raises(ValueError, match="chist"):
        histograms.compact_history_attribution(counts, np.zeros((1, 2, 240), np.uint32), 950, 4)
    with pytest.raises(ValueError, match="hist_index"):
        histograms.compact_history_attribution(counts, s.chist, 950, 4, hist_index=[0, 2])
    bad = s.chist.copy()
    bad[0, 1, 60] = 13  # n above 12
    with pytest.raises(ValueError, match="canonical"):
        histograms.compact_history_attribution(counts, bad, 950, 4)
    # ... but not in a slot no valid column uses
    histograms.compact_history_attribution(counts, bad, 950, 4, col_valid=[1, 0])
