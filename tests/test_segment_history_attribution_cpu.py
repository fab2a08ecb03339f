"""CPU: ``histograms.segment_history_attribution`` -- the host twin of the individual tail score
attribution straight from ragged segments -- is ``history_attribution`` over ``segment_counts``
field by field on every case and interval; it equals a restatement in plain Python integers
written out here, with a ``Fraction`` check that the loss is the three separately rounded f64
operations of the definition; ``hist`` is left as it was; the case list reaches every situation it
is aimed at; the argument errors are raised."""
from fractions import Fraction

import numpy as np
import pytest

import _segment_history_attr_cases as C
from nvidia_resiliency_ext.straggler import histograms

FIELDS = ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share", "loss_all")
CASES = C.cases()
M64 = (1 << 64) - 1
W = [int(v) for v in histograms.weights()]


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype == np.float64:
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), what  # every NaN is "not taken": one pattern
        got, want = got.view(np.uint64)[~gn], want.view(np.uint64)[~wn]
    assert np.array_equal(got, want), what


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_twin_is_history_attribution_over_segment_counts(c):
    h = c.h
    for iv, (counts, before, _), got in zip(h.intervals, C.walk(c.name), C.twin(c.name)):
        kept = before.copy()
        want = histograms.history_attribution(counts, before, h.pm, c.top, **C.attr_kwargs(h))
        for f in FIELDS:
            same_bits(getattr(got, f), getattr(want, f), (iv.name, f))
        assert got.idx.shape == (h.R, c.top) and got.loss_all.shape == (h.R, h.K)
        assert np.array_equal(before, kept)  # hist is read only


def bucket(x):
    if x < 8:
        return x
    e = x.bit_length() - 1
    return 8 * (e - 2) + ((x >> (e - 3)) & 7)


def definition(h, iv, before, top):
    """The ABI's definition in plain Python integers over the retained keys: per row the list of
    (column, loss, tail, total, calls, T, share), ranked, and the dense losses."""
    keys, rows, dense = iv.keys.tolist(), [], []
    for r in range(h.R):
        terms, losses = [], [float("nan")] * h.K
        for k in range(h.K):
            s = k if h.hist_index is None else int(h.hist_index[k])
            if s < 0 or (h.col_valid is not None and not h.col_valid[k]):
                continue
            n = int(iv.lens[r * h.K + k])
            if n <= 0:
                continue
            e = int(iv.off[r * h.K + k]) + n
            b = [bucket(x) for x in keys[e - (min(n, iv.cap) if iv.cap else n):e]]
            hist = [int(v) for v in before[r, s]]
            N = sum(hist)
            if N == 0:
                continue
            rank, acc, T = (h.pm * (N - 1)) // 1000, 0, 0
            for T, v in enumerate(hist):
                acc += v
                if acc > rank:
                    break
            tail, total = sum(W[v] for v in b if v > T) & M64, sum(W[v] for v in b) & M64
            btail = sum(v * W[i] for i, v in enumerate(hist) if i > T) & M64
            btotal = sum(v * W[i] for i, v in enumerate(hist)) & M64
            if btotal == 0:
                continue  # 0 / 0 (btail <= btotal): a NaN share, a NaN loss
            share = float(btail) / float(btotal)
            prod = float(total) * share
            loss = float(tail) - prod
            # each of the three operations is the correctly rounded exact result
            assert Fraction(share) == Fraction(float(Fraction(btail, btotal)))
            assert Fraction(prod) == Fraction(float(Fraction(float(total)) * Fraction(share)))
            assert Fraction(loss) == Fraction(float(Fraction(float(tail)) - Fraction(prod)))
            losses[k] = loss
            terms.append((k, loss, tail, total, sum(v > T for v in b) & 0xFFFFFFFF, T, share))
        terms.sort(key=lambda t: (-t[1], t[0]))  # -0.0 == +0.0: ties go to the lower column
        rows.append(terms[:top])
        dense.append(losses)
    return rows, dense


@pytest.mark.parametrize("c", [c for c in CASES if c.h.R * c.h.K <= 4100], ids=lambda c: c.name)
def test_twin_equals_the_definition_in_python_integers(c):
    h = c.h
    for iv, (_, before, _), got in zip(h.intervals, C.walk(c.name), C.twin(c.name)):
        rows, dense = definition(h, iv, before, c.top)
        same_bits(got.loss_all, np.asarray(dense, np.float64).reshape(h.R, h.K), iv.name)
        for r, terms in enumerate(rows):
            n = len(terms)
            assert got.idx[r].tolist() == [t[0] for t in terms] + [-1] * (c.top - n), (iv.name, r)
            same_bits(got.loss[r, :n], np.asarray([t[1] for t in terms], np.float64), (iv.name, r))
            assert got.tail_ns[r, :n].tolist() == [t[2] for t in terms]
            assert got.total_ns[r, :n].tolist() == [t[3] for t in terms]
            assert got.tail_calls[r, :n].tolist() == [t[4] for t in terms]
            assert got.thr_bucket[r, :n].tolist() == [t[5] for t in terms]
            same_bits(got.base_share[r, :n], np.asarray([t[6] for t in terms], np.float64), (iv.name, r))
            assert np.isnan(got.loss[r, n:]).all() and np.isnan(got.base_share[r, n:]).all()
            assert not got.tail_ns[r, n:].any() and not got.total_ns[r, n:].any()
            assert not got.tail_calls[r, n:].any() and (got.thr_bucket[r, n:] == -1).all()


def test_a_contracted_multiply_subtract_could_not_pass():
    """Over the winners of all cases, tail - total * share rounded after each operation differs
    somewhere from the same expression rounded once (what a fused multiply-subtract gives)."""
    differs = 0
    for c in CASES:
        for a in C.twin(c.name):
            for r, j in zip(*np.nonzero(a.idx >= 0)):
                tail, total, share = int(a.tail_ns[r, j]), int(a.total_ns[r, j]), float(a.base_share[r, j])
                if tail >= 1 << 53 or total >= 1 << 53:
                    continue  # special_keys: the conversion rounds first
                exact = Fraction(tail) - Fraction(total) * Fraction(share)
                fused = exact.numerator / exact.denominator  # int / int: correctly rounded
                separate = float(tail) - float(total) * share
                assert a.loss[r, j] == separate
                differs += fused != separate
    assert differs > 0


@pytest.mark.parametrize("c", [c for c in CASES if c.planted], ids=lambda c: c.name)
def test_planted_winners_sit_where_the_case_says(c):
    tw = C.twin(c.name)
    for (i, r, j), k in c.planted.items():
        assert tw[i].idx[r, j] == k, (i, r, j, tw[i].idx[r])


def test_the_case_list_reaches_what_it_is_aimed_at():
    """Every situation the cases are aimed at occurs in the list, by the twin's own results."""
    seen = dict(tie_among_winners=False, zero_tie=False, pads=False, empty_row_next_to_taken=False,
                nan_would_rank_first=False, negative_below_positive=False, trimmed_winner=False,
                empty_element=False, no_history=False, invalid_column=False, no_slot=False)
    lengths, below_width, at_width = set(), set(), set()
    for c in CASES:
        h = c.h
        for iv, (counts, before, _), a in zip(h.intervals, C.walk(c.name), C.twin(c.name)):
            taken = (~np.isnan(a.loss_all)).sum(1)
            if (taken >= c.top).any():
                at_width.add(c.top)
            if ((taken > 0) & (taken < c.top)).any():
                below_width.add(c.top)
            seen["pads"] |= bool(((a.idx[:, 0] >= 0) & (a.idx[:, -1] == -1)).any())
            seen["empty_row_next_to_taken"] |= bool((taken == 0).any() and (taken > 0).any())
            for r in range(h.R):
                n = int((a.idx[r] >= 0).sum())
                if n == 0:
                    continue
                eq = a.loss[r, 1:n] == a.loss[r, :n - 1]
                if eq.any():
                    assert (np.diff(a.idx[r, :n])[eq] > 0).all()  # the lower column first
                    seen["tie_among_winners"] |= bool((a.loss[r, :n - 1][eq] != 0).any())
                    seen["zero_tie"] |= bool((a.loss[r, :n - 1][eq] == 0).any())
                v = a.loss[r, :n]
                if (v < 0).any() and (v > 0).any():
                    seen["negative_below_positive"] |= bool(np.flatnonzero(v < 0).min() > np.flatnonzero(v > 0).max())
                for k in a.idx[r, :n].tolist():
                    lengths.add(C.retained(iv, r * h.K + k))
                    seen["trimmed_winner"] |= bool(iv.cap and iv.lens[r * h.K + k] > iv.cap)
            for r, k in zip(*np.nonzero(np.isnan(a.loss_all))):
                s = k if h.hist_index is None else int(h.hist_index[k])
                if h.col_valid is not None and not h.col_valid[k]:
                    seen["invalid_column"] = True
                elif s < 0:
                    seen["no_slot"] = True
                elif C.retained(iv, r * h.K + k) == 0:
                    seen["empty_element"] = True
                elif not before[r, s].any():
                    seen["no_history"] = True
                else:  # a history, samples and still no loss: every history sample in bucket 0
                    assert before[r, s, 0] and not before[r, s, 1:].any()
                    tail = sum(int(n) * W[b] for b, n in enumerate(counts[r, k]) if b > 0)
                    best = np.nanmax(a.loss_all[r]) if (~np.isnan(a.loss_all[r])).any() else -np.inf
                    seen["nan_would_rank_first"] |= bool(tail > best > -np.inf)
    assert all(seen.values()), seen
    assert set(C.WINNER_LENGTHS) <= lengths and max(lengths) > 256 * 4, sorted(lengths)
    assert {1, 2, 4, 5, 8, 16} <= set(C.TOPS) == {c.top for c in CASES}
    assert {1, 4, 8, 16} <= at_width and {2, 5, 9, 16} <= below_width, (at_width, below_width)
    # the select kernel's second and third batch of 2,048 columns hold winners; one-element splits
    assert C.case("K2049").h.K == 2049 and C.twin("K2049")[0].idx[0, 0] == 2048
    assert C.case("K4100").h.K == 4100 and C.twin("K4100")[0].idx[:, 0].tolist() == [4099, 4097]
    assert (C.twin("K4100")[0].idx[0] >= 0).all() and 2048 in C.twin("K4100")[0].idx[0]
    assert any(c.h.R == 2049 and c.h.K == 1 for c in CASES)


def test_a_count_is_not_a_cost():
    """The planted winner order is not the order of tail_calls."""
    c = C.case("count_is_not_cost")
    for (_, _, score), a in zip(C.walk(c.name), C.twin(c.name)):
        order = np.argsort(-score.tail_calls[1], kind="stable")
        assert int(order[0]) == 0 and score.tail_calls[1, 0] >= 3 * score.tail_calls[1, 2]
        assert a.idx[1, 0] == 2 and a.loss[1, 0] >= 10 * max(a.loss[1, 1], 0.0)
        assert not (a.loss_all[0] > a.loss[1, 0] / 10).any()
    # per row the taken tails add up to the score's tail_ns
    iv = c.h.intervals[0]
    full = histograms.segment_history_attribution(iv.keys, iv.off, iv.lens, c.h.K, c.h.hist0, c.h.pm, 4)
    assert np.array_equal(full.tail_ns.sum(1), C.walk(c.name)[0][2].tail_ns)


def test_argument_checks():
    keys, off, lens = np.zeros(4, np.uint32), np.array([0, 2]), np.array([2, 2], np.int32)
    hist = np.zeros((1, 2, 240), np.uint32)
    for top in (0, 17, True, 1.5):
        with pytest.raises(ValueError, match="top"):
            histograms.segment_history_attribution(keys, off, lens, 2, hist, 950, top)
    for pm in (-1, 1001, 0.5):
        with pytest.raises(ValueError, match="permille"):
            histograms.segment_history_attribution(keys, off, lens, 2, hist, pm, 4)
    with pytest.raises(ValueError, match="R \\* K"):
        histograms.segment_history_attribution(keys, off, lens, 3, hist, 950, 4)
    with pytest.raises(ValueError, match="hist must have shape"):
        histograms.segment_history_attribution(keys, off, lens, 2, np.zeros((2, 2, 240), np.uint32), 950, 4)
    with pytest.raises(ValueError, match="hist_index"):
        histograms.segment_history_attribution(keys, off, lens, 2, hist, 950, 4, hist_index=[0, 2])
