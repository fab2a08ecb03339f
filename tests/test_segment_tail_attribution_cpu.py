"""CPU: ``histograms.segment_tail_attribution`` -- the host twin of the tail score attribution
straight from ragged segments -- is ``tail_attribution`` over ``segment_counts`` field by field on
every case; the case list reaches what it is aimed at; and on record-like segments the twin names
the kernel that costs a rank its tail score where the count of tail calls names a cheap one."""
from fractions import Fraction

import numpy as np
import pytest

import _segment_tail_attr_cases as C
from nvidia_resiliency_ext.straggler import histograms

FIELDS = ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share", "loss_all")
CASES = C.cases()


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype == np.float64:
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), what  # every NaN is "not taken": one pattern
        got, want = got.view(np.uint64)[~gn], want.view(np.uint64)[~wn]
    assert np.array_equal(got, want), what


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_twin_is_tail_attribution_over_segment_counts(c):
    s = c.seg
    counts = histograms.segment_counts(s.keys, s.off, s.lens, s.K, s.cap)
    want = histograms.tail_attribution(counts, s.pm, c.top, s.col_valid, thr_index=s.thr_index)
    got = C.twin(c.name)
    for f in FIELDS:
        same_bits(getattr(got, f), getattr(want, f), f)
    assert got.idx.shape == (s.R, c.top) and got.loss_all.shape == (s.R, s.K)


@pytest.mark.parametrize("c", [c for c in CASES if c.planted], ids=lambda c: c.name)
def test_planted_winners_sit_where_the_case_says(c):
    a = C.twin(c.name)
    for (r, j), k in c.planted.items():
        assert a.idx[r, j] == k, (r, j, a.idx[r])


def test_the_inherited_cases_reach_their_branches():
    """What the cases of ``_segment_tail_cases`` give under top 16."""
    taken, ties, lengths = set(), 0, set()
    seen = dict(negative=False, trimmed=False, skipped=False, no_index=False)
    for c in CASES[:len(C.S.cases())]:
        a, s = C.twin(c.name), c.seg
        assert c.top == 16
        n_taken = (~np.isnan(a.loss_all)).sum(1)
        taken |= set(n_taken.tolist())
        for r in range(s.R):
            v = a.loss_all[r][~np.isnan(a.loss_all[r])]
            ties = max(ties, v.size - np.unique(v).size)  # losses equal to an earlier column's
            for k in a.idx[r][a.idx[r] >= 0]:
                n = int(s.lens[r * s.K + k])
                lengths.add(min(n, s.cap) if s.cap else n)
                seen["trimmed"] |= bool(s.cap and n > s.cap)
        seen["negative"] |= bool((a.loss < 0).any())
        seen["skipped"] |= bool(s.col_valid is not None and np.isnan(a.loss_all[:, s.col_valid == 0]).all()
                                and (s.col_valid == 0).any())
        seen["no_index"] |= bool(s.thr_index is not None and np.isnan(a.loss_all[:, s.thr_index < 0]).all())
    assert {0, 1, 1800} <= taken and set(range(3, 34)) & taken, sorted(taken)
    assert ties >= 1789, ties                      # R1_K2048: a row of tied losses
    assert {1, 1025} <= lengths and any(n <= 16 for n in lengths) and any(n > 16 for n in lengths)
    assert all(seen.values()), seen
    # ties go to the lower column: a row's columns of equal loss are in increasing order
    a = C.twin("R1_K2048")
    eq = a.loss[0, 1:] == a.loss[0, :-1]
    assert eq.any() and (np.diff(a.idx[0])[eq] > 0).all()
    # all four starts inside a 16-byte vector among the winners
    s = C.case("lengths_unaligned").seg
    a = C.twin("lengths_unaligned")
    starts = {int(s.off[r * s.K + k] + s.lens[r * s.K + k] - min(s.lens[r * s.K + k], s.cap or 1 << 30)) % 4
              for r in range(s.R) for k in a.idx[r] if k >= 0}
    assert starts == {0, 1, 2, 3}


def test_the_added_cases_reach_what_they_are_aimed_at():
    assert {c.top for c in CASES} >= {1, 3, 4, 5, 8, 9, 16}
    a = C.twin("K2100_second_batch")
    assert C.case("K2100_second_batch").seg.K > 2048 and (a.idx[0, :2] >= 2048).any()
    for name in ("long_winner_cap0", "long_winner_cap3000"):
        s = C.case(name).seg
        assert C.twin(name).idx[0, 0] == 1 and s.lens[1] == 4100
        assert min(4100, s.cap or 4100) > 256 * 4 and s.cap in (0, 3000)
    a = C.twin("only_negative_losses")
    assert (a.idx[0, :4] >= 0).all() and (a.loss[0, :4] < 0).all() and (a.loss[1, :4] > 0).all()
    assert (a.idx[:, 4] == -1).all() and np.isnan(a.loss[:, 4]).all() and np.isnan(a.base_share[:, 4]).all()
    assert not a.tail_ns[:, 4].any() and not a.total_ns[:, 4].any() and not a.tail_calls[:, 4].any()
    assert (a.thr_bucket[:, 4] == -1).all()
    a = C.twin("exactly_top_and_one_less")
    assert (a.idx[0] >= 0).all() and (~np.isnan(a.loss_all[0])).sum() == 9
    assert (a.idx[1, :8] >= 0).all() and a.idx[1, 8] == -1 and (~np.isnan(a.loss_all[1])).sum() == 8
    a = C.twin("fewer_than_top16")
    assert (a.idx >= 0).sum(1).tolist() == [3, 1] and (a.idx[0, 3:] == -1).all()
    a = C.twin("duplicated_columns")
    assert a.idx[0, :2].tolist() == [2, 4] and a.loss[0, 0] == a.loss[0, 1] and a.loss[0, 0] != 0.0
    for r in range(3):  # the pair ties in every row, the lower column first wherever both are listed
        assert a.loss_all[r, 2] == a.loss_all[r, 4]
        at = {int(k): j for j, k in enumerate(a.idx[r]) if k in (2, 4)}
        assert len(at) < 2 or at[2] + 1 == at[4]
    a = C.twin("column_in_one_row")
    assert np.isnan(a.loss_all[[0, 2], 2]).all() and not np.isnan(a.loss_all[1, 2])


def test_a_contracted_multiply_subtract_could_not_pass():
    """Over the winners of all cases, tail - total * share rounded after each operation differs
    somewhere from the same expression rounded once (what a fused multiply-subtract gives)."""
    differs = 0
    for c in CASES:
        a = C.twin(c.name)
        for r, j in zip(*np.nonzero(a.idx >= 0)):
            tail, total, share = int(a.tail_ns[r, j]), int(a.total_ns[r, j]), float(a.base_share[r, j])
            assert tail < 1 << 53 and total < 1 << 53   # both convert to f64 exactly
            exact = Fraction(tail) - Fraction(total) * Fraction(share)
            fused = exact.numerator / exact.denominator  # int / int: correctly rounded
            separate = float(tail) - float(total) * share
            assert a.loss[r, j] == separate
            differs += fused != separate
    assert differs > 0


def scenario():
    """8 ranks x 6 kernels as segments; kernel 0 is cheap, jittery and called often; rank 5's
    kernel 3 (2 ms) is 2x slower on every 16th call."""
    bases = [5_000, 200_000, 200_000, 2_000_000, 200_000, 200_000]
    calls = [4096, 256, 256, 64, 256, 256]
    jitter = [0.10, 0.02, 0.02, 0.02, 0.02, 0.02]
    rng = np.random.default_rng(7)
    keys, lens = [], []
    for r in range(8):
        for k in range(6):
            d = bases[k] * (1.0 + jitter[k] * rng.standard_normal(calls[k]))
            if r == 5 and k == 3:
                d[::16] *= 2
            keys.append(d.astype(np.uint32))
            lens.append(calls[k])
    lens = np.asarray(lens, np.int32)
    off = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    return np.concatenate(keys), off, lens


def test_a_count_is_not_a_cost_for_segments():
    keys, off, lens = scenario()
    s = histograms.segment_tail_scores(keys, off, lens, 6, 950)
    a = histograms.segment_tail_attribution(keys, off, lens, 6, 950, 6)
    assert int(np.argmin(s.score)) == 5 and s.score[5] < 0.97 and np.delete(s.score, 5).min() > 1.0
    order = np.argsort(-s.tail_calls[5], kind="stable")
    assert int(order[0]) == 0                          # by tail calls the cheap, jittery kernel leads
    assert s.tail_calls[5, 0] >= 5 * s.tail_calls[5, 3]
    assert a.idx[5, 0] == 3                            # by excess tail time the 2 ms kernel does
    assert a.loss[5, 0] >= 10 * max(a.loss[5, 1], 0.0)
    for r in range(8):
        if r != 5:
            assert not (a.loss_all[r] > a.loss[5, 0] / 10).any(), r
    # per row the taken tails add up to the score's tail_ns
    assert np.array_equal(a.tail_ns.sum(1), s.tail_ns)


def test_argument_checks():
    keys, off, lens = np.zeros(4, np.uint32), np.array([0, 2]), np.array([2, 2], np.int32)
    for top in (0, 17, True, 1.5):
        with pytest.raises(ValueError, match="top"):
            histograms.segment_tail_attribution(keys, off, lens, 2, 950, top)
    with pytest.raises(ValueError, match="permille"):
        histograms.segment_tail_attribution(keys, off, lens, 2, 1001, 4)
    with pytest.raises(ValueError, match="R \\* K"):
        histograms.segment_tail_attribution(keys, off, lens, 3, 950, 4)
