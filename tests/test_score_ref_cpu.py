"""CPU: the plain scoring reference (tests/_score_ref.py) against what the project already
trusts -- the C oracle's kernel_ref / scores / score_partials / stragglers and
oracle_report.section_summary_torch_semantics -- on the seeded inputs the GPU tests use, and the
input conditions those GPU tests rely on, so that none of them can pass vacuously.

The oracle sums left to right; the reference sums exactly.  n non-negative terms added in any
order are within n * 2^-53 of the exact sum (relative), so the oracle's sums and scores are held
to the bounds the kernels are held to (_score_ref.sum_bound, score_rel_bound)."""
from fractions import Fraction

import numpy as np
import pytest

import _score_ref as R
import oracle as O
import oracle_report

KS = [1, 2, 255, 256, 257, 2047, 2048, 2049, 4097]


def _oracle_form(x):
    """The options the oracle has: a column filter, an explicit reference in column order with
    NaN for "none", a plain [R][K] float64 history."""
    K = x["med"].shape[1]
    ref = x["ref"][x["perm"]].copy()
    ref[~(ref >= 0)] = np.nan
    hist = np.ascontiguousarray(x["hist"][:, x["slot"]])
    assert hist.shape[1] == K
    return ref, hist


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows", [1, 3])
def test_scores_and_history_match_the_oracle(rows, K):
    x = R.score_inputs(rows, K, np.float32, seed=1000 * rows + K)
    ref, hist = _oracle_form(x)
    want = R.score_terms(x["num"], x["med"], x["avg"], col_valid=x["col_valid"], ref=ref, hist=hist)
    assert (want.w[want.elig] >= 0).all()  # (a): the bound is a relative one
    sr, si, mr, mi, _ = R.finish(want.partials)
    oh = hist.astype(np.float64)
    gr, gi = O.scores(x["num"], x["med"], x["avg"], col_valid=x["col_valid"], ref=ref, hist=oh)
    for got, exp, n in ((gr, sr, want.partials[:, 2]), (gi, si, want.partials[:, 5])):
        assert np.array_equal(np.isnan(got), n == 0) and np.array_equal(np.isnan(exp), n == 0)
        ok = n > 0
        assert (np.abs(got[ok] - exp[ok]) <= R.score_rel_bound(n[ok]) * np.abs(exp[ok])).all()
    assert np.array_equal(oh, want.new_hist.astype(np.float64))  # the new history, exactly
    assert np.array_equal(O.stragglers(sr, 0.75).astype(bool), mr)
    assert np.array_equal(O.stragglers(si, 0.75).astype(bool), mi)


@pytest.mark.parametrize("K", [1, 257, 2049])
def test_partials_match_the_oracle_shard_by_shard(K):
    x = R.score_inputs(3, K, np.float32, seed=3000 + K)
    ref, hist = _oracle_form(x)
    shard = np.arange(K) % 3
    for g in range(3):
        mask = (shard == g).astype(np.uint8)
        want = R.score_terms(x["num"], x["med"], x["avg"], col_valid=mask, ref=ref, hist=hist)
        got = O.score_partials(x["num"], x["med"], x["avg"], ref, col_in_shard=mask,
                               hist=hist.astype(np.float64))
        p = want.partials
        assert np.array_equal(got[:, [2, 5]], p[:, [2, 5]])  # counts: exact
        for base in (0, 3):
            n = p[:, base + 2]
            for i in (base, base + 1):
                assert (np.abs(got[:, i] - p[:, i]) <= R.sum_bound(n, p[:, i])).all()


@pytest.mark.parametrize("rows", [0, 1, 31, 32, 33, 300])
def test_kernel_ref_matches_the_oracle(rows):
    g = np.random.default_rng(rows)
    K = 257
    num = g.integers(1, 9, (rows, K)).astype(np.int32)
    num[g.random((rows, K)) < 0.01] = 0
    med = g.uniform(1, 100, (rows, K)).astype(np.float32)
    ref, _, missing = R.kernel_ref(num, med)
    assert R.same_bits(ref, O.kernel_ref(num, med))
    assert rows < 3 or 0 < missing.sum() < K  # both kinds of column


def test_stragglers_match_the_oracle():
    thr = 0.75
    s = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, thr, np.nextafter(thr, 0), np.nextafter(thr, 1)])
    assert np.array_equal(O.stragglers(s, thr).astype(bool), R.stragglers(s, thr))
    assert R.stragglers(s, thr).tolist() == [False, False, True, True, True, False, True, False]


def test_finalize_adds_shards_in_order():
    big, one = 2.0 ** 53, 1.0
    p = np.zeros((3, 1, 6))
    p[:, 0, 1] = (big, one, one)      # (big + 1) + 1 == big in float64; 1 + 1 + big would not
    p[:, 0, 0] = (big, 0, 0)
    p[:, 0, 2] = 1
    assert R.finalize(p, 3)[0][0] == 1.0
    assert R.finalize(p[::-1], 3)[0][0] == big / (big + 2)


@pytest.mark.parametrize("n", [1, 2, 5, 1000, 8193])
def test_section_stats_match_torch_semantics(n):
    for name, v in R.section_patterns(n, seed=n).items():
        want, trust = R.section_stats(v), oracle_report.section_summary_torch_semantics(list(v))
        assert want["num"] == trust["NUM"] == n
        for a, b in (("min", "MIN"), ("max", "MAX"), ("med", "MED")):
            assert want[a] == trust[b], (name, a)
        if name in R.WELL_CONDITIONED:
            assert want["avg"] == pytest.approx(trust["AVG"], rel=1e-14), name
            assert n == 1 or want["std"] == pytest.approx(trust["STD"], rel=1e-12), name
        else:
            amax = np.abs(v).max()
            assert abs(want["avg"] - trust["AVG"]) <= n * R.EPS * amax
            assert n == 1 or abs(want["std"] - trust["STD"]) <= 4 * n * R.EPS * amax
        assert n > 1 or np.isnan(want["std"])
    assert R.section_stats([])["num"] == 0 and np.isnan(R.section_stats([])["avg"])


def test_section_scores_reference_by_hand():
    med = np.array([[2.0, 4.0, 1.0], [1.0, 8.0, 1.0]])
    present = np.array([[1, 1, 0], [1, 1, 1]], np.uint8)
    hist = np.array([[np.inf, 1.0, 5.0], [0.5, 16.0, 5.0]])
    rel, ind, new, zero = R.section_scores(med, present, hist=hist)
    assert R.same_bits(rel, np.array([[0.5, 1.0, np.nan], [1.0, 0.5, np.nan]]))
    assert R.same_bits(ind, np.array([[1.0, 0.25, np.nan], [0.5, 1.0, 1.0]]))
    assert R.same_bits(new, np.array([[2.0, 1.0, 5.0], [0.5, 8.0, 1.0]])) and not zero
    ref_in = np.array([-1.0, 3.0, np.nan], np.float32)
    rel, _, _, _ = R.section_scores(med, present, ref_in=ref_in,
                                    ref_index=np.array([1, 0, 2], np.int32), ind=False)
    assert R.same_bits(rel, np.array([[1.5, np.nan, np.nan], [3.0, np.nan, np.nan]]))


# ------------------------------------------------------------------ what the GPU tests rely on
def test_two_term_inputs_tell_a_fused_multiply_add_apart():
    """(b): in at least a quarter of the rows round(s1*w1 + t0) != round(round(s1*w1) + t0)."""
    x = R.two_term_inputs()
    num, med, avg = x["num"], x["med"], x["avg"]
    assert num.shape == (256, 2304) and ((num > 0).sum(1) == 2).all() and (avg >= 0).all()
    want = R.score_terms(num, med, avg, ref=x["ref"], hist=x["hist"])
    assert (want.partials[:, [2, 5]] == 2).all()
    for t in (want.t_rel, want.t_ind):
        differ = 0
        for r in range(256):
            c0, c1 = x["pairs"][r // 64]
            base = float(x["ref"][c1]) if t is want.t_rel else min(x["hist"][r, c1], med[r, c1])
            s1 = np.float64(base) / med[r, c1]
            unfused = (s1 * want.w[r, c1]) + t[r, c0]
            assert unfused == t[r, c1] + t[r, c0]
            fused = float(Fraction(float(s1)) * Fraction(float(want.w[r, c1])) + Fraction(float(t[r, c0])))
            differ += fused != unfused
        assert differ >= 64, differ


def test_rounding_order_row_separates_mask_before_and_after_rounding():
    """(c): score < thr and float32(score) >= thr."""
    x = R.rounding_order_row()
    want = R.score_terms(x["num"], x["med"], x["avg"], hist=x["hist"])
    _, si, _, mi, _ = R.finish(want.partials, thr_ind=x["thr"])
    assert si[0] < x["thr"] and mi[0] and np.float32(si[0]) >= x["thr"]
    _, s32, _, m32, _ = R.finish(want.partials, thr_ind=x["thr"], round_f32=True)
    assert s32[0] == 0.75 and not m32[0]
