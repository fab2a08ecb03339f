"""CPU: ``histograms.rank_attribution`` -- the host twin of nvrx_rank_attribution -- against a
brute-force loop that follows the definition (include/nvrx_straggler.h, "Rank attribution") word
for word, on hand-made columns.  Every comparison is equality: integers, and f64 as bit patterns."""
import numpy as np
import pytest

from nvidia_resiliency_ext.straggler import histograms

NAN, INF = float("nan"), float("inf")


def brute(loss, top, rows=None):
    """Per column: pick, `top` times, the taken element not yet picked with the largest value,
    the lowest row among equals (-0.0 == +0.0 in Python as in IEEE)."""
    x = np.asarray(loss, np.float64)
    R, K = x.shape
    idx = np.full((K, top), -1, np.int32)
    out = np.full((K, top), np.nan)
    taken, positive = np.zeros(K, np.int32), np.zeros(K, np.int32)
    for k in range(K):
        left = [r for r in range(R) if x[r, k] == x[r, k] and (rows is None or rows[r])]
        taken[k] = len(left)
        positive[k] = sum(1 for r in left if x[r, k] > 0.0)
        for j in range(top):
            if not left:
                break
            best = left[0]
            for r in left[1:]:
                if x[r, k] > x[best, k]:
                    best = r
            left.remove(best)
            idx[k, j] = best
            out[k, j] = x[best, k]
    return idx, out, taken, positive


def same(res, ref):
    idx, out, taken, positive = ref
    assert res.idx.dtype == np.int32 and res.taken.dtype == np.int32 and res.positive.dtype == np.int32
    assert np.array_equal(res.idx, idx)
    assert np.array_equal(res.loss.view(np.uint64), out.view(np.uint64))
    assert np.array_equal(res.taken, taken)
    assert np.array_equal(res.positive, positive)


def check(cols, top, rows=None):
    x = np.array(cols, np.float64).T.copy()  # a list of columns -> [R, K]
    res = histograms.rank_attribution(x, top, rows)
    same(res, brute(x, top, rows))
    return res


def test_all_nan():
    res = check([[NAN] * 5], 3)
    assert res.idx.tolist() == [[-1, -1, -1]] and res.taken.tolist() == [0] and res.positive.tolist() == [0]
    assert np.isnan(res.loss).all()


def test_all_equal_gives_the_first_rows():
    for top in (1, 4, 7):
        res = check([[2.5] * 9], top)
        assert res.idx[0].tolist() == list(range(top))
        assert res.taken.tolist() == [9] and res.positive.tolist() == [9]


def test_signed_zeros_tie_and_keep_their_bits():
    res = check([[-0.0, 0.0, -0.0, 0.0], [0.0, -0.0, -1.0, -0.0]], 4)
    assert res.idx.tolist() == [[0, 1, 2, 3], [0, 1, 3, 2]]
    assert np.signbit(res.loss[0]).tolist() == [True, False, True, False]
    assert np.signbit(res.loss[1]).tolist() == [False, True, True, True]
    assert res.positive.tolist() == [0, 0] and res.taken.tolist() == [4, 4]


def test_infinities_and_negatives_order_like_values():
    res = check([[-INF, 3.0, INF, NAN, -2.0, INF], [-5.0, -INF, -1.0, -1.0, NAN, -7.0]], 6)
    assert res.idx.tolist() == [[2, 5, 1, 4, 0, -1], [2, 3, 0, 5, 1, -1]]
    assert res.positive.tolist() == [3, 0] and res.taken.tolist() == [5, 5]


def test_top_beyond_taken_pads():
    res = check([[NAN, 1.0, NAN, 4.0]], 16)
    assert res.idx[0].tolist() == [3, 1] + [-1] * 14
    assert np.isnan(res.loss[0, 2:]).all() and res.loss[0, :2].tolist() == [4.0, 1.0]


def test_fewer_rows_than_top():
    res = check([[1.0, 2.0], [NAN, NAN], [7.0, 7.0]], 8)
    assert res.idx[:, :2].tolist() == [[1, 0], [-1, -1], [0, 1]]
    assert (res.idx[:, 2:] == -1).all()


def test_rows_mask_out_the_would_be_winner():
    cols = [[1.0, 9.0, 3.0, NAN], [5.0, 8.0, 5.0, 6.0]]
    res = check(cols, 2, rows=np.array([1, 0, 1, 1], np.uint8))
    assert res.idx.tolist() == [[2, 0], [3, 0]]
    assert res.taken.tolist() == [2, 3]
    res = check(cols, 2, rows=np.zeros(4, bool))
    assert (res.idx == -1).all() and res.taken.tolist() == [0, 0] and res.positive.tolist() == [0, 0]


def test_random_columns_with_ties_and_nans():
    rng = np.random.default_rng(7)
    x = rng.integers(-3, 4, size=(37, 11)).astype(np.float64)
    x[rng.random(x.shape) < 0.3] = NAN
    x[x == 0.0] *= rng.choice([-1.0, 1.0], size=int((x == 0.0).sum()))
    rows = rng.random(37) < 0.8
    for top in (1, 5, 16):
        same(histograms.rank_attribution(x, top), brute(x, top))
        same(histograms.rank_attribution(x, top, rows), brute(x, top, rows))


def test_empty_shapes_and_refusals():
    res = histograms.rank_attribution(np.zeros((0, 3)), 2)
    assert res.idx.tolist() == [[-1, -1]] * 3 and res.taken.tolist() == [0, 0, 0]
    assert histograms.rank_attribution(np.zeros((4, 0)), 2).idx.shape == (0, 2)
    for bad in (0, 17, True, 1.5):
        with pytest.raises(ValueError, match="top"):
            histograms.rank_attribution(np.zeros((2, 2)), bad)
    with pytest.raises(ValueError, match="shape"):
        histograms.rank_attribution(np.zeros(3), 2)
    with pytest.raises(ValueError, match="rows"):
        histograms.rank_attribution(np.zeros((2, 2)), 2, rows=np.ones(3, bool))
