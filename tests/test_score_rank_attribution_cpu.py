"""The host twins ``histograms.score_losses`` / ``score_rank_attribution`` (no GPU).

``score_losses`` against a brute-force loop in Python floats (IEEE doubles, one operation per
statement) over the eligibility table; ``score_rank_attribution`` as ``rank_attribution`` of those
losses plus the winners' s; and the two directions of the attribution list the same elements.
Every comparison is an equality: integers, and f64 as bits."""
import numpy as np
import pytest

from _score_ref import inputs
from nvidia_resiliency_ext.straggler import histograms

NAN = float("nan")


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def bit(x):
    return int(np.float64(x).view(np.uint64))


def same(a, b):
    """Equal bit for bit, any NaN matching any NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(b)
    return (a.shape == b.shape and np.array_equal(np.isnan(a), nan) and
            np.array_equal(bits(a[~nan]), bits(b[~nan])))


def brute(num, med, avg, kind, col_valid=None, ref=None, ref_index=None, ref_missing=None,
          hist=None, hist_index=None, hist_stride=0, rows=None):
    R, K = med.shape
    loss = np.full((R, K), NAN)
    s_all = np.full((R, K), NAN)
    err = 0
    for r in range(R):
        for k in range(K):
            elig = int(num[r, k]) > 0 and (col_valid is None or col_valid[k] != 0)
            if kind == "relative":
                ri = k if ref_index is None else int(ref_index[k])
                rf = float(ref[ri])
                elig = elig and rf >= 0 and not (ref_missing is not None and ref_missing[ri] != 0)
                base = rf
            else:
                hi = k if hist_index is None else int(hist_index[k])
                base = float(hist.reshape(-1)[r * (hist_stride or K) + hi])
            m = float(med[r, k])
            w = float(int(num[r, k])) * float(avg[r, k])
            s = base / m if m != 0.0 else NAN  # never taken at MED == 0: its s is not compared
            d = 1.0 - s
            ls = w * d
            s_all[r, k] = s
            if elig and m == 0.0 and (rows is None or rows[r]):
                err = 1
            if elig and m != 0.0 and ls == ls:
                loss[r, k] = ls
    return loss, s_all, err


def table():
    """One element per rule, 2 rows x 10 columns, relative kind; row 1 is plain."""
    K = 10
    num = np.full((2, K), 3, np.int32)
    med = np.full((2, K), 2.0)
    avg = np.full((2, K), 5.0)
    ref = np.ones(K, np.float32)
    col_valid = np.ones(K, np.uint8)
    missing = np.zeros(K, np.uint32)
    col_valid[0] = 0               # filtered column
    num[0, 1] = 0                  # absent kernel
    ref[2] = -1.0                  # no reference
    ref[3] = np.nan
    missing[4] = 1                 # flagged missing
    med[0, 5] = 0.0                # eligible MED == 0: err, not taken
    avg[0, 6] = np.nan             # NaN loss
    avg[0, 7] = -5.0               # negative AVG at s = 1: loss -0.0
    med[0, 7] = 1.0
    num[0, 8] = -2                 # <= 0 is absent too
    return dict(num=num, med=med, avg=avg), dict(ref=ref, col_valid=col_valid, ref_missing=missing)


def test_the_eligibility_table():
    x, base = table()
    loss, s, err = histograms.score_losses(x["num"], x["med"], x["avg"], "relative", **base)
    wl, ws, werr = brute(x["num"], x["med"], x["avg"], "relative", **base)
    assert same(loss, wl) and err == werr == 1
    take = ~np.isnan(wl)
    assert same(s[take], ws[take])
    assert np.isnan(loss[0, [0, 1, 2, 3, 4, 5, 6, 8]]).all() and np.isnan(loss[1, [0, 2, 3, 4]]).all()
    assert loss[0, 7] == 0.0 and np.signbit(loss[0, 7]) and s[0, 7] == 1.0
    assert loss[0, 9] == 7.5 and s[0, 9] == 0.5
    # MED == 0 on an element that is not eligible: no error
    x["num"][0, 5] = 0
    assert histograms.score_losses(x["num"], x["med"], x["avg"], "relative", **base)[2] == 0
    # ... and in a row that is off: no error either, the other row's is seen
    x["num"][0, 5] = 3
    assert histograms.score_losses(x["num"], x["med"], x["avg"], "relative", rows=[0, 1], **base)[2] == 0
    assert histograms.score_losses(x["num"], x["med"], x["avg"], "relative", rows=[1, 0], **base)[2] == 1


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("R,K", [(1, 1), (5, 7), (16, 16), (33, 9)])
def test_score_losses_against_the_loop(dt, R, K):
    x = inputs(R, K, dt, seed=100 * R + K)
    x["med"][R // 2, K // 2] = 0.0
    x["avg"][0, K - 1] = np.nan
    for kind, kw in (("relative", dict(col_valid=x["col_valid"], ref=x["ref"], ref_index=x["perm"],
                                       ref_missing=x["missing"])),
                     ("relative", dict(ref=x["ref"])),
                     ("individual", dict(col_valid=x["col_valid"], hist=x["hist"],
                                         hist_index=x["slot"], hist_stride=x["stride"])),
                     ("individual", dict(hist=np.ascontiguousarray(x["hist"][:, :K])))):
        loss, s, err = histograms.score_losses(x["num"], x["med"], x["avg"], kind, **kw)
        wl, ws, werr = brute(x["num"], x["med"], x["avg"], kind, **kw)
        assert loss.dtype == np.float64 and same(loss, wl) and err == werr, (kind, sorted(kw))
        take = ~np.isnan(wl)
        assert same(s[take], ws[take])


@pytest.mark.parametrize("top", [1, 3, 16])
def test_rank_attribution_of_the_losses(top):
    R, K = 23, 11
    x = inputs(R, K, np.float32, seed=3)
    x["med"][4, 2] = 0.0
    x["num"][4, 2] = 9
    x["col_valid"][2] = 1
    rows = (np.arange(R) % 4 != 1).astype(np.uint8)
    for kind, kw in (("relative", dict(col_valid=x["col_valid"], ref=x["ref"], ref_index=x["perm"],
                                       ref_missing=x["missing"])),
                     ("individual", dict(col_valid=x["col_valid"], hist=x["hist"],
                                         hist_index=x["slot"], hist_stride=x["stride"]))):
        for rw in (None, rows):
            got = histograms.score_rank_attribution(x["num"], x["med"], x["avg"], top, kind, rows=rw, **kw)
            loss, s, err = histograms.score_losses(x["num"], x["med"], x["avg"], kind, rows=rw, **kw)
            want = histograms.rank_attribution(loss, top, rw)
            assert np.array_equal(got.idx, want.idx) and same(got.loss, want.loss)
            assert np.array_equal(got.taken, want.taken) and np.array_equal(got.positive, want.positive)
            assert got.err == err
            for k in range(K):
                for j in range(top):
                    r = got.idx[k, j]
                    assert np.isnan(got.score[k, j]) if r < 0 else \
                        bit(got.score[k, j]) == bit(s[r, k])
    with pytest.raises(ValueError, match="top"):
        histograms.score_rank_attribution(x["num"], x["med"], x["avg"], 17, "relative", ref=x["ref"])
    with pytest.raises(ValueError, match="kind"):
        histograms.score_losses(x["num"], x["med"], x["avg"], "sections")
    with pytest.raises(ValueError, match="ref"):
        histograms.score_losses(x["num"], x["med"], x["avg"], "relative")
    with pytest.raises(ValueError, match="hist"):
        histograms.score_losses(x["num"], x["med"], x["avg"], "individual")


@pytest.mark.parametrize("R,K", [(16, 16), (7, 13), (1, 5)])
def test_both_directions_list_the_same_elements(R, K):
    """top = 16 >= R, K: the per-row sort of loss_all and the per-column result both list every
    taken element."""
    x = inputs(R, K, np.float64, seed=R + K)
    kw = dict(col_valid=x["col_valid"], ref=x["ref"], ref_index=x["perm"], ref_missing=x["missing"])
    loss, s, _ = histograms.score_losses(x["num"], x["med"], x["avg"], "relative", **kw)
    by_row = set()
    for r in range(R):
        take = np.nonzero(~np.isnan(loss[r]))[0]
        for k in take[np.argsort(-loss[r, take], kind="stable")][:16]:
            by_row.add((r, int(k), bit(loss[r, k])))
    got = histograms.score_rank_attribution(x["num"], x["med"], x["avg"], 16, "relative", **kw)
    by_col = {(int(got.idx[k, j]), k, bit(got.loss[k, j]))
              for k in range(K) for j in range(16) if got.idx[k, j] >= 0}
    assert by_row == by_col and len(by_col) == int(got.taken.sum()) == int((~np.isnan(loss)).sum())
