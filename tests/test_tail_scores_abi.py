"""CPU: the tail-score entry points are exported and bound, their host-side argument checks run
before any launch (NVRX_ERR_INVALID with a message naming the argument), and the numpy helpers
``histograms.tail_threshold`` / ``tail_scores`` equal the definition written in plain Python
integers (``_tail_ref``): integers equal, f64 bit patterns equal, no tolerance."""
import ctypes
import re

import numpy as np
import pytest

import _tail_ref as REF
from nvidia_resiliency_ext.straggler import _native, histograms, ops

NAMES = ("nvrx_histogram_sum", "nvrx_histogram_tail_threshold", "nvrx_histogram_tail_scores")
BINS = 240
PMS = (0, 500, 990, 999, 1000)


def _invalid(rc, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error()
    assert re.search(word, msg.decode()), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def _sum(counts=16, R=1, K=1, acc=0, fleet=16):
    return _native.lib().nvrx_histogram_sum(counts, R, K, acc, fleet, None)


def _thr(fleet=16, K=1, pm=990, col_valid=None, thr=16, sums=16):
    return _native.lib().nvrx_histogram_tail_threshold(fleet, K, pm, col_valid, thr, sums, None)


def _scores(**kw):
    f = dict(R=1, K=1, counts=16, thr=16, thr_index=None, fleet_sums=16, tail_ns=16, total_ns=16,
             score=16, tail_calls=None, strag=None, score_thr=0.75)
    f.update(kw)
    a = _native.TailArgs(*(f[n] for n, _ in _native.TailArgs._fields_))
    return _native.lib().nvrx_histogram_tail_scores(ctypes.byref(a), None)


def test_symbols_loaded_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in _native.SIGNATURES
        assert getattr(L, n).argtypes == _native.SIGNATURES[n][1]
    assert L.nvrx_abi_version() == _native.ABI_VERSION == 6  # additive
    # the struct mirrors the header: 2 i64, 9 pointers, 1 f64
    assert ctypes.sizeof(_native.TailArgs) == 12 * 8
    for n in ("histogram_sum", "histogram_tail_threshold", "histogram_tail_scores"):
        assert callable(getattr(ops, n))


def test_bad_sum_arguments():
    _invalid(_sum(counts=None), "counts")
    _invalid(_sum(fleet=None), "fleet")
    _invalid(_sum(counts=20), "counts")  # not 16-byte aligned
    _invalid(_sum(fleet=24), "fleet")
    _invalid(_sum(R=-1), "R")
    _invalid(_sum(K=-1), "K")
    _invalid(_sum(K=(1 << 31) // 240 + 1), r"K \* 240")
    _invalid(_sum(R=1 << 20, K=1 << 12), r"R \* K")


def test_bad_threshold_arguments():
    _invalid(_thr(fleet=None), "fleet")
    _invalid(_thr(fleet=24), "fleet")
    _invalid(_thr(thr=None), "thr")
    _invalid(_thr(sums=None), "fleet_sums")
    _invalid(_thr(K=-1), "K")
    _invalid(_thr(K=(1 << 31) // 240 + 1), r"K \* 240")
    for pm in (-1, 1001):
        _invalid(_thr(pm=pm), "permille")


def test_bad_scores_arguments():
    _invalid(_native.lib().nvrx_histogram_tail_scores(None, None), "args")
    for n in ("counts", "thr", "fleet_sums", "tail_ns", "total_ns", "score"):
        _invalid(_scores(**{n: None}), n)
    _invalid(_scores(counts=20), "counts")
    _invalid(_scores(R=-1), "R")
    _invalid(_scores(K=-1), "K")
    _invalid(_scores(K=(1 << 31) // 240 + 1), r"K \* 240")
    _invalid(_scores(R=1 << 20, K=1 << 12), r"R \* K")


def test_empty_shapes_launch_nothing():
    # R == 0 or K == 0: OK without touching the device (null arrays allowed)
    assert _sum(counts=None, R=0, fleet=None) == _native.NVRX_OK
    assert _sum(counts=None, K=0, fleet=None) == _native.NVRX_OK
    assert _thr(fleet=None, K=0, thr=None, sums=None) == _native.NVRX_OK
    assert _scores(R=0, counts=None, score=None) == _native.NVRX_OK
    assert _scores(K=0, counts=None, thr=None) == _native.NVRX_OK


def test_ops_wrappers_check_before_any_tensor():
    with pytest.raises(ValueError, match="accumulate"):
        ops.histogram_sum(None, accumulate=True)
    for bad in (-1, 1001, 0.5, True):
        with pytest.raises(ValueError, match="permille"):
            ops.histogram_tail_threshold(None, bad)
        with pytest.raises(ValueError, match="permille"):
            histograms.tail_threshold(np.zeros((1, BINS), np.int64), bad)


# ---------------------------------------------------------------- the numpy helpers
def _random_counts(rng, R, K, hi=1000):
    c = rng.integers(0, hi, size=(R, K, BINS), dtype=np.uint64)
    return (c * (rng.random((R, K, BINS)) < 0.1)).astype(np.uint32)


def _cases():
    rng = np.random.default_rng(2401)
    out = {"random": _random_counts(rng, 5, 7)}
    c = _random_counts(rng, 3, 4)
    c[:, 2] = 0  # N_k = 0
    c[1] = 0     # a row without samples
    out["zero_column_and_row"] = c
    c = np.zeros((2, 2, BINS), np.uint32)
    c[:, :, 0] = (3, 9)  # weight 0 only: fleet_total == 0
    out["bucket0_only"] = c
    c = np.zeros((3, 3, BINS), np.uint32)
    c[0, 0, 237], c[1, 0, 238], c[2, 0, 239] = 5, 6, 7
    c[:, 1, 239] = 4  # a fleet entirely in bucket 239: T = 239, no tail
    c[:, 2, 100], c[2, 2, 238] = 50, 1
    out["wide_buckets"] = c
    c = np.zeros((3, 2, BINS), np.uint32)
    c[:, 0, 120], c[:, 0, 130], c[0, 1, 60], c[2, 1, 61] = 0xFFFFFFFF, 0xFFFFFFFF, 0x80000000, 0xFFFFFFFF
    out["full_u32"] = c
    # sums above 2^53: the u64 -> f64 rounding shows (odd low bits survive in the integers)
    c = np.zeros((2, 3, BINS), np.uint32)
    c[0, 0, 230], c[1, 0, 231], c[0, 1, 9], c[1, 1, 11], c[:, 2, 236] = 0xFFFFFFFF, 0xFFFFFFFD, 1, 3, 0xFFFFFFF1
    out["above_2_53"] = c
    return out


CASES = _cases()


def _check(c, pm, col_valid=None):
    lists = c.view(np.uint32).tolist()  # an int32 view holds u32 counts
    F, T, sums, rows = REF.full(lists, pm, 0.75, col_valid)
    got_T = histograms.tail_threshold(np.asarray(F, dtype=object).astype(np.uint64), pm)
    plain_T, _ = REF.threshold(F, pm)
    assert got_T.dtype == np.int64 and got_T.tolist() == plain_T
    g = histograms.tail_scores(c, pm, col_valid=col_valid)
    assert g.threshold_bucket.tolist() == T
    assert (g.fleet_tail, g.fleet_total) == sums
    assert g.tail_ns.dtype == np.uint64 and g.tail_ns.tolist() == [r["tail_ns"] for r in rows]
    assert g.total_ns.tolist() == [r["total_ns"] for r in rows]
    assert [REF.bits(s) for s in g.score] == [REF.bits(r["score"]) for r in rows]
    assert g.tail_calls.tolist() == [r["calls"] for r in rows]
    fs = float(sums[0]) / float(sums[1]) if sums[1] else float("nan")
    assert REF.bits(g.fleet_share) == REF.bits(fs)
    return g, rows


@pytest.mark.parametrize("pm", PMS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_helpers_equal_the_python_integer_reference(name, pm):
    c = CASES[name]
    _check(c, pm)
    _check(c.view(np.int32), pm)  # device counts come as int32


def test_numpy_helpers_col_valid():
    c = CASES["random"]
    valid = [1, 0, 1, 1, 0, 1, 1]
    g, _ = _check(c, 990, valid)
    assert [t < 0 for t in g.threshold_bucket] == [not v for v in valid]


def test_properties_of_the_definition():
    # pm = 1000: T is the fleet's highest occupied bucket, no tail, every score exactly 1.0
    g, _ = _check(CASES["random"], 1000)
    assert g.tail_ns.tolist() == [0] * 5 and g.score.tolist() == [1.0] * 5 and g.fleet_share == 0.0
    # weight-0 samples only: NaN everywhere, nothing flagged
    g, rows = _check(CASES["bucket0_only"], 500)
    assert all(s != s for s in g.score) and not any(r["strag"] for r in rows)
    # a fleet in bucket 239 alone has T = 239
    g, _ = _check(CASES["wide_buckets"], 0)
    assert g.threshold_bucket[1] == 239
    # the rounding of u64 -> f64 is visible: the integers are not representable
    g, _ = _check(CASES["above_2_53"], 500)
    assert g.fleet_total > 2 ** 53 and float(g.fleet_total) != g.fleet_total


@pytest.mark.parametrize("pm", PMS)
def test_threshold_is_the_bucket_quantile_bounds_brackets(pm):
    us = histograms.edges_us()
    for name, c in CASES.items():
        F = histograms.merge(c).sum(0)
        T = histograms.tail_threshold(F, pm)
        for k in range(F.shape[0]):
            lo, hi = histograms.quantile_bounds(F[k], pm)
            if T[k] < 0:
                assert lo != lo and hi != hi, (name, k)
            else:
                assert (lo, hi) == (float(us[T[k]]), float(us[T[k] + 1])), (name, k)
