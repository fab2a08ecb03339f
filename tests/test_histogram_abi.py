"""CPU: the histogram entry points are exported and bound, the bucket scheme is the one the
header states (against Python integers), the host-side argument checks run before any launch
(NVRX_ERR_INVALID with a message naming the argument), and the numpy helpers of
``straggler.histograms`` agree with the C functions."""
import ctypes
import math
import re

import numpy as np
import pytest

from nvidia_resiliency_ext.straggler import _native, histograms, ops

NAMES = ("nvrx_histogram_bucket", "nvrx_histogram_edge", "nvrx_segment_histogram_strided",
         "nvrx_segment_histogram_ragged", "nvrx_profiler_get_histograms")
BIG = (1 << 30) + 1  # above NVRX_MAX_SEGMENT
BINS = 240


def _bucket(x: int) -> int:
    if x < 8:
        return x
    e = x.bit_length() - 1
    return 8 * (e - 2) + ((x >> (e - 3)) & 7)


def _edge(b: int) -> int:
    return b if b < 8 else (8 + b % 8) << (b // 8 - 1)


EDGES = [_edge(b) for b in range(BINS + 1)]
SPECIAL = [0, 7, 8, 0xDFFFFFFF, 0xE0000000, 0xEFFFFFFF, 0xF0000000, 0xFFFFFFFF]


def _keys():
    rng = np.random.default_rng(240)
    k = EDGES[:BINS] + [e - 1 for e in EDGES[1:]] + SPECIAL
    return k + rng.integers(0, 1 << 32, size=100_000, dtype=np.uint64).tolist()


def _strided(ns=16, nseg=1, stride=8, begin=0, length=8, cap=0, acc=0, counts=16, num=None):
    return _native.lib().nvrx_segment_histogram_strided(ns, nseg, stride, begin, length, cap, acc,
                                                        counts, num, None)


def _ragged(ns=16, off=16, lens=None, nseg=1, max_len=8, cap=0, aligned16=0, acc=0, counts=16,
            num=None):
    return _native.lib().nvrx_segment_histogram_ragged(ns, off, lens, nseg, max_len, cap, aligned16,
                                                       acc, counts, num, None)


def _invalid(rc, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error()
    assert re.search(word, msg.decode()), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def test_symbols_loaded_and_bound():
    assert _native.HIST_BINS == BINS == histograms.BINS
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in _native.SIGNATURES
        assert getattr(L, n).argtypes == _native.SIGNATURES[n][1]
    assert L.nvrx_abi_version() == 6  # additive: no struct or signature changed


def test_bucket_and_edge_against_python_integers():
    L = _native.lib()
    for b in range(BINS + 1):
        assert L.nvrx_histogram_edge(b) == EDGES[b], b
    assert L.nvrx_histogram_edge(-1) == L.nvrx_histogram_edge(BINS + 1) == (1 << 64) - 1
    for x in _keys():
        assert L.nvrx_histogram_bucket(x) == _bucket(x), hex(x)


def test_edge_properties():
    L = _native.lib()
    assert all(EDGES[b] < EDGES[b + 1] for b in range(BINS))  # monotone
    assert EDGES[238] == _native.KEY_WIDE == histograms.KEY_WIDE
    assert EDGES[BINS] == 2 ** 32 and EDGES[0] == 0
    # every bucket from 8 up is exactly 1/8 of its octave's base wide: at most 12.5 % of its edge
    assert all(8 * (EDGES[b + 1] - EDGES[b]) <= EDGES[b] for b in range(8, BINS))
    keys = _keys()
    prev = -1
    for x in sorted(keys):
        b = L.nvrx_histogram_bucket(x)
        assert 0 <= b < BINS and b >= prev  # monotone in the key
        assert L.nvrx_histogram_edge(b) <= x < L.nvrx_histogram_edge(b + 1), hex(x)
        prev = b
    # buckets 238 and 239 hold exactly the wide keys
    assert L.nvrx_histogram_bucket(_native.KEY_WIDE - 1) == 237
    assert L.nvrx_histogram_bucket(_native.KEY_WIDE) == 238


def test_numpy_helpers_agree_with_the_c_functions():
    L = _native.lib()
    keys = _keys()
    got = histograms.bucket_of(np.asarray(keys, np.uint32))
    assert got.dtype == np.int64
    assert got.tolist() == [L.nvrx_histogram_bucket(x) for x in keys]
    ek = histograms.edges_keys()
    assert ek.dtype == np.uint64 and ek.shape == (BINS + 1,)
    assert ek.tolist() == [L.nvrx_histogram_edge(b) for b in range(BINS + 1)]
    us = histograms.edges_us()
    assert us.dtype == np.float32 and us.shape == (BINS + 1,) and us[BINS] == np.inf
    assert np.all(np.diff(us[:BINS].astype(np.float64)) > 0)
    # plain ns below the wide keys: the edge converted like every sample
    assert us[:238].tolist() == [np.float32(e) / np.float32(1000) for e in EDGES[:238]]
    assert us[238] == np.float32(float(_native.KEY_WIDE)) / np.float32(1000)  # 3.76 s
    # bucket 239 starts at key 0xF0000000: the f32 with KEY_WIDE_F32BITS + 0x10000000 as its bits
    b239 = np.array([_native.KEY_WIDE_F32BITS + 0x10000000], np.uint32).view(np.float32)[0]
    assert us[239] == b239 / np.float32(1000)
    with pytest.raises(ValueError):
        histograms.bucket_of(np.array([1 << 32], np.uint64))


def test_bad_strided_arguments():
    _invalid(_strided(counts=None), "counts")
    _invalid(_strided(counts=20), "counts")  # not 16-byte aligned
    _invalid(_strided(ns=None), "ns")
    _invalid(_strided(nseg=-1), "nseg")
    _invalid(_strided(length=-1), "seg_len")
    _invalid(_strided(begin=-1), "seg_begin")
    _invalid(_strided(stride=-1), "seg_stride")
    _invalid(_strided(nseg=1 << 31), "nseg")
    _invalid(_strided(length=BIG, stride=BIG), "NVRX_MAX_SEGMENT")
    _invalid(_strided(nseg=2, stride=4, length=8), "seg_stride")  # overlapping segments
    # a cap brings the retained length back in range: the check is on what is retained
    assert _strided(nseg=0, length=BIG, stride=BIG, cap=8192) == _native.NVRX_OK


def test_bad_ragged_arguments():
    _invalid(_ragged(counts=None), "counts")
    _invalid(_ragged(ns=None), "ns")
    _invalid(_ragged(off=None), "seg_off")
    _invalid(_ragged(nseg=-1), "nseg")
    _invalid(_ragged(max_len=-1), "max_len")
    _invalid(_ragged(nseg=1 << 31), "nseg")
    _invalid(_ragged(max_len=BIG), "NVRX_MAX_SEGMENT")


def test_zero_segments_launch_nothing():
    # nseg == 0: OK without touching the device (null arrays allowed)
    for acc in (0, 1):
        assert _strided(ns=None, nseg=0, counts=None, acc=acc) == _native.NVRX_OK
        assert _ragged(ns=None, off=None, nseg=0, counts=None, acc=acc) == _native.NVRX_OK


def test_profiler_get_histograms_arguments():
    L = _native.lib()
    cnt = ctypes.c_int64()
    _invalid(L.nvrx_profiler_get_histograms(None, 0, ctypes.byref(cnt), None, None, None), "handle")


def test_ops_wrappers_need_out_to_accumulate():
    # checked first: no tensor is looked at, so this runs without a GPU
    with pytest.raises(ValueError, match="accumulate"):
        ops.segment_histogram_strided(None, 1, 8, 0, 8, accumulate=True)
    with pytest.raises(ValueError, match="accumulate"):
        ops.segment_histogram_ragged(None, None, None, 8, accumulate=True)


def _counts(**bins):
    c = np.zeros(BINS, np.int64)
    for b, n in bins.items():
        c[int(b[1:])] = n
    return c


def test_quantile_bounds():
    us = histograms.edges_us()
    one = _counts(b100=17)
    for pm in (0, 1, 500, 999, 1000):
        assert histograms.quantile_bounds(one, pm) == (float(us[100]), float(us[101]))
    # 1 : 999 -- rank (pm * 999) // 1000 is 0 only for pm <= 1
    lo = _counts(b50=1, b120=999)
    assert histograms.quantile_bounds(lo, 0) == (float(us[50]), float(us[51]))
    assert histograms.quantile_bounds(lo, 1) == (float(us[50]), float(us[51]))
    assert histograms.quantile_bounds(lo, 2) == (float(us[120]), float(us[121]))
    assert histograms.quantile_bounds(lo, 1000) == (float(us[120]), float(us[121]))
    # 999 : 1 -- only the last rank (pm = 1000) reaches the upper bucket
    hi = _counts(b50=999, b120=1)
    assert histograms.quantile_bounds(hi, 999) == (float(us[50]), float(us[51]))
    assert histograms.quantile_bounds(hi, 1000) == (float(us[120]), float(us[121]))
    # the last bucket is open above
    assert histograms.quantile_bounds(_counts(b239=3), 500) == (float(us[239]), math.inf)
    assert all(math.isnan(v) for v in histograms.quantile_bounds(np.zeros(BINS, np.int64), 500))
    for bad in (-1, 1001, 0.5, True):
        with pytest.raises(ValueError, match="permille"):
            histograms.quantile_bounds(one, bad)
    # device counts come as int32 tensors / arrays
    assert histograms.quantile_bounds(one.astype(np.int32), 500) == (float(us[100]), float(us[101]))


def test_merge_is_int64_and_does_not_wrap():
    a = np.full((3, BINS), 0xFFFFFFFF, np.uint32)
    m = histograms.merge(a, a.view(np.int32), a[0])  # an int32 view holds u32 counts
    assert m.dtype == np.int64 and m.shape == (3, BINS)
    assert int(m[0, 0]) == 3 * 0xFFFFFFFF > 2 ** 32
    assert histograms.merge(np.ones(BINS, np.int32)).dtype == np.int64
    with pytest.raises(ValueError):
        histograms.merge(np.ones(BINS - 1, np.int64))
    with pytest.raises(ValueError):
        histograms.merge()
