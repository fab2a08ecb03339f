"""CPU: the quantile entry points are exported and bound, and their host-side argument
checks run before any launch (no GPU needed): NVRX_ERR_INVALID with a message naming the
argument.  The ops wrappers reject a bad permille list with ValueError."""
import ctypes
import re

import pytest

from nvidia_resiliency_ext.straggler import _native, ops

NAMES = ("nvrx_segment_quantiles_strided", "nvrx_segment_quantiles_ragged",
         "nvrx_profiler_get_quantiles")
BIG = (1 << 30) + 1  # above NVRX_MAX_SEGMENT


def _pm(*v):
    return (ctypes.c_int32 * max(len(v), 1))(*v)


def _strided(ns=16, nseg=1, stride=8, begin=0, length=8, cap=0, pm=_pm(500), nq=1, out=16, num=None):
    return _native.lib().nvrx_segment_quantiles_strided(ns, nseg, stride, begin, length, cap, pm, nq,
                                                        out, num, None)


def _ragged(ns=16, off=16, lens=None, nseg=1, max_len=8, cap=0, aligned16=0, pm=_pm(500), nq=1,
            out=16, num=None):
    return _native.lib().nvrx_segment_quantiles_ragged(ns, off, lens, nseg, max_len, cap, aligned16,
                                                       pm, nq, out, num, None)


def _invalid(rc, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error()
    assert re.search(word, msg.decode()), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def test_symbols_loaded_and_bound():
    assert _native.NVRX_MAX_QUANTILES == 8
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in _native.SIGNATURES
        assert getattr(L, n).argtypes == _native.SIGNATURES[n][1]
    assert L.nvrx_abi_version() == 6  # additive: no struct or signature changed


@pytest.mark.parametrize("call", [_strided, _ragged])
def test_bad_quantile_requests(call):
    _invalid(call(nq=0), "nq")
    _invalid(call(nq=9, pm=_pm(*range(9))), "nq")
    _invalid(call(nq=-1), "nq")
    _invalid(call(pm=None), "permille")
    _invalid(call(pm=_pm(-1)), "permille")
    _invalid(call(pm=_pm(1001)), "permille")
    _invalid(call(pm=_pm(0, 500, 1001), nq=3), r"permille\[2\]")


def test_bad_strided_arguments():
    _invalid(_strided(out=None), "out")
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
    _invalid(_ragged(out=None), "out")
    _invalid(_ragged(ns=None), "ns")
    _invalid(_ragged(off=None), "seg_off")
    _invalid(_ragged(nseg=-1), "nseg")
    _invalid(_ragged(max_len=-1), "max_len")
    _invalid(_ragged(nseg=1 << 31), "nseg")
    _invalid(_ragged(max_len=BIG), "NVRX_MAX_SEGMENT")


def test_zero_segments_launch_nothing():
    # nseg == 0: OK without touching the device (null arrays allowed), after the request checks
    assert _strided(ns=None, nseg=0, out=None) == _native.NVRX_OK
    assert _ragged(ns=None, off=None, nseg=0, out=None) == _native.NVRX_OK
    _invalid(_strided(ns=None, nseg=0, out=None, nq=0), "nq")


def test_profiler_get_quantiles_arguments():
    L = _native.lib()
    cnt = ctypes.c_int64()
    _invalid(L.nvrx_profiler_get_quantiles(None, _pm(500), 1, 0, ctypes.byref(cnt), None, None, None),
             "handle")


@pytest.mark.parametrize("bad", [(), tuple(range(9)), (-1,), (1001,), (500, -1), (0.5,), None, 500])
def test_ops_wrappers_reject_bad_permille(bad):
    # the permille check comes first: no tensor is looked at, so this runs without a GPU
    with pytest.raises(ValueError, match="permille"):
        ops.segment_quantiles_strided(None, 1, 8, 0, 8, bad)
    with pytest.raises(ValueError, match="permille"):
        ops.segment_quantiles_ragged(None, None, None, 8, bad)


def test_permille_array_accepts_the_documented_requests():
    a = ops.permille_array((0, 1, 250, 500, 900, 990, 999, 1000))
    assert list(a) == [0, 1, 250, 500, 900, 990, 999, 1000]
    assert list(ops.permille_array([1000, 1000, 0])) == [1000, 1000, 0]  # repeats, any order
