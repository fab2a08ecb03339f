"""CPU: the segment geometry checks of the six nvrx_segment_* entries (one shared checker per
addressing).  One fault table over all of them: every fault is NVRX_ERR_INVALID before any
launch, with a message that starts with the called entry's name and names the offending argument.
The valid calls here all have nseg == 0, which launches nothing: no pointer is ever followed."""
import ctypes
import re

import pytest

from nvidia_resiliency_ext.straggler import _native

BIG = (1 << 30) + 1  # above NVRX_MAX_SEGMENT
P = 16               # a non-null, 16-byte aligned address that no accepted call here reads

STRIDED = ("nvrx_segment_stats_strided", "nvrx_segment_quantiles_strided",
           "nvrx_segment_histogram_strided")
RAGGED = ("nvrx_segment_stats_ragged", "nvrx_segment_quantiles_ragged",
          "nvrx_segment_histogram_ragged")
# each entry's own limit: nseg must be below it
NSEG_LIMIT = {n: 1 << 31 for n in STRIDED + RAGGED}
NSEG_LIMIT["nvrx_segment_stats_strided"] = 1 << 33

_PM = (ctypes.c_int32 * 3)(0, 500, 1000)
_SOA = _native.StatsSoA(P, P, P, P, P, P)


def _strided(entry, ns=P, nseg=1, stride=8, begin=0, length=8, cap=0):
    f = getattr(_native.lib(), entry)
    if "stats" in entry:
        return f(ns, nseg, stride, begin, length, cap, _native.NVRX_STATS_FAST,
                 ctypes.byref(_SOA), None, 0, None)
    if "quantiles" in entry:
        return f(ns, nseg, stride, begin, length, cap, _PM, 3, P, None, None)
    return f(ns, nseg, stride, begin, length, cap, 0, P, None, None)


def _ragged(entry, ns=P, off=P, nseg=1, max_len=8, cap=0):
    f = getattr(_native.lib(), entry)
    if "stats" in entry:
        return f(ns, off, None, nseg, max_len, cap, _native.NVRX_STATS_FAST, 0,
                 ctypes.byref(_SOA), None, 0, None)
    if "quantiles" in entry:
        return f(ns, off, None, nseg, max_len, cap, 0, _PM, 3, P, None, None)
    return f(ns, off, None, nseg, max_len, cap, 0, 0, P, None, None)


# (geometry, the argument the message names); "LIMIT" stands for the entry's own nseg limit
STRIDED_FAULTS = [
    (dict(ns=None), "ns"),
    (dict(nseg=-1), "nseg"),
    (dict(length=-1), "seg_len"),
    (dict(begin=-1), "seg_begin"),
    (dict(stride=-1), "seg_stride"),
    (dict(nseg="LIMIT"), "nseg"),
    (dict(nseg=2, stride=4, length=8), "seg_stride"),   # overlapping segments
    (dict(length=BIG, stride=BIG), "seg_len"),          # retained length above NVRX_MAX_SEGMENT
    (dict(nseg=0, length=BIG, stride=BIG), "seg_len"),  # checked even when nothing would run
]
RAGGED_FAULTS = [
    (dict(ns=None), "ns"),
    (dict(off=None), "seg_off"),
    (dict(nseg=-1), "nseg"),
    (dict(max_len=-1), "max_len"),
    (dict(nseg="LIMIT"), "nseg"),
    (dict(max_len=BIG), "max_len"),
    (dict(nseg=0, max_len=BIG), "max_len"),
]
FAULTS = ([(_strided, e, g, a) for e in STRIDED for g, a in STRIDED_FAULTS] +
          [(_ragged, e, g, a) for e in RAGGED for g, a in RAGGED_FAULTS])


def _id(case):
    _, entry, geom, _ = case
    return entry[len("nvrx_segment_"):] + "-" + ",".join(f"{k}={v}" for k, v in geom.items())


@pytest.mark.parametrize("case", FAULTS, ids=_id)
def test_geometry_fault(case):
    call, entry, geom, arg = case
    geom = {k: NSEG_LIMIT[entry] if v == "LIMIT" else v for k, v in geom.items()}
    assert call(entry, **geom) == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error().decode()
    assert msg.startswith(entry + ": "), msg
    assert re.search(rf"\b{arg}\b", msg[len(entry) + 2:]), (arg, msg)
    if BIG in geom.values():
        assert "NVRX_MAX_SEGMENT" in msg, msg


@pytest.mark.parametrize("entry", STRIDED)
def test_valid_degenerate_strided(entry):
    # nothing to do: null arrays allowed, no launch
    assert _strided(entry, ns=None, nseg=0) == _native.NVRX_OK
    assert _strided(entry, ns=None, nseg=0, length=0, stride=0) == _native.NVRX_OK
    # a cap brings the retained length back in range: the check is on what is retained
    assert _strided(entry, nseg=0, length=BIG, stride=BIG, cap=8192) == _native.NVRX_OK
    # overlap is a fault of two or more segments only
    assert _strided(entry, nseg=0, stride=4, length=8) == _native.NVRX_OK


@pytest.mark.parametrize("entry", RAGGED)
def test_valid_degenerate_ragged(entry):
    assert _ragged(entry, ns=None, off=None, nseg=0) == _native.NVRX_OK
    assert _ragged(entry, ns=None, off=None, nseg=0, max_len=0) == _native.NVRX_OK
    assert _ragged(entry, nseg=0, max_len=BIG, cap=8192) == _native.NVRX_OK


def test_geometry_is_reported_before_family_faults():
    # with several faults the geometry is reported first (quantiles: after permille)
    L = _native.lib()
    assert L.nvrx_segment_histogram_strided(P, -1, 8, 0, 8, 0, 0, None, None, None) == \
        _native.NVRX_ERR_INVALID
    assert re.search(r"\bnseg\b", L.nvrx_last_error().decode())
    assert L.nvrx_segment_stats_ragged(P, P, None, -1, 8, 0, 7, 0, None, None, 0, None) == \
        _native.NVRX_ERR_INVALID
    assert re.search(r"\bnseg\b", L.nvrx_last_error().decode())
    assert L.nvrx_segment_quantiles_ragged(P, P, None, -1, 8, 0, 0, _PM, 0, P, None, None) == \
        _native.NVRX_ERR_INVALID
    assert re.search(r"\bnq\b", L.nvrx_last_error().decode())
