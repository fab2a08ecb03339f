"""CPU: nvrx_score_attribution is exported and bound, the ABI version is unchanged, and its
host-side argument checks run before any launch (no GPU needed): NVRX_ERR_INVALID with a message
naming the argument.  The ops wrapper rejects a bad top / kind with ValueError."""
import ctypes
import re

import pytest

from nvidia_resiliency_ext.straggler import _native, ops

NAME = "nvrx_score_attribution"
PTR = 64  # a non-null "pointer": every check below fails (or R == 0 returns) before it is used


def _call(R=1, K=1, value_f64=0, num=PTR, med=PTR, avg=PTR, col_valid=None, ref=PTR, ref_index=None,
          ref_missing=None, hist=PTR, hist_index=None, hist_stride=0, kind=_native.NVRX_ATTR_RELATIVE,
          top=8, idx=PTR, loss=PTR, score=PTR, wsum=None, err=None):
    a = _native.AttributionArgs(R, K, value_f64, num, med, avg, col_valid, ref, ref_index,
                                ref_missing, hist, hist_index, hist_stride, kind, top, idx, loss,
                                score, wsum, err)
    return _native.lib().nvrx_score_attribution(ctypes.byref(a), None)


def _invalid(rc, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error()
    assert re.search(word, msg.decode()), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def test_symbol_loaded_and_bound():
    assert _native.NVRX_MAX_ATTRIBUTION == 16
    assert (_native.NVRX_ATTR_RELATIVE, _native.NVRX_ATTR_INDIVIDUAL) == (0, 1)
    raw = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(raw, NAME)
    assert NAME in _native.SIGNATURES
    assert getattr(_native.lib(), NAME).argtypes == _native.SIGNATURES[NAME][1]
    assert _native.lib().nvrx_abi_version() == _native.ABI_VERSION == 6  # additive change


def test_args_struct_layout():
    # the ctypes mirror of nvrx_attribution_args: 2 i64, i32 (+pad), 10 pointers / i64, 2 i32,
    # 5 pointers
    A = _native.AttributionArgs
    assert ctypes.sizeof(A) == 16 + 8 + 10 * 8 + 8 + 5 * 8
    assert A.kind.offset == 104 and A.top.offset == 108 and A.idx.offset == 112
    assert A.err.offset == 144


@pytest.mark.parametrize("top", [0, 17, -1, 1 << 20])
def test_bad_top(top):
    _invalid(_call(top=top), r"\btop\b")
    _invalid(_call(R=0, top=top), r"\btop\b")  # the request is checked even with nothing to do


@pytest.mark.parametrize("kind", [2, -1, 7])
def test_unknown_kind(kind):
    _invalid(_call(kind=kind), "kind")


@pytest.mark.parametrize("arg", ["num", "med", "avg", "idx", "loss", "score"])
@pytest.mark.parametrize("kind", [_native.NVRX_ATTR_RELATIVE, _native.NVRX_ATTR_INDIVIDUAL])
def test_null_arrays(arg, kind):
    _invalid(_call(kind=kind, **{arg: None}), rf"\b{arg}\b")


def test_kind_needs_its_base():
    _invalid(_call(kind=_native.NVRX_ATTR_RELATIVE, ref=None), r"\bref\b")
    _invalid(_call(kind=_native.NVRX_ATTR_INDIVIDUAL, hist=None), r"\bhist\b")


def test_negative_sizes():
    _invalid(_call(R=-1), r"\bR\b")
    _invalid(_call(K=-1), r"\bK\b")
    _invalid(_call(K=1 << 31), r"\bK\b")
    _invalid(_native.lib().nvrx_score_attribution(None, None), "args")


def test_nothing_to_do_launches_nothing():
    # R == 0 or K == 0: NVRX_OK without touching the device (this runs without one); wsum and
    # err may be NULL, and the arrays may be too when there is nothing to read or write
    assert _call(R=0) == _native.NVRX_OK
    assert _call(K=0) == _native.NVRX_OK
    assert _call(R=0, num=None, med=None, avg=None, idx=None, loss=None, score=None,
                 ref=None) == _native.NVRX_OK
    assert _call(R=0, kind=_native.NVRX_ATTR_INDIVIDUAL, hist=None) == _native.NVRX_OK


@pytest.mark.parametrize("top", [0, 17, -3, 2.0, None, True, "8"])
def test_ops_wrapper_rejects_bad_top(top):
    # the request check comes first: no tensor is looked at, so this runs without a GPU
    with pytest.raises(ValueError, match="top"):
        ops.score_attribution(None, None, None, top=top, kind="relative")


@pytest.mark.parametrize("kind", ["absolute", "", None, 0, "RELATIVE"])
def test_ops_wrapper_rejects_unknown_kind(kind):
    with pytest.raises(ValueError, match="kind"):
        ops.score_attribution(None, None, None, top=8, kind=kind)


def test_detector_not_initialized():
    # as the other Detector classmethods (kernel_quantiles, generate_report): an assertion
    from nvidia_resiliency_ext.straggler import Detector

    assert not Detector.initialized
    with pytest.raises(AssertionError):
        Detector.kernel_attribution()


def test_attribution_request_accepts_the_documented_range():
    assert ops.attribution_request(1, "relative") == (1, _native.NVRX_ATTR_RELATIVE)
    assert ops.attribution_request(16, "individual") == (16, _native.NVRX_ATTR_INDIVIDUAL)
