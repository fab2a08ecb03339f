"""CPU: nvrx_segment_history_scores_compact_ragged is exported and bound, the ABI is still 6, the
ctypes struct has the layout the C compiler gives ``nvrx_segchist_args`` (sizeof and every offset,
from a tiny C probe, as C11 and as C++17), and its host-side argument checks run before any launch
(NVRX_ERR_INVALID with a message that names the argument)."""
import ctypes
import os
import re
import subprocess

import pytest

from nvidia_resiliency_ext.straggler import _native, histograms, ops

NAME = "nvrx_segment_history_scores_compact_ragged"
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
FIELDS = [n for n, _ in _native.SegCHistArgs._fields_]
SCORE_OUT = ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns", "score")


def _invalid(rc, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error().decode()
    assert msg.startswith(NAME + ": ") and re.search(word, msg), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def _call(**kw):
    # distinct fake addresses: nothing is launched before a check fails, or with R or K of 0
    f = dict(R=1, K=1, ns=16, seg_off=32, seg_len=48, max_len=8, cap=0, aligned16=0, chist=64,
             hist_stride=0, hist_index=None, col_valid=None, skip_rows=None, permille=990, mode=3,
             score_thr=0.75, tail_ns=128, total_ns=136, base_tail_ns=144, base_total_ns=152,
             score=160, strag=None, tail_calls=None, folded=168)
    f.update(kw)
    a = _native.SegCHistArgs(*(f[n] for n in FIELDS))
    return _native.lib().nvrx_segment_history_scores_compact_ragged(ctypes.byref(a), None)


def test_symbol_loaded_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    assert hasattr(raw, NAME) and NAME in _native.SIGNATURES
    assert getattr(L, NAME).argtypes == _native.SIGNATURES[NAME][1]
    assert L.nvrx_abi_version() == _native.ABI_VERSION == 6  # additive
    assert callable(ops.segment_history_scores_compact_ragged)
    for n in ("compact_to_dense", "compact_from_dense", "compact_is_canonical",
              "compact_history_scores", "segment_compact_history_scores"):
        assert callable(getattr(histograms, n))
    assert _native.CHIST_ENTRIES == histograms.CHIST_ENTRIES == 12
    assert _native.CHIST_BYTES == histograms.CHIST_BYTES == 64
    with open(os.path.join(INC, "nvrx_straggler.h")) as f:
        text = f.read()
    assert NAME in text.split("*/", 1)[0]  # listed in the header's index comment
    assert re.search(r"#define NVRX_CHIST_ENTRIES 12\b", text) and re.search(r"#define NVRX_CHIST_BYTES 64\b", text)


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")])
def test_struct_layout_matches_the_c_compiler(tmp_path, compiler, std, ext):
    src = tmp_path / f"probe.{ext}"
    lines = "".join(f'    printf("{n} %zu\\n", offsetof(nvrx_segchist_args, {n}));\n' for n in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nvrx_straggler.h"\n'
                   'int main(void) {\n    printf("sizeof %zu\\n", sizeof(nvrx_segchist_args));\n'
                   '    /* the prototype, unevaluated: nothing to link */\n'
                   '    (void)sizeof(nvrx_segment_history_scores_compact_ragged('
                   '(const nvrx_segchist_args*)0, (void*)0));\n'
                   f'{lines}    return 0;\n}}\n')
    exe = tmp_path / "probe"
    subprocess.run([compiler, std, "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)], check=True)
    out = dict(l.split(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == ctypes.sizeof(_native.SegCHistArgs)
    assert list(out) == FIELDS
    for n in FIELDS:
        assert int(out[n]) == getattr(_native.SegCHistArgs, n).offset, n


def test_bad_arguments():
    _invalid(_native.lib().nvrx_segment_history_scores_compact_ragged(None, None), "args")
    for mode in (0, 4, 7, -1):
        _invalid(_call(mode=mode), "mode")
    for pm in (-1, 1001):
        _invalid(_call(permille=pm), "permille")
    _invalid(_call(hist_stride=-1), "hist_stride")
    _invalid(_call(K=3, hist_stride=2), "hist_stride")  # identity slots would leave the row
    for n in ("ns", "seg_off", "chist", "folded") + SCORE_OUT:
        _invalid(_call(**{n: None}), "null " + n)
    _invalid(_call(chist=72), "chist not 16-byte")
    _invalid(_call(seg_off=36), "seg_off not 8-byte")
    for n in SCORE_OUT + ("folded",):
        _invalid(_call(**{n: 1028}), n + " not 8-byte")
    for addr in (128, 136, 144, 152, 160):  # folded is an accumulator of the pass, like the four sums
        _invalid(_call(folded=addr), "folded aliases")
    _invalid(_call(R=-1), "negative R")
    _invalid(_call(K=-1), "negative K")
    _invalid(_call(max_len=-1), "max_len")
    _invalid(_call(max_len=(1 << 30) + 1), "NVRX_MAX_SEGMENT")
    _invalid(_call(K=(1 << 31) // 240 + 1), r"K \* 240")
    _invalid(_call(R=1 << 20, K=1 << 12), r"R \* K")
    # update alone needs no score output, but the history and folded
    none = {n: None for n in SCORE_OUT}
    _invalid(_call(mode=2, chist=None, **none), "null chist")
    _invalid(_call(mode=2, folded=None, **none), "null folded")
    # an empty ns is fine only when no segment can hold a sample
    _invalid(_call(ns=None, max_len=1), "null ns")


def test_cap_bounds_the_retained_run():
    # max_len above NVRX_MAX_SEGMENT is accepted when cap trims it; R == 0 so nothing is launched
    assert _call(R=0, max_len=(1 << 30) + 1, cap=100) == _native.NVRX_OK


def test_score_alone_needs_no_folded_and_empty_shapes_launch_nothing():
    for mode in (1, 2, 3):
        assert _call(R=0, ns=None, seg_off=None, chist=None, score=None, folded=None, mode=mode) == _native.NVRX_OK
        assert _call(K=0, ns=None, seg_off=None, chist=None, tail_ns=None, folded=None, mode=mode) == _native.NVRX_OK
    assert _call(R=0, mode=1, folded=None) == _native.NVRX_OK


def test_ops_wrapper_checks_before_any_tensor():
    for bad in (-1, 1001, 0.5, True):
        with pytest.raises(ValueError, match="permille"):
            ops.segment_history_scores_compact_ragged(None, None, None, 1, 1, None, permille=bad)
    with pytest.raises(ValueError, match="at least one"):
        ops.segment_history_scores_compact_ragged(None, None, None, 1, 1, None, permille=990,
                                                  score=False, update=False)
