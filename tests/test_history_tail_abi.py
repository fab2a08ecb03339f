"""CPU: nvrx_histogram_history_scores is exported and bound, the ctypes struct has the layout the
C compiler gives ``nvrx_histtail_args`` (sizeof and every offset, from a tiny C probe), and its
host-side argument checks run before any launch (NVRX_ERR_INVALID with a message)."""
import ctypes
import os
import re
import subprocess

import pytest

from nvidia_resiliency_ext.straggler import _native, ops

NAME = "nvrx_histogram_history_scores"
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
FIELDS = [n for n, _ in _native.HistTailArgs._fields_]


def _invalid(rc, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error()
    assert re.search(word, msg.decode()), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def _call(**kw):
    f = dict(R=1, K=1, counts=16, hist=32, hist_stride=0, hist_index=None, col_valid=None,
             skip_rows=None, permille=990, mode=3, score_thr=0.75, tail_ns=16, total_ns=16,
             base_tail_ns=16, base_total_ns=16, score=16, strag=None, tail_calls=None)
    f.update(kw)
    a = _native.HistTailArgs(*(f[n] for n in FIELDS))
    return _native.lib().nvrx_histogram_history_scores(ctypes.byref(a), None)


def test_symbol_loaded_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    assert hasattr(raw, NAME) and NAME in _native.SIGNATURES
    assert getattr(L, NAME).argtypes == _native.SIGNATURES[NAME][1]
    assert L.nvrx_abi_version() == _native.ABI_VERSION == 6  # additive
    assert (_native.NVRX_HTAIL_SCORE, _native.NVRX_HTAIL_UPDATE) == (1, 2)
    assert callable(ops.histogram_history_scores)


def test_struct_layout_matches_the_c_compiler(tmp_path):
    src = tmp_path / "probe.c"
    lines = "".join(f'    printf("{n} %zu\\n", offsetof(nvrx_histtail_args, {n}));\n' for n in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nvrx_straggler.h"\n'
                   'int main(void) {\n    printf("sizeof %zu\\n", sizeof(nvrx_histtail_args));\n'
                   f'    printf("flags %d %d\\n", NVRX_HTAIL_SCORE, NVRX_HTAIL_UPDATE);\n{lines}'
                   '    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)], check=True)
    out = dict(l.split(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == ctypes.sizeof(_native.HistTailArgs)
    assert out.pop("flags") == f"{_native.NVRX_HTAIL_SCORE} {_native.NVRX_HTAIL_UPDATE}"
    assert list(out) == FIELDS
    for n in FIELDS:
        assert int(out[n]) == getattr(_native.HistTailArgs, n).offset, n


def test_bad_arguments():
    _invalid(_native.lib().nvrx_histogram_history_scores(None, None), "args")
    for mode in (0, 4, 7, -1):
        _invalid(_call(mode=mode), "mode")
    for pm in (-1, 1001):
        _invalid(_call(permille=pm), "permille")
    _invalid(_call(hist_stride=-1), "hist_stride")
    _invalid(_call(K=3, hist_stride=2), "hist_stride")  # identity slots would leave the row
    for n in ("counts", "hist", "tail_ns", "total_ns", "base_tail_ns", "base_total_ns", "score"):
        _invalid(_call(**{n: None}), n)
    _invalid(_call(counts=20), "counts")  # not 16-byte aligned
    _invalid(_call(hist=24), "hist")
    _invalid(_call(total_ns=20), "8-byte")
    _invalid(_call(R=-1), "R")
    _invalid(_call(K=-1), "K")
    _invalid(_call(K=(1 << 31) // 240 + 1), r"K \* 240")
    _invalid(_call(R=1 << 20, K=1 << 12), r"R \* K")
    # update alone needs no score output
    _invalid(_call(mode=2, tail_ns=None, total_ns=None, base_tail_ns=None, base_total_ns=None,
                   score=None, hist=None), "hist")


def test_empty_shapes_launch_nothing():
    for mode in (1, 2, 3):
        assert _call(R=0, counts=None, hist=None, score=None, mode=mode) == _native.NVRX_OK
        assert _call(K=0, counts=None, hist=None, tail_ns=None, mode=mode) == _native.NVRX_OK


def test_ops_wrapper_checks_before_any_tensor():
    for bad in (-1, 1001, 0.5, True):
        with pytest.raises(ValueError, match="permille"):
            ops.histogram_history_scores(None, None, permille=bad)
    with pytest.raises(ValueError, match="at least one"):
        ops.histogram_history_scores(None, None, permille=990, score=False, update=False)
