"""CPU: nvrx_histogram_history_attribution_compact is exported and bound, the ABI is still 6, the
ctypes struct has the layout the C compiler gives ``nvrx_histchistattr_args`` (sizeof and every
offset, from a tiny C probe, as C11 and as C++17) in the stated field order, and its host-side
argument checks run before any launch (NVRX_ERR_INVALID with a message that starts with the
entry's name and names the argument)."""
import ctypes
import os
import re
import subprocess

import pytest

from nvidia_resiliency_ext.straggler import _native, histograms, ops

NAME = "nvrx_histogram_history_attribution_compact"
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
ORDER = ["R", "K", "counts", "top", "chist", "hist_stride", "hist_index", "col_valid", "permille",
         "idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share", "loss_all"]
FIELDS = [n for n, _ in _native.HistCHistAttrArgs._fields_]
OUT8 = ("loss", "tail_ns", "total_ns", "base_share", "loss_all")
OUTS = ("idx",) + OUT8 + ("tail_calls", "thr_bucket")


def _invalid(rc, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error().decode()
    assert msg.startswith(NAME + ": ") and re.search(word, msg), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def _call(**kw):
    f = dict(R=1, K=1, counts=16, top=4, chist=64, hist_stride=0, hist_index=None, col_valid=None,
             permille=990, idx=16, loss=16, tail_ns=16, total_ns=16, tail_calls=16, thr_bucket=16,
             base_share=16, loss_all=16)
    f.update(kw)
    a = _native.HistCHistAttrArgs(*(f[n] for n in FIELDS))
    return getattr(_native.lib(), NAME)(ctypes.byref(a), None)


def test_symbol_loaded_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    assert hasattr(raw, NAME) and NAME in _native.SIGNATURES
    assert getattr(L, NAME).argtypes == _native.SIGNATURES[NAME][1]
    assert L.nvrx_abi_version() == _native.ABI_VERSION == 6  # additive
    assert callable(ops.histogram_history_attribution_compact)
    assert "ops.histogram_history_attribution_compact" in histograms.compact_history_attribution.__doc__
    with open(os.path.join(INC, "nvrx_straggler.h")) as f:
        text = f.read()
    assert NAME in text.split("*/", 1)[0]  # listed in the header's index comment
    assert "#define NVRX_ABI_VERSION 6\n" in text


def test_field_order_and_the_outputs_of_the_dense_entry():
    assert FIELDS == ORDER
    dense = [n for n, _ in _native.TailAttrArgs._fields_]
    assert FIELDS[-8:] == dense[-8:]  # the eight outputs of nvrx_tailattr_args, in its order


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")])
def test_struct_layout_matches_the_c_compiler(tmp_path, compiler, std, ext):
    src = tmp_path / f"probe.{ext}"
    lines = "".join(f'    printf("{n} %zu\\n", offsetof(nvrx_histchistattr_args, {n}));\n' for n in ORDER)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nvrx_straggler.h"\n'
                   'int main(void) {\n    printf("sizeof %zu\\n", sizeof(nvrx_histchistattr_args));\n'
                   '    /* the prototype, unevaluated: nothing to link */\n'
                   '    (void)sizeof(nvrx_histogram_history_attribution_compact('
                   '(const nvrx_histchistattr_args*)0, (void*)0));\n'
                   f'{lines}    return 0;\n}}\n')
    exe = tmp_path / "probe"
    subprocess.run([compiler, std, "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)], check=True)
    out = dict(l.split(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == ctypes.sizeof(_native.HistCHistAttrArgs)
    assert list(out) == ORDER
    offsets = [int(out[n]) for n in ORDER]
    assert offsets == sorted(offsets) and len(set(offsets)) == len(offsets)  # declared in this order
    for n in ORDER:
        assert int(out[n]) == getattr(_native.HistCHistAttrArgs, n).offset, n


def test_bad_arguments():
    _invalid(getattr(_native.lib(), NAME)(None, None), "args")
    for top in (0, 17, -1):
        _invalid(_call(top=top), "top")
    for pm in (-1, 1001):
        _invalid(_call(permille=pm), "permille")
    _invalid(_call(hist_stride=-1), "hist_stride")
    _invalid(_call(K=3, hist_stride=2), "hist_stride below K")  # identity slots would leave the row
    for n in ("counts", "chist") + OUTS:
        _invalid(_call(**{n: None}), "null " + n)
    _invalid(_call(counts=24), "counts not 16-byte")
    _invalid(_call(chist=72), "chist not 16-byte")
    for n in OUT8:
        _invalid(_call(**{n: 20}), n + " not 8-byte")
    _invalid(_call(R=-1), "negative R")
    _invalid(_call(K=-1), "negative K")
    _invalid(_call(R=1, K=(1 << 31) // 240 + 1), r"K \* 240")
    _invalid(_call(R=1 << 20, K=1 << 12), r"R \* K")


def test_hist_stride_with_hist_index_may_be_below_K():
    # R == 0: nothing is launched, the check alone runs
    assert _call(R=0, K=3, hist_stride=2, hist_index=16) == _native.NVRX_OK


def test_empty_shapes_launch_nothing():
    none = {n: None for n in ("counts", "chist") + OUTS}
    assert _call(R=0) == _native.NVRX_OK
    assert _call(R=0, **none) == _native.NVRX_OK
    assert _call(K=0, **none) == _native.NVRX_OK


def test_ops_wrapper_checks_before_any_tensor():
    for bad in (0, 17, True, 1.5):
        with pytest.raises(ValueError, match="top"):
            ops.histogram_history_attribution_compact(None, None, permille=990, top=bad)
    for bad in (-1, 1001, 0.5, True):
        with pytest.raises(ValueError, match="permille"):
            ops.histogram_history_attribution_compact(None, None, permille=bad, top=4)
