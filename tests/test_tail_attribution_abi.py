"""CPU: nvrx_histogram_tail_base / nvrx_histogram_tail_attribution are exported and bound, the
ctypes struct has the layout the C compiler gives ``nvrx_tailattr_args`` (sizeof and every offset,
from a tiny C probe), and the host-side argument checks run before any launch (NVRX_ERR_INVALID
with a message)."""
import ctypes
import os
import re
import subprocess

import pytest

from nvidia_resiliency_ext.straggler import _native, batch, ops, straggler

NAMES = ("nvrx_histogram_tail_base", "nvrx_histogram_tail_attribution")
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
FIELDS = [n for n, _ in _native.TailAttrArgs._fields_]


def _invalid(rc, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error()
    assert re.search(word, msg.decode()), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def _call(**kw):
    f = dict(R=1, K=1, counts=16, kind=0, top=4, thr=16, thr_index=None, base=16, hist=None,
             hist_stride=0, hist_index=None, col_valid=None, permille=950, idx=16, loss=16,
             tail_ns=16, total_ns=16, tail_calls=16, thr_bucket=16, base_share=16, loss_all=16)
    f.update(kw)
    a = _native.TailAttrArgs(*(f[n] for n in FIELDS))
    return _native.lib().nvrx_histogram_tail_attribution(ctypes.byref(a), None)


def _ind(**kw):
    return _call(**dict(dict(kind=1, thr=None, base=None, hist=32), **kw))


def test_symbols_loaded_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    for name in NAMES:
        assert hasattr(raw, name) and name in _native.SIGNATURES
        assert getattr(L, name).argtypes == _native.SIGNATURES[name][1]
    assert L.nvrx_abi_version() == _native.ABI_VERSION == 6  # additive
    assert callable(ops.histogram_tail_base) and callable(ops.histogram_tail_attribution)


def test_struct_layout_matches_the_c_compiler(tmp_path):
    src = tmp_path / "probe.c"
    lines = "".join(f'    printf("{n} %zu\\n", offsetof(nvrx_tailattr_args, {n}));\n' for n in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nvrx_straggler.h"\n'
                   'int main(void) {\n    printf("sizeof %zu\\n", sizeof(nvrx_tailattr_args));\n'
                   '    printf("consts %d %d %d\\n", NVRX_ATTR_RELATIVE, NVRX_ATTR_INDIVIDUAL, '
                   f'NVRX_MAX_ATTRIBUTION);\n{lines}    return 0;\n}}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)], check=True)
    out = dict(l.split(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == ctypes.sizeof(_native.TailAttrArgs)
    assert out.pop("consts") == (f"{_native.NVRX_ATTR_RELATIVE} {_native.NVRX_ATTR_INDIVIDUAL} "
                                 f"{_native.NVRX_MAX_ATTRIBUTION}")
    assert list(out) == FIELDS
    for n in FIELDS:
        assert int(out[n]) == getattr(_native.TailAttrArgs, n).offset, n


def test_bad_arguments_attribution():
    _invalid(_native.lib().nvrx_histogram_tail_attribution(None, None), "args")
    for top in (0, 17, -1):
        _invalid(_call(top=top), "top")
        _invalid(_call(top=top, R=0), "top")  # checked even where nothing would be launched
    for kind in (2, -1):
        _invalid(_call(kind=kind), "kind")
    for n in ("counts", "thr", "base", "idx", "loss", "tail_ns", "total_ns", "tail_calls",
              "thr_bucket", "base_share", "loss_all"):
        _invalid(_call(**{n: None}), n)
    for n in ("counts", "hist", "idx", "loss_all"):
        _invalid(_ind(**{n: None}), n)
    for pm in (-1, 1001):
        _invalid(_ind(permille=pm), "permille")
    _invalid(_ind(hist_stride=-1), "hist_stride")
    _invalid(_ind(K=3, hist_stride=2), "hist_stride")
    _invalid(_call(counts=20), "counts")  # not 16-byte aligned
    _invalid(_ind(hist=24), "hist")
    _invalid(_call(base=20), "base")
    for n in ("loss", "tail_ns", "total_ns", "base_share", "loss_all"):
        _invalid(_call(**{n: 20}), "8-byte")
    _invalid(_call(R=-1), "R")
    _invalid(_call(K=-1), "K")
    _invalid(_call(K=(1 << 31) // 240 + 1), r"K \* 240")
    _invalid(_call(R=1 << 20, K=1 << 12), r"R \* K")


def test_bad_arguments_base():
    base = _native.lib().nvrx_histogram_tail_base
    _invalid(base(None, 1, 16, 16, None), "fleet")
    _invalid(base(16, 1, None, 16, None), "thr")
    _invalid(base(16, 1, 16, None, None), "base")
    _invalid(base(24, 1, 16, 16, None), "fleet")
    _invalid(base(16, 1, 16, 24, None), "base")
    _invalid(base(16, -1, 16, 16, None), "K")
    _invalid(base(16, (1 << 31) // 240 + 1, 16, 16, None), r"K \* 240")


def test_empty_shapes_launch_nothing():
    assert _native.lib().nvrx_histogram_tail_base(None, 0, None, None, None) == _native.NVRX_OK
    for call in (_call, _ind):
        assert call(R=0, counts=None, idx=None, loss_all=None) == _native.NVRX_OK
        assert call(K=0, counts=None, thr=None, base=None, hist=None, loss=None) == _native.NVRX_OK


def test_wrappers_check_before_any_tensor():
    for top in (0, 17, True, 2.5):
        with pytest.raises(ValueError, match="top"):
            ops.histogram_tail_attribution(None, top=top, kind="relative")
    with pytest.raises(ValueError, match="kind"):
        ops.histogram_tail_attribution(None, top=4, kind="both")


def test_result_types_carry_the_attribution_last():
    import dataclasses
    for cls in (straggler.TailScore, straggler.IndividualTailScore, batch.BatchTailScores,
                batch.BatchIndividualTailScores):
        f = dataclasses.fields(cls)[-1]
        assert f.name == "attribution" and f.default is None
    assert [f.name for f in dataclasses.fields(straggler.KernelTailAttribution)] == [
        "name", "loss_ns", "tail_ns", "total_ns", "tail_calls", "threshold_us", "base_share"]
    assert ops.TailAttribution.PACKED == 4 * 8 + 3 * 4
