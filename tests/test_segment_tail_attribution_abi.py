"""CPU: nvrx_segment_tail_attribution_ragged is exported and bound, the ctypes struct has the
layout the C compiler gives ``nvrx_segtailattr_args`` (sizeof and every offset, from a tiny C
probe), the ABI version is unchanged (the entry is additive), and the host-side argument checks
run before any launch (NVRX_ERR_INVALID with a message naming the argument)."""
import ctypes
import os
import re
import subprocess

import pytest

from nvidia_resiliency_ext.straggler import _native, ops

NAME = "nvrx_segment_tail_attribution_ragged"
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
FIELDS = [n for n, _ in _native.SegTailAttrArgs._fields_]
OUTPUTS = ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share", "loss_all")


def _invalid(rc, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error()
    assert re.search(word, msg.decode()), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def _attr(**kw):
    f = dict(R=1, K=1, ns=16, seg_off=16, seg_len=16, max_len=8, cap=0, aligned16=0, top=4, thr=16,
             thr_index=None, base=16, **{n: 16 for n in OUTPUTS})
    f.update(kw)
    a = _native.SegTailAttrArgs(*(f[n] for n in FIELDS))
    return getattr(_native.lib(), NAME)(ctypes.byref(a), None)


def test_symbol_loaded_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    assert hasattr(raw, NAME) and NAME in _native.SIGNATURES
    assert getattr(L, NAME).argtypes == _native.SIGNATURES[NAME][1]
    assert L.nvrx_abi_version() == _native.ABI_VERSION == 6  # additive
    assert callable(ops.segment_tail_attribution_ragged)


def test_struct_layout_matches_the_c_compiler(tmp_path):
    src = tmp_path / "probe.c"
    lines = "".join(f'    printf("{n} %zu\\n", offsetof(nvrx_segtailattr_args, {n}));\n' for n in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nvrx_straggler.h"\n'
                   'int main(void) {\n    printf("sizeof %zu\\n", sizeof(nvrx_segtailattr_args));\n'
                   f'{lines}    return 0;\n}}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)], check=True)
    out = dict(l.split(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == ctypes.sizeof(_native.SegTailAttrArgs)
    assert list(out) == FIELDS
    for n in FIELDS:
        assert int(out[n]) == getattr(_native.SegTailAttrArgs, n).offset, n


def test_header_names_the_entry_beyond_the_reference():
    with open(os.path.join(INC, "nvrx_straggler.h")) as f:
        head = f.read().split("#ifndef NVRX_STRAGGLER_H")[0]
    assert NAME in head.split("Beyond the reference")[1]


def test_bad_arguments():
    _invalid(getattr(_native.lib(), NAME)(None, None), "args")
    for n in ("ns", "seg_off", "thr", "base") + OUTPUTS:
        _invalid(_attr(**{n: None}), "null " + n)
    for n in ("seg_off", "base", "loss", "tail_ns", "total_ns", "base_share", "loss_all"):
        _invalid(_attr(**{n: 20}), n + " not 8-byte aligned")
    for top in (0, -1, 17):
        _invalid(_attr(top=top), "top")
    _invalid(_attr(R=-1), "R")
    _invalid(_attr(K=-1), "K")
    _invalid(_attr(max_len=-1), "max_len")
    _invalid(_attr(K=(1 << 31) // 240 + 1), r"K \* 240")
    _invalid(_attr(R=1 << 20, K=1 << 12), r"R \* K")
    _invalid(_attr(max_len=(1 << 30) + 1), "max_len longer than NVRX_MAX_SEGMENT")
    assert _attr(max_len=(1 << 30) + 1, cap=8, R=0) == _native.NVRX_OK  # the retained run counts


def test_empty_shapes_launch_nothing():
    none = dict(ns=None, seg_off=None, seg_len=None, thr=None, base=None, **{n: None for n in OUTPUTS})
    assert _attr(R=0, **none) == _native.NVRX_OK
    assert _attr(K=0, **none) == _native.NVRX_OK
    _invalid(_attr(R=0, top=0, **none), "top")  # top is checked for every shape


def test_the_wrapper_checks_before_any_launch():
    import torch
    cpu = torch.zeros(4, dtype=torch.int32)
    for top in (0, 17, True, 2.5):
        with pytest.raises(ValueError, match="top"):
            ops.segment_tail_attribution_ragged(None, None, None, 2, 8, None, None, top=top)
    with pytest.raises(ValueError, match="K must"):
        ops.segment_tail_attribution_ragged(cpu, None, None, -1, 8, None, None, top=4)
    with pytest.raises(ValueError, match="device"):
        ops.segment_tail_attribution_ragged(cpu, torch.zeros(4, dtype=torch.int64), cpu, 2, 8,
                                            None, None, top=4)
