"""CPU: nvrx_segment_fleet_histogram_ragged / nvrx_segment_tail_scores_ragged are exported and
bound, the ctypes struct has the layout the C compiler gives ``nvrx_segtail_args`` (sizeof and
every offset, from a tiny C probe), the ABI version is unchanged (the entries are additive), and
the host-side argument checks run before any launch (NVRX_ERR_INVALID with a message naming the
argument)."""
import ctypes
import os
import re
import subprocess

import pytest

from nvidia_resiliency_ext.straggler import _native, ops

NAMES = ("nvrx_segment_fleet_histogram_ragged", "nvrx_segment_tail_scores_ragged")
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
FIELDS = [n for n, _ in _native.SegTailArgs._fields_]


def _invalid(rc, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error()
    assert re.search(word, msg.decode()), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def _tail(**kw):
    f = dict(R=1, K=1, ns=16, seg_off=16, seg_len=16, max_len=8, cap=0, aligned16=0, thr=16,
             thr_index=None, fleet_sums=16, tail_ns=16, total_ns=16, score=16, tail_calls=None,
             strag=None, score_thr=0.75)
    f.update(kw)
    a = _native.SegTailArgs(*(f[n] for n in FIELDS))
    return _native.lib().nvrx_segment_tail_scores_ragged(ctypes.byref(a), None)


def _fleet(**kw):
    f = dict(ns=16, seg_off=16, seg_len=16, R=1, K=1, max_len=8, cap=0, aligned16=0, accumulate=0,
             fleet=16)
    f.update(kw)
    return _native.lib().nvrx_segment_fleet_histogram_ragged(*f.values(), None)


def test_symbols_loaded_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    for name in NAMES:
        assert hasattr(raw, name) and name in _native.SIGNATURES
        assert getattr(L, name).argtypes == _native.SIGNATURES[name][1]
    assert L.nvrx_abi_version() == _native.ABI_VERSION == 6  # additive
    assert callable(ops.segment_fleet_histogram_ragged) and callable(ops.segment_tail_scores_ragged)


def test_struct_layout_matches_the_c_compiler(tmp_path):
    src = tmp_path / "probe.c"
    lines = "".join(f'    printf("{n} %zu\\n", offsetof(nvrx_segtail_args, {n}));\n' for n in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nvrx_straggler.h"\n'
                   'int main(void) {\n    printf("sizeof %zu\\n", sizeof(nvrx_segtail_args));\n'
                   f'{lines}    return 0;\n}}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)], check=True)
    out = dict(l.split(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == ctypes.sizeof(_native.SegTailArgs)
    assert list(out) == FIELDS
    for n in FIELDS:
        assert int(out[n]) == getattr(_native.SegTailArgs, n).offset, n


def test_header_names_the_entries_beyond_the_reference():
    with open(os.path.join(INC, "nvrx_straggler.h")) as f:
        head = f.read().split("#ifndef NVRX_STRAGGLER_H")[0]
    beyond = head.split("Beyond the reference")[1]
    for name in NAMES:
        assert name in beyond


def test_bad_arguments_tail():
    _invalid(_native.lib().nvrx_segment_tail_scores_ragged(None, None), "args")
    for n in ("ns", "seg_off", "thr", "fleet_sums", "tail_ns", "total_ns", "score"):
        _invalid(_tail(**{n: None}), n)
    for n in ("seg_off", "fleet_sums", "tail_ns", "total_ns", "score"):
        _invalid(_tail(**{n: 20}), n + " not 8-byte aligned")
    _invalid(_tail(R=-1), "R")
    _invalid(_tail(K=-1), "K")
    _invalid(_tail(max_len=-1), "max_len")
    _invalid(_tail(K=(1 << 31) // 240 + 1), r"K \* 240")
    _invalid(_tail(R=1 << 20, K=1 << 12), r"R \* K")
    _invalid(_tail(max_len=(1 << 30) + 1), "max_len longer than NVRX_MAX_SEGMENT")
    assert _tail(max_len=(1 << 30) + 1, cap=8, R=0) == _native.NVRX_OK  # the retained run counts


def test_bad_arguments_fleet():
    for n in ("ns", "seg_off", "fleet"):
        _invalid(_fleet(**{n: None}), n)
    _invalid(_fleet(seg_off=20), "seg_off not 8-byte aligned")
    _invalid(_fleet(fleet=24), "fleet not 16-byte aligned")
    _invalid(_fleet(R=-1), "R")
    _invalid(_fleet(K=-1), "K")
    _invalid(_fleet(max_len=-1), "max_len")
    _invalid(_fleet(K=(1 << 31) // 240 + 1), r"K \* 240")
    _invalid(_fleet(R=1 << 20, K=1 << 12), r"R \* K")
    _invalid(_fleet(max_len=(1 << 30) + 1), "max_len longer than NVRX_MAX_SEGMENT")


def test_empty_shapes_launch_nothing():
    none = dict(ns=None, seg_off=None, seg_len=None)
    assert _fleet(R=0, fleet=None, **none) == _native.NVRX_OK
    assert _fleet(K=0, fleet=None, **none) == _native.NVRX_OK
    out = dict(thr=None, fleet_sums=None, tail_ns=None, total_ns=None, score=None)
    assert _tail(R=0, **none, **out) == _native.NVRX_OK
    assert _tail(K=0, **none, **out) == _native.NVRX_OK


def test_wrappers_check_before_any_launch():
    with pytest.raises(ValueError, match="accumulate"):
        ops.segment_fleet_histogram_ragged(None, None, None, 4, 8, accumulate=True)
    import torch
    cpu = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="device"):
        ops.segment_fleet_histogram_ragged(cpu, torch.zeros(4, dtype=torch.int64), cpu, 2, 8)
    with pytest.raises(ValueError, match="K must"):
        ops.segment_tail_scores_ragged(cpu, None, None, -1, 8, None, None)
