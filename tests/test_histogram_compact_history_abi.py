"""CPU: nvrx_histogram_history_scores_compact, nvrx_compact_history_from_dense and
nvrx_compact_history_to_dense are exported and bound, the ABI is still 6, the ctypes struct has the
layout the C compiler gives ``nvrx_histchist_args`` (sizeof and every offset, from a tiny C probe,
as C11 and as C++17), and the host-side argument checks run before any launch (NVRX_ERR_INVALID
with a message that starts with the entry's name and names the argument)."""
import ctypes
import os
import re
import subprocess

import pytest

from nvidia_resiliency_ext.straggler import _native, batch, histograms, ops

NAME = "nvrx_histogram_history_scores_compact"
FROM, TO = "nvrx_compact_history_from_dense", "nvrx_compact_history_to_dense"
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
FIELDS = [n for n, _ in _native.HistCHistArgs._fields_]
SCORE_OUT = ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns", "score")


def _invalid(rc, word, name=NAME):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error().decode()
    assert msg.startswith(name + ": ") and re.search(word, msg), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def _call(**kw):
    # distinct fake addresses: nothing is launched before a check fails, or with R or K of 0
    f = dict(R=1, K=1, counts=1024, chist=64, hist_stride=0, hist_index=None, col_valid=None,
             skip_rows=None, permille=990, mode=3, score_thr=0.75, tail_ns=128, total_ns=136,
             base_tail_ns=144, base_total_ns=152, score=160, strag=None, tail_calls=None, folded=168)
    f.update(kw)
    a = _native.HistCHistArgs(*(f[n] for n in FIELDS))
    return _native.lib().nvrx_histogram_history_scores_compact(ctypes.byref(a), None)


def _from(hist=1024, chist=64, R=1, stride=1, folded=128):
    return _native.lib().nvrx_compact_history_from_dense(hist, chist, R, stride, folded, None)


def _to(chist=64, hist=1024, R=1, stride=1):
    return _native.lib().nvrx_compact_history_to_dense(chist, hist, R, stride, None)


def test_symbols_loaded_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    with open(os.path.join(INC, "nvrx_straggler.h")) as f:
        text = f.read()
    for n in (NAME, FROM, TO):
        assert hasattr(raw, n) and n in _native.SIGNATURES
        assert getattr(L, n).argtypes == _native.SIGNATURES[n][1]
        assert n in text.split("*/", 1)[0]  # listed in the header's index comment
    assert L.nvrx_abi_version() == _native.ABI_VERSION == 6  # additive
    assert FIELDS == [n for n, _ in _native.HistTailArgs._fields_[:3]] + ["chist"] + \
        [n for n, _ in _native.HistTailArgs._fields_[4:]] + ["folded"]
    for n in ("histogram_history_scores_compact", "compact_history_from_dense",
              "compact_history_to_dense"):
        assert callable(getattr(ops, n))
    assert callable(batch.MatrixReporter.convert_tail_history)
    for n in ("compact_history_scores", "compact_from_dense", "compact_to_dense"):
        assert callable(getattr(histograms, n))


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")])
def test_struct_layout_matches_the_c_compiler(tmp_path, compiler, std, ext):
    src = tmp_path / f"probe.{ext}"
    lines = "".join(f'    printf("{n} %zu\\n", offsetof(nvrx_histchist_args, {n}));\n' for n in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nvrx_straggler.h"\n'
                   'int main(void) {\n    printf("sizeof %zu\\n", sizeof(nvrx_histchist_args));\n'
                   '    /* the prototypes, unevaluated: nothing to link */\n'
                   '    (void)sizeof(nvrx_histogram_history_scores_compact('
                   '(const nvrx_histchist_args*)0, (void*)0));\n'
                   '    (void)sizeof(nvrx_compact_history_from_dense((const uint32_t*)0, (void*)0, '
                   '(int64_t)0, (int64_t)0, (uint64_t*)0, (void*)0));\n'
                   '    (void)sizeof(nvrx_compact_history_to_dense((const void*)0, (uint32_t*)0, '
                   '(int64_t)0, (int64_t)0, (void*)0));\n'
                   f'{lines}    return 0;\n}}\n')
    exe = tmp_path / "probe"
    subprocess.run([compiler, std, "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)], check=True)
    out = dict(l.split(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == ctypes.sizeof(_native.HistCHistArgs)
    assert list(out) == FIELDS
    for n in FIELDS:
        assert int(out[n]) == getattr(_native.HistCHistArgs, n).offset, n


def test_bad_arguments_of_the_score_entry():
    _invalid(_native.lib().nvrx_histogram_history_scores_compact(None, None), "args")
    for mode in (0, 4, 7, -1):
        _invalid(_call(mode=mode), "mode")
    for pm in (-1, 1001):
        _invalid(_call(permille=pm), "permille")
    _invalid(_call(hist_stride=-1), "hist_stride")
    _invalid(_call(K=3, hist_stride=2), "hist_stride")  # identity slots would leave the row
    for n in ("counts", "chist", "folded") + SCORE_OUT:
        _invalid(_call(**{n: None}), "null " + n)
    _invalid(_call(chist=72), "chist not 16-byte")
    _invalid(_call(counts=1032), "counts not 16-byte")
    for n in SCORE_OUT + ("folded",):
        _invalid(_call(**{n: 2052}), n + " not 8-byte")
    for addr in (128, 136, 144, 152, 160):  # folded is an accumulator of the pass, like the four sums
        _invalid(_call(folded=addr), "folded aliases")
    _invalid(_call(R=-1), "negative R")
    _invalid(_call(K=-1), "negative K")
    _invalid(_call(K=(1 << 31) // 240 + 1), r"K \* 240")
    _invalid(_call(R=1 << 20, K=1 << 12), r"R \* K")
    # update alone needs no score output, but the counts, the history and folded
    none = {n: None for n in SCORE_OUT}
    _invalid(_call(mode=2, counts=None, **none), "null counts")
    _invalid(_call(mode=2, chist=None, **none), "null chist")
    _invalid(_call(mode=2, folded=None, **none), "null folded")
    _invalid(_call(mode=2, folded=2052, **none), "folded not 8-byte")


def test_empty_shapes_launch_nothing_and_score_alone_needs_no_folded():
    for mode in (1, 2, 3):
        assert _call(R=0, counts=None, chist=None, score=None, folded=None, mode=mode) == _native.NVRX_OK
        assert _call(K=0, counts=None, chist=None, tail_ns=None, folded=None, mode=mode) == _native.NVRX_OK
    assert _call(R=0, mode=1, folded=None) == _native.NVRX_OK


def test_bad_arguments_of_the_conversions():
    for name, call in ((FROM, _from), (TO, _to)):
        _invalid(call(R=-1), "negative R", name)
        _invalid(call(stride=-1), "negative stride", name)
        _invalid(call(stride=(1 << 31) // 240 + 1), r"stride \* 240", name)
        _invalid(call(R=1 << 20, stride=1 << 12), r"R \* stride", name)
        _invalid(call(hist=None), "null hist", name)
        _invalid(call(chist=None), "null chist", name)
        _invalid(call(hist=1032), "hist not 16-byte", name)
        _invalid(call(chist=72), "chist not 16-byte", name)
        assert call(R=0) == _native.NVRX_OK and call(stride=0) == _native.NVRX_OK
        assert call(R=0, hist=None, chist=None) == _native.NVRX_OK
    _invalid(_from(folded=132), "folded not 8-byte", FROM)
    assert _from(R=0, folded=None) == _native.NVRX_OK  # folded is optional


def test_wrappers_check_before_any_tensor():
    for bad in (-1, 1001, 0.5, True):
        with pytest.raises(ValueError, match="permille"):
            ops.histogram_history_scores_compact(None, None, permille=bad)
    with pytest.raises(ValueError, match="at least one"):
        ops.histogram_history_scores_compact(None, None, permille=990, score=False, update=False)


def test_reporter_refusals_come_before_any_allocation():
    # a reporter shell without a device: every refusal below must fire before a tensor is made
    rep = batch.MatrixReporter.__new__(batch.MatrixReporter)
    rep.R, rep.K, rep.exchange = 2, 3, False
    rep._htail = rep._ctail = rep._rtail = None
    rep._absorbed = {"dense": 0, "compact": 0}
    with pytest.raises(NotImplementedError, match="attribute"):
        rep.individual_tail_scores(None, attribute=4, history="compact")
    with pytest.raises(ValueError, match="history"):
        rep.individual_tail_scores(None, history="sparse")
    for to in ("compact", "dense"):
        with pytest.raises(RuntimeError, match="no (dense|compact) history"):
            rep.convert_tail_history(to)
    with pytest.raises(ValueError, match="to must be"):
        rep.convert_tail_history("sparse")
    rep.exchange = True
    with pytest.raises(NotImplementedError, match="exchange"):
        rep.individual_tail_scores(None, history="compact")
    with pytest.raises(NotImplementedError, match="exchange"):
        rep.convert_tail_history("compact")
    assert rep._htail is None and rep._ctail is None
