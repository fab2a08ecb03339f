"""CPU: nvrx_compact_history_age and nvrx_histogram_history_age are exported and bound, the ABI is
still 6, the prototypes in the header compile as C11 and as C++17, and the host-side argument
checks run before any launch (NVRX_ERR_INVALID with a message that names the argument)."""
import ctypes
import os
import re
import subprocess

import pytest

from nvidia_resiliency_ext.straggler import _native, batch, histograms, ops
from nvidia_resiliency_ext.straggler.straggler import Detector

COMPACT = "nvrx_compact_history_age"
DENSE = "nvrx_histogram_history_age"
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def _invalid(rc, name, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error().decode()
    assert msg.startswith(name + ": ") and re.search(word, msg), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def _compact(**kw):
    # distinct fake addresses: nothing is launched before a check fails, or with R or stride of 0
    f = dict(chist=64, R=1, stride=1, shift=1, evicted=128, full=136)
    f.update(kw)
    return _native.lib().nvrx_compact_history_age(f["chist"], f["R"], f["stride"], f["shift"],
                                                  f["evicted"], f["full"], None)


def _dense(**kw):
    f = dict(hist=64, R=1, stride=1, shift=1)
    f.update(kw)
    return _native.lib().nvrx_histogram_history_age(f["hist"], f["R"], f["stride"], f["shift"], None)


def test_symbols_loaded_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    for name in (COMPACT, DENSE):
        assert hasattr(raw, name) and name in _native.SIGNATURES
        assert getattr(L, name).argtypes == _native.SIGNATURES[name][1]
    assert L.nvrx_abi_version() == _native.ABI_VERSION == 6  # additive
    assert callable(ops.compact_history_age) and callable(ops.histogram_history_age)
    assert callable(histograms.compact_age) and callable(histograms.history_age)
    assert callable(batch.MatrixReporter.age_tail_history) and callable(Detector.age_tail_history)
    with open(os.path.join(INC, "nvrx_straggler.h")) as f:
        text = f.read()
    index = text.split("*/", 1)[0]  # listed in the header's index comment
    assert COMPACT in index and DENSE in index
    assert re.search(r"#define NVRX_ABI_VERSION 6\b", text)


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")])
def test_prototypes_compile(tmp_path, compiler, std, ext):
    src = tmp_path / f"probe.{ext}"
    src.write_text('#include <stdint.h>\n#include "nvrx_straggler.h"\n'
                   'int main(void) {\n'
                   '    /* the prototypes, unevaluated: nothing to link */\n'
                   '    (void)sizeof(nvrx_compact_history_age((void*)0, (int64_t)1, (int64_t)1, '
                   '(int32_t)1, (uint64_t*)0, (uint64_t*)0, (void*)0));\n'
                   '    (void)sizeof(nvrx_histogram_history_age((uint32_t*)0, (int64_t)1, (int64_t)1, '
                   '(int32_t)1, (void*)0));\n'
                   '    return 0;\n}\n')
    subprocess.run([compiler, std, "-Wall", "-Werror", "-I", INC, str(src), "-o",
                    str(tmp_path / "probe")], check=True)


def test_compact_bad_arguments():
    _invalid(_compact(chist=None), COMPACT, "null chist")
    _invalid(_compact(chist=72), COMPACT, "chist not 16-byte")
    _invalid(_compact(evicted=132), COMPACT, "evicted not 8-byte")
    _invalid(_compact(full=1028), COMPACT, "full not 8-byte")
    _invalid(_compact(full=128), COMPACT, "full aliases evicted")
    for s in (0, 32, -1, 64):
        _invalid(_compact(shift=s), COMPACT, "shift")
    _invalid(_compact(R=-1), COMPACT, "negative R")
    _invalid(_compact(stride=-1), COMPACT, "negative stride")
    _invalid(_compact(R=1 << 20, stride=1 << 11), COMPACT, r"R \* stride")
    _invalid(_compact(R=1, stride=1 << 31), COMPACT, r"R \* stride")


def test_dense_bad_arguments():
    _invalid(_dense(hist=None), DENSE, "null hist")
    _invalid(_dense(hist=72), DENSE, "hist not 16-byte")
    for s in (0, 32, -1):
        _invalid(_dense(shift=s), DENSE, "shift")
    _invalid(_dense(R=-1), DENSE, "negative R")
    _invalid(_dense(stride=-1), DENSE, "negative stride")
    _invalid(_dense(stride=(1 << 31) // 240 + 1), DENSE, r"stride \* 240")
    _invalid(_dense(R=1 << 20, stride=1 << 11), DENSE, r"R \* stride must")
    # 2^26 elements are fine for the compact entry's limit, their 2^26 * 60 vectors are not
    _invalid(_dense(R=1 << 13, stride=1 << 13), DENSE, "vectors")


def test_empty_shapes_launch_nothing_and_need_no_pointer():
    for kw in (dict(R=0), dict(stride=0), dict(R=0, stride=0)):
        assert _compact(chist=None, evicted=None, full=None, **kw) == _native.NVRX_OK
        assert _compact(**kw) == _native.NVRX_OK
        assert _dense(hist=None, **kw) == _native.NVRX_OK
    # the checks of the other arguments still run
    _invalid(_compact(R=0, shift=0), COMPACT, "shift")
    _invalid(_dense(stride=0, hist=8), DENSE, "hist not 16-byte")


def test_wrappers_check_before_any_tensor():
    for bad in (0, 32, -1, 1.5, True):
        with pytest.raises(ValueError, match="shift"):
            ops.compact_history_age(None, bad)
        with pytest.raises(ValueError, match="shift"):
            ops.histogram_history_age(None, bad)
