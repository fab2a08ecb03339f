"""nvrx_score_rank_attribution at the C boundary (no GPU): the symbol is exported and bound, the
ABI is still 6, the ctypes struct has the layout the C compiler gives ``nvrx_scorerank_args`` (as
C11 and as C++17), the host-side argument checks -- those of nvrx_score_attribution and those of
nvrx_rank_attribution -- run before any launch, each with a message, and R == 0 / K == 0
succeed."""
import ctypes
import os
import re
import subprocess

import pytest

from nvidia_resiliency_ext.straggler import _native, histograms, ops

NAME = "nvrx_score_rank_attribution"
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
ORDER = ["R", "K", "value_f64", "num", "med", "avg", "col_valid", "ref", "ref_index", "ref_missing",
         "hist", "hist_index", "hist_stride", "kind", "top", "row_valid", "idx", "loss", "score",
         "taken", "positive", "err", "work"]
FIELDS = [n for n, _ in _native.ScoreRankArgs._fields_]
INS = ("num", "med", "avg")
OUTS = ("idx", "loss", "score", "taken", "positive")


def _invalid(rc, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error().decode()
    assert msg.startswith(NAME + ": ") and re.search(word, msg), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def _call(**kw):
    f = dict(R=1, K=1, value_f64=0, num=16, med=16, avg=16, col_valid=None, ref=16, ref_index=None,
             ref_missing=None, hist=None, hist_index=None, hist_stride=0,
             kind=_native.NVRX_ATTR_RELATIVE, top=4, row_valid=None, idx=16, loss=16, score=16,
             taken=16, positive=16, err=None, work=None)
    f.update(kw)
    a = _native.ScoreRankArgs(*(f[n] for n in FIELDS))
    return getattr(_native.lib(), NAME)(ctypes.byref(a), None)


def test_symbol_loaded_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    assert hasattr(raw, NAME) and NAME in _native.SIGNATURES
    assert getattr(L, NAME).argtypes == _native.SIGNATURES[NAME][1]
    assert L.nvrx_abi_version() == _native.ABI_VERSION == 6  # additive
    assert callable(ops.score_rank_attribution) and callable(histograms.score_rank_attribution)
    assert callable(histograms.score_losses)
    assert "ops.score_rank_attribution" in histograms.score_rank_attribution.__doc__
    with open(os.path.join(INC, "nvrx_straggler.h")) as f:
        text = f.read()
    assert NAME in text.split("*/", 1)[0]  # listed in the header's index comment
    assert "#define NVRX_ABI_VERSION 6\n" in text
    assert "ONE PLAN SERVES BOTH ENTRIES" in text and "nvrx_score_rank_attribution_plan" not in text


def test_field_order():
    assert FIELDS == ORDER


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")])
def test_struct_layout_matches_the_c_compiler(tmp_path, compiler, std, ext):
    src = tmp_path / f"probe.{ext}"
    lines = "".join(f'    printf("{n} %zu\\n", offsetof(nvrx_scorerank_args, {n}));\n' for n in ORDER)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nvrx_straggler.h"\n'
                   'int main(void) {\n    printf("sizeof %zu\\n", sizeof(nvrx_scorerank_args));\n'
                   '    /* the prototype, unevaluated: nothing to link */\n'
                   '    (void)sizeof(nvrx_score_rank_attribution((const nvrx_scorerank_args*)0, (void*)0));\n'
                   f'{lines}    return 0;\n}}\n')
    exe = tmp_path / "probe"
    subprocess.run([compiler, std, "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)], check=True)
    out = dict(l.split(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == ctypes.sizeof(_native.ScoreRankArgs)
    assert list(out) == ORDER
    offsets = [int(out[n]) for n in ORDER]
    assert offsets == sorted(offsets) and len(set(offsets)) == len(offsets)  # declared in this order
    for n in ORDER:
        assert int(out[n]) == getattr(_native.ScoreRankArgs, n).offset, n


def test_bad_arguments():
    _invalid(getattr(_native.lib(), NAME)(None, None), "args")
    for top in (0, 17, -1):
        _invalid(_call(top=top), "top")
    for kind in (-1, 2):
        _invalid(_call(kind=kind), "kind")
    _invalid(_call(R=-1), "negative R")
    _invalid(_call(K=-1), "negative K")
    _invalid(_call(R=1 << 31), "R must be below")
    _invalid(_call(K=1 << 31), "K must be below")
    _invalid(_call(value_f64=2), "value_f64")
    _invalid(_call(hist_index=16), "hist_index requires hist_stride")
    for n in INS + OUTS:
        _invalid(_call(**{n: None}), "null " + n)
    _invalid(_call(ref=None), "relative kind needs ref")
    _invalid(_call(kind=_native.NVRX_ATTR_INDIVIDUAL), "individual kind needs hist")
    _invalid(_call(R=65, K=1), "null work")  # two splits: the plan needs a work space
    for n in ("loss", "score"):
        _invalid(_call(**{n: 20}), n + " not 8-byte")
    _invalid(_call(R=65, K=1, work=20), "work not 8-byte")


def test_empty_shapes_launch_nothing():
    none = {n: None for n in INS + OUTS + ("ref",)}
    assert _call(R=0) == _native.NVRX_OK
    assert _call(R=0, **none) == _native.NVRX_OK
    assert _call(K=0, **none) == _native.NVRX_OK
    assert _call(K=0, kind=_native.NVRX_ATTR_INDIVIDUAL, **none) == _native.NVRX_OK


def test_ops_wrapper_checks_before_any_tensor():
    for bad in (0, 17, True, 1.5):
        with pytest.raises(ValueError, match="top"):
            ops.score_rank_attribution(None, None, None, top=bad, kind="relative")
    with pytest.raises(ValueError, match="kind"):
        ops.score_rank_attribution(None, None, None, top=4, kind="sections")
