"""nvrx_rank_attribution / nvrx_rank_attribution_plan at the C boundary.  CPU: the symbols are
exported and bound, the ABI is still 6, the ctypes struct has the layout the C compiler gives
``nvrx_rankattr_args`` (as C11 and as C++17), the plan function keeps its promises, and the
host-side argument checks run before any launch.  GPU (marked): the same argument errors on the
device's own pointers, and R == 0 / K == 0 leave sentinel-filled outputs untouched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from nvidia_resiliency_ext.straggler import _native, histograms, ops

NAME = "nvrx_rank_attribution"
PLAN = "nvrx_rank_attribution_plan"
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
ORDER = ["R", "K", "loss", "ld", "row_valid", "top", "idx", "loss_out", "taken", "positive", "work"]
FIELDS = [n for n, _ in _native.RankAttrArgs._fields_]
OUTS = ("idx", "loss_out", "taken", "positive")


def _invalid(rc, word, name=NAME):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error().decode()
    assert msg.startswith(name + ": ") and re.search(word, msg), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def _call(**kw):
    f = dict(R=1, K=1, loss=16, ld=0, row_valid=None, top=4, idx=16, loss_out=16, taken=16,
             positive=16, work=None)
    f.update(kw)
    a = _native.RankAttrArgs(*(f[n] for n in FIELDS))
    return getattr(_native.lib(), NAME)(ctypes.byref(a), None)


def _plan(R, K, top):
    t, s, w = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = getattr(_native.lib(), PLAN)(R, K, top, ctypes.byref(t), ctypes.byref(s), ctypes.byref(w))
    assert rc == _native.NVRX_OK
    return t.value, s.value, w.value


def test_symbols_loaded_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    for n in (NAME, PLAN):
        assert hasattr(raw, n) and n in _native.SIGNATURES
        assert getattr(L, n).argtypes == _native.SIGNATURES[n][1]
    assert L.nvrx_abi_version() == _native.ABI_VERSION == 6  # additive
    assert callable(ops.rank_attribution) and callable(histograms.rank_attribution)
    assert "ops.rank_attribution" in histograms.rank_attribution.__doc__
    with open(os.path.join(INC, "nvrx_straggler.h")) as f:
        text = f.read()
    assert NAME in text.split("*/", 1)[0]  # listed in the header's index comment
    assert "#define NVRX_ABI_VERSION 6\n" in text


def test_field_order():
    assert FIELDS == ORDER


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")])
def test_struct_layout_matches_the_c_compiler(tmp_path, compiler, std, ext):
    src = tmp_path / f"probe.{ext}"
    lines = "".join(f'    printf("{n} %zu\\n", offsetof(nvrx_rankattr_args, {n}));\n' for n in ORDER)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nvrx_straggler.h"\n'
                   'int main(void) {\n    printf("sizeof %zu\\n", sizeof(nvrx_rankattr_args));\n'
                   '    /* the prototypes, unevaluated: nothing to link */\n'
                   '    (void)sizeof(nvrx_rank_attribution((const nvrx_rankattr_args*)0, (void*)0));\n'
                   '    (void)sizeof(nvrx_rank_attribution_plan((int64_t)1, (int64_t)1, (int32_t)1,\n'
                   '                 (int64_t*)0, (int64_t*)0, (int64_t*)0));\n'
                   f'{lines}    return 0;\n}}\n')
    exe = tmp_path / "probe"
    subprocess.run([compiler, std, "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)], check=True)
    out = dict(l.split(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == ctypes.sizeof(_native.RankAttrArgs)
    assert list(out) == ORDER
    offsets = [int(out[n]) for n in ORDER]
    assert offsets == sorted(offsets) and len(set(offsets)) == len(offsets)  # declared in this order
    for n in ORDER:
        assert int(out[n]) == getattr(_native.RankAttrArgs, n).offset, n


def test_plan_small_R_is_one_split_without_work():
    for R in (1, 3, 4, 5, 63, 64):
        for K in (1, 64, 65, 4096):
            for top in (1, 8, 16):
                tiles, splits, work = _plan(R, K, top)
                assert (tiles, splits, work) == ((K + 63) // 64, 1, 0), (R, K, top)
    assert _plan(65, 1, 4)[1] == 2  # the other side of the gate


def test_plan_splits_and_work_bytes():
    for K in (1, 63, 64, 65, 130, 2048, 131072):
        for top in (1, 4, 8, 16):
            prev = 0
            for R in (1, 64, 65, 128, 129, 257, 1024, 4096, 16384, 1 << 20):
                if R * K >= 1 << 31:
                    continue
                tiles, splits, work = _plan(R, K, top)
                assert tiles == (K + 63) // 64 and splits >= 1
                assert splits <= (R + 63) // 64  # a split is no shorter than 64 rows ...
                assert tiles * splits < 2048 + tiles  # ... and the grid is about 2048 workgroups
                assert (work == 0) == (splits == 1)
                assert work >= prev, (R, K, top)  # monotone in R
                prev = work
    for R, K in ((257, 130), (16384, 2048)):
        works = [_plan(R, K, top)[2] for top in range(1, 17)]
        assert works == sorted(works) and works[0] > 0  # monotone in top
        assert len({_plan(R, K, top)[:2] for top in range(1, 17)}) == 1  # the grid is not top's
    assert _plan(16384, 2048, 8)[:2] == (32, 64)  # about 2048 workgroups
    assert _plan(65, 2048 * 64, 8) == (2048, 1, 0)  # the grid bound, not R, decides here


def test_plan_empty_shapes_and_null_outputs():
    assert _plan(0, 5, 4) == (0, 1, 0)
    assert _plan(5, 0, 4) == (0, 1, 0)
    assert getattr(_native.lib(), PLAN)(100, 100, 4, None, None, None) == _native.NVRX_OK
    assert ops.rank_attribution_plan(257, 130, 16) == _plan(257, 130, 16)


def test_plan_bad_arguments():
    plan = getattr(_native.lib(), PLAN)
    for top in (0, 17, -1):
        _invalid(plan(1, 1, top, None, None, None), "top", PLAN)
    _invalid(plan(-1, 1, 4, None, None, None), "negative R", PLAN)
    _invalid(plan(1, -1, 4, None, None, None), "negative K", PLAN)


def test_bad_arguments():
    _invalid(getattr(_native.lib(), NAME)(None, None), "args")
    for top in (0, 17, -1):
        _invalid(_call(top=top), "top")
    _invalid(_call(R=-1), "negative R")
    _invalid(_call(K=-1), "negative K")
    _invalid(_call(K=3, ld=2), "ld below K")
    _invalid(_call(R=1 << 20, K=1 << 12), r"R \* ld")
    _invalid(_call(R=1 << 20, K=1, ld=1 << 12), r"R \* ld")
    for n in ("loss",) + OUTS:
        _invalid(_call(**{n: None}), "null " + n)
    _invalid(_call(R=65, K=1), "null work")  # two splits: the plan needs a work space
    for n in ("loss", "loss_out"):
        _invalid(_call(**{n: 20}), n + " not 8-byte")
    _invalid(_call(R=65, K=1, work=20), "work not 8-byte")


def test_empty_shapes_launch_nothing():
    none = {n: None for n in ("loss",) + OUTS}
    assert _call(R=0) == _native.NVRX_OK
    assert _call(R=0, **none) == _native.NVRX_OK
    assert _call(K=0, **none) == _native.NVRX_OK


def test_ops_wrapper_checks_before_any_tensor():
    for bad in (0, 17, True, 1.5):
        with pytest.raises(ValueError, match="top"):
            ops.rank_attribution(None, top=bad)


@pytest.mark.gpu
def test_gpu_argument_errors_and_untouched_outputs():
    import torch

    d = torch.device("cuda:0")
    R, K, top = 65, 3, 4
    loss = torch.zeros((R, K), dtype=torch.float64, device=d)
    out = ops.RankAttribution.empty(K, top, d)
    work = torch.empty(ops.rank_attribution_plan(R, K, top)[2] + 8, dtype=torch.uint8, device=d)
    good = dict(R=R, K=K, loss=loss.data_ptr(), top=top, idx=out.idx.data_ptr(),
                loss_out=out.loss.data_ptr(), taken=out.taken.data_ptr(),
                positive=out.positive.data_ptr(), work=work.data_ptr())
    for top_ in (0, 17):
        _invalid(_call(**dict(good, top=top_)), "top")
    _invalid(_call(**dict(good, work=None)), "null work")
    _invalid(_call(**dict(good, work=work.data_ptr() + 4)), "work not 8-byte")
    _invalid(_call(**dict(good, loss=loss.data_ptr() + 4)), "loss not 8-byte")
    _invalid(_call(**dict(good, loss_out=out.loss.data_ptr() + 4)), "loss_out not 8-byte")
    _invalid(_call(**dict(good, ld=2)), "ld below K")
    for n in ("loss",) + OUTS:
        _invalid(_call(**dict(good, **{n: None})), "null " + n)
    # R == 0 / K == 0: nothing is launched, sentinels stay
    for shape in ((0, K), (R, 0)):
        o = ops.RankAttribution.empty(K, top, d)
        o.idx.fill_(-77), o.loss.fill_(-77.0), o.taken.fill_(-77), o.positive.fill_(-77)
        f = dict(good, R=shape[0], K=shape[1], idx=o.idx.data_ptr(), loss_out=o.loss.data_ptr(),
                 taken=o.taken.data_ptr(), positive=o.positive.data_ptr())
        assert _call(**f) == _native.NVRX_OK
        torch.cuda.synchronize()
        assert (o.idx == -77).all() and (o.loss == -77.0).all()
        assert (o.taken == -77).all() and (o.positive == -77).all()
    # and the good call runs
    assert _call(**good) == _native.NVRX_OK
    torch.cuda.synchronize()
    assert out.idx.cpu().numpy().tolist() == [[0, 1, 2, 3]] * K
    assert np.array_equal(out.taken.cpu().numpy(), np.full(K, R, np.int32))
