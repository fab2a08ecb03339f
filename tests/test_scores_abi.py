"""CPU: the host-side argument checks of the scoring and section entry points run before any
launch (no GPU needed; fake non-null pointers, so nothing is dereferenced): NVRX_ERR_INVALID with
a message naming the argument, and the zero-size forms return NVRX_OK without a device."""
import ctypes
import re

import pytest

from nvidia_resiliency_ext.straggler import _native

P = 16  # a non-null "pointer": never dereferenced, every call here stops at a host check


def _invalid(rc, word):
    assert rc == _native.NVRX_ERR_INVALID
    msg = _native.lib().nvrx_last_error().decode()
    assert re.search(word, msg), (word, msg)
    with pytest.raises(RuntimeError, match=word):
        _native.check(rc, "x")


def _score_args(**kw):
    f = dict(R=1, K=1, value_f64=0, num=P, med=P, avg=P, col_valid=None, ref=P, ref_index=None,
             ref_missing=None, hist=None, hist_index=None, hist_stride=0, partials=P, err=None,
             round_f32=0, thr_rel=0.75, thr_ind=0.75, gpu_rel=None, gpu_ind=None, strag_rel=None,
             strag_ind=None, done=None, reset_col_ref=None, reset_ncols=0)
    f.update(kw)
    return _native.ScoreArgs(*(f[name] for name, _ in _native.ScoreArgs._fields_))


def _scores(**kw):
    return _native.lib().nvrx_scores(ctypes.byref(_score_args(**kw)), None)


def _kernel_ref(num=P, med=P, R=1, K=1, ref=P, scratch=P):
    return _native.lib().nvrx_kernel_ref(num, med, R, K, ref, scratch, None)


def _finalize(partials=P, R=1, nshards=1):
    return _native.lib().nvrx_finalize_scores(partials, R, nshards, 0, 0.75, 0.75, P, P, P, P, None, None)


def _section_scores(med=P, present=P, R=1, S=1, ref_in=None, ref_index=None, ref_work=P, hist=P,
                    out_rel=P, out_ind=P):
    return _native.lib().nvrx_section_scores(med, present, R, S, ref_in, ref_index, ref_work, hist,
                                             0, out_rel, out_ind, None, None)


def _section_stats(vals=P, off=P, nsec=1, max_len=8, outs=(P,) * 6):
    return _native.lib().nvrx_section_stats(vals, off, nsec, max_len, *outs, None)


def _pack(med=P, ids=P, n=1, times=P, total=1):
    return _native.lib().nvrx_pack_min_times(med, ids, n, times, total, None)


def _stragglers(score=P, n=1, mask=P):
    return _native.lib().nvrx_stragglers(score, n, 0.75, mask, None)


def test_kernel_ref_row_limit_is_the_launchers():
    # 32 rows per block of grid.y, at most 65535 blocks: one row more is refused up front
    _invalid(_kernel_ref(R=32 * 65535 + 1), "too many rows")
    _invalid(_kernel_ref(R=1 << 40), "too many rows")


def test_kernel_ref_arguments():
    _invalid(_kernel_ref(R=-1), "negative size")
    _invalid(_kernel_ref(K=-1), "negative size")
    _invalid(_kernel_ref(ref=None), "ref")
    _invalid(_kernel_ref(scratch=None), "scratch")
    _invalid(_kernel_ref(num=None), "num")
    _invalid(_kernel_ref(med=None), "med")


def test_scores_arguments():
    assert _native.lib().nvrx_scores(None, None) == _native.NVRX_ERR_INVALID
    _invalid(_native.lib().nvrx_scores(None, None), "args")
    _invalid(_scores(R=-1), "negative size")
    _invalid(_scores(K=-1), "negative size")
    _invalid(_scores(partials=None), "no output")
    for name in ("num", "med", "avg"):
        _invalid(_scores(**{name: None}), name)
    _invalid(_scores(hist=P, hist_index=P), "hist_index requires hist_stride")
    _invalid(_scores(value_f64=2), "value_f64")
    _invalid(_scores(value_f64=-1), "value_f64")
    _invalid(_scores(reset_col_ref=P, reset_ncols=4), "reset_col_ref needs done")
    _invalid(_scores(done=P, reset_ncols=4), "reset_col_ref")
    _invalid(_scores(done=P, reset_col_ref=P, reset_ncols=-1), "reset_ncols")


def test_finalize_scores_arguments():
    _invalid(_finalize(R=-1), "R")
    _invalid(_finalize(nshards=0), "nshards")
    _invalid(_finalize(nshards=-2), "nshards")
    _invalid(_finalize(partials=None), "partials")


def test_section_scores_arguments():
    _invalid(_section_scores(R=-1), "negative size")
    _invalid(_section_scores(S=-1), "negative size")
    _invalid(_section_scores(med=None), "med")
    _invalid(_section_scores(present=None), "present")
    _invalid(_section_scores(hist=None), "individual scores need hist")
    _invalid(_section_scores(ref_work=None), "ref_in or ref_work")


def test_section_stats_arguments():
    _invalid(_section_stats(nsec=-1), "negative size")
    _invalid(_section_stats(max_len=-1), "negative size")
    _invalid(_section_stats(vals=None), "null array")
    _invalid(_section_stats(off=None), "null array")
    for i in range(6):
        _invalid(_section_stats(outs=(P,) * i + (None,) + (P,) * (5 - i)), "null array")


def test_pack_min_times_arguments():
    _invalid(_pack(n=-1), "negative size")
    _invalid(_pack(total=-1), "negative size")
    _invalid(_pack(times=None), "times")
    _invalid(_pack(med=None), "null inputs")
    _invalid(_pack(ids=None), "null inputs")
    _invalid(_pack(n=2, total=1), "n > total")


def test_stragglers_arguments():
    _invalid(_stragglers(n=-1), "negative n")
    _invalid(_stragglers(score=None), "score")
    _invalid(_stragglers(mask=None), "mask")


def test_zero_sizes_launch_nothing():
    OK = _native.NVRX_OK
    assert _kernel_ref(num=None, med=None, R=5, K=0, ref=None, scratch=None) == OK
    assert _scores(R=0, num=None, med=None, avg=None, partials=None, ref=None) == OK
    assert _finalize(partials=None, R=0) == OK
    assert _section_scores(med=None, present=None, R=0, S=3) == OK
    assert _section_scores(med=None, present=None, R=3, S=0) == OK
    assert _section_stats(vals=None, off=None, nsec=0, outs=(None,) * 6) == OK
    assert _stragglers(score=None, n=0, mask=None) == OK
    assert _pack(med=None, ids=None, n=0, times=None, total=0) == OK
