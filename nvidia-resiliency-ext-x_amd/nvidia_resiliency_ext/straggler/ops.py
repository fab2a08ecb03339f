"""Torch-tensor front end of the HIP kernels (thin: allocation + argument marshalling).

Every function takes/returns device tensors and enqueues work on the current HIP stream;
all arithmetic happens in libnvrx_hip.so.  Shape checks run on the host before any
launch (the C layer re-checks).
"""
from __future__ import annotations

import ctypes
import numbers
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native as N

STATS_FAST = N.NVRX_STATS_FAST
STATS_EXACT = N.NVRX_STATS_EXACT


@dataclass
class SegmentStats:
    """SoA statistics of a batch of segments (device tensors, float32 microseconds)."""

    num: torch.Tensor
    min: torch.Tensor
    max: torch.Tensor
    med: torch.Tensor
    avg: torch.Tensor
    std: torch.Tensor

    @classmethod
    def empty(cls, n: int, device) -> "SegmentStats":
        f = lambda dt: torch.empty(n, dtype=dt, device=device)  # noqa: E731
        return cls(f(torch.int32), f(torch.float32), f(torch.float32), f(torch.float32),
                   f(torch.float32), f(torch.float32))

    def view(self, *shape) -> "SegmentStats":
        return SegmentStats(*(getattr(self, k).view(*shape) for k in
                              ("num", "min", "max", "med", "avg", "std")))

    def soa(self) -> N.StatsSoA:
        return N.StatsSoA(self.num.data_ptr(), self.min.data_ptr(), self.max.data_ptr(),
                          self.med.data_ptr(), self.avg.data_ptr(), self.std.data_ptr())

    def cpu(self) -> "SegmentStats":
        return SegmentStats(*(getattr(self, k).cpu() for k in
                              ("num", "min", "max", "med", "avg", "std")))


def _stream(stream):
    return N.stream_handle(stream)


def _check_strided(ns, nseg, seg_stride, seg_begin, seg_len):
    """The strided triple of every segment_*_strided call: device u32 keys holding all segments."""
    N.require_device(ns, "ns")
    if ns.dtype not in (torch.int32, torch.uint32):
        raise TypeError("ns must be a 32-bit integer tensor of duration keys")
    if nseg > 0 and (nseg - 1) * seg_stride + seg_begin + seg_len > ns.numel():
        raise ValueError("segments exceed the ns tensor")


def _check_ragged(ns, seg_off, seg_len) -> int:
    """The ragged triple of every segment_*_ragged call; returns nseg (seg_len None: seg_off
    holds nseg + 1 offsets)."""
    N.require_device(ns, "ns")
    N.require_device(seg_off, "seg_off")
    if ns.dtype not in (torch.int32, torch.uint32):
        raise TypeError("ns must be a 32-bit integer tensor of duration keys")
    if seg_off.dtype != torch.int64 or (seg_len is not None and seg_len.dtype != torch.int32):
        raise TypeError("seg_off must be int64 and seg_len int32")
    if seg_len is not None:
        N.require_device(seg_len, "seg_len")
    return seg_off.numel() - (0 if seg_len is not None else 1)


def _num_output(num, nseg):
    if num is not None:
        N.require_device(num, "num")
        if num.dtype != torch.int32 or num.numel() < nseg or not num.is_contiguous():
            raise ValueError("num must be a contiguous int32 tensor of >= nseg elements")


def segment_stats_strided(ns: torch.Tensor, nseg: int, seg_stride: int, seg_begin: int,
                          seg_len: int, cap: int = 0, mode: int = STATS_FAST,
                          out: Optional[SegmentStats] = None, col_ref: Optional[torch.Tensor] = None,
                          ncols: int = 0, stream=None, colref_ready: bool = False) -> SegmentStats:
    """Stats of segments ns.flat[s*seg_stride + seg_begin : +seg_len] (u32 duration keys,
    ``_native.duration_keys``: plain ns below 3.76 s -- raw u32 ns of 3.76 s and more need
    ``encode_ns_u32_`` first; a u32 above ``_native.KEY_MAX`` comes from no u64 duration), last
    `cap` samples retained (CircularBuffer.h:53-69).  reference: CuptiProfiler.cpp:44-74."""
    _check_strided(ns, nseg, seg_stride, seg_begin, seg_len)
    if out is None:
        out = SegmentStats.empty(nseg, ns.device)
    soa = out.soa()
    if col_ref is not None and (col_ref.numel() < 2 * ncols or col_ref.dtype != torch.int32):
        raise ValueError("col_ref must be an int32 tensor of >= 2*ncols elements")
    if colref_ready:  # col_ref holds the initial reference already (a previous scores epilogue)
        mode |= N.NVRX_STATS_COLREF_READY
    N.call("nvrx_segment_stats_strided", ns.data_ptr(), nseg, seg_stride, seg_begin, seg_len,
           cap, mode, ctypes.byref(soa), N.ptr(col_ref), ncols, _stream(stream))
    return out


def encode_ns_u32_(ns: torch.Tensor, stream=None) -> torch.Tensor:
    """In place: raw u32 integer-ns durations (any value below 2^32, never encoded) -> duration
    keys.  Values below 3.76 s are unchanged; from 3.76 s up they become the key of f32(ns), the
    value CuptiProfiler.cpp:187 keeps.  Not idempotent: encode raw ns once."""
    N.require_device(ns, "ns")
    if ns.dtype not in (torch.int32, torch.uint32) or not ns.is_contiguous():
        raise TypeError("ns must be a contiguous 32-bit integer tensor")
    N.call("nvrx_encode_ns_u32", ns.data_ptr(), ns.numel(), _stream(stream))
    return ns


def segment_stats_ragged(ns: torch.Tensor, seg_off: torch.Tensor, seg_len: Optional[torch.Tensor],
                         max_len: int, cap: int = 0, mode: int = STATS_FAST, aligned16: bool = False,
                         out: Optional[SegmentStats] = None, col_ref: Optional[torch.Tensor] = None,
                         ncols: int = 0, stream=None) -> SegmentStats:
    """Stats of ragged segments; segments of <= 128 retained samples are bit-exact in every
    field.  col_ref ([2*ncols] int32): fused per-column reference, as for the strided call."""
    nseg = _check_ragged(ns, seg_off, seg_len)
    if out is None:
        out = SegmentStats.empty(max(nseg, 0), ns.device)
    soa = out.soa()
    N.call("nvrx_segment_stats_ragged", ns.data_ptr(), seg_off.data_ptr(),
           N.ptr(seg_len), nseg, max_len, cap, mode, int(aligned16), ctypes.byref(soa),
           N.ptr(col_ref), ncols if col_ref is not None else 0, _stream(stream))
    return out


def permille_array(permille):
    """The quantile requests as the C ABI takes them (a host int32 array): a non-empty
    sequence of at most ``_native.NVRX_MAX_QUANTILES`` ints in [0, 1000]; ValueError if not."""
    try:
        pm = list(permille)
    except TypeError:
        raise ValueError("permille must be a sequence of ints in [0, 1000]") from None
    if not 1 <= len(pm) <= N.NVRX_MAX_QUANTILES:
        raise ValueError(f"permille must hold 1 to {N.NVRX_MAX_QUANTILES} entries, got {len(pm)}")
    for v in pm:
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v <= 1000:
            raise ValueError(f"permille entries must be ints in [0, 1000], got {v!r}")
    return (ctypes.c_int32 * len(pm))(*(int(v) for v in pm))


def _quantile_outputs(nq, nseg, device, out, num):
    if out is None:
        out = torch.empty((nq, nseg), dtype=torch.float32, device=device)
    N.require_device(out, "out")
    if out.dtype != torch.float32 or tuple(out.shape) != (nq, nseg) or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of shape [nq, nseg]")
    _num_output(num, nseg)
    return out


def segment_quantiles_strided(ns: torch.Tensor, nseg: int, seg_stride: int, seg_begin: int,
                              seg_len: int, permille, cap: int = 0,
                              out: Optional[torch.Tensor] = None, num: Optional[torch.Tensor] = None,
                              stream=None) -> torch.Tensor:
    """Quantiles of the segments of ``segment_stats_strided`` (same addressing, same ring
    retention).  ``permille``: up to 8 ints in [0, 1000]; row j of the returned [nq, nseg] float32
    tensor holds, per segment of n retained samples, the sample of 0-based rank
    ``(permille[j] * (n - 1)) // 1000`` among the sorted duration keys, in us -- a sample, never an
    interpolation (0 -> MIN, 1000 -> MAX, 500 of an odd n -> MED, bit for bit); NaN for an empty
    segment.  ``num`` (int32 [nseg], optional) receives the retained lengths."""
    pm = permille_array(permille)
    _check_strided(ns, nseg, seg_stride, seg_begin, seg_len)
    out = _quantile_outputs(len(pm), max(nseg, 0), ns.device, out, num)
    N.call("nvrx_segment_quantiles_strided", ns.data_ptr(), nseg, seg_stride, seg_begin, seg_len,
           cap, pm, len(pm), out.data_ptr(), N.ptr(num), _stream(stream))
    return out


def segment_quantiles_ragged(ns: torch.Tensor, seg_off: torch.Tensor, seg_len: Optional[torch.Tensor],
                             max_len: int, permille, cap: int = 0, aligned16: bool = False,
                             out: Optional[torch.Tensor] = None, num: Optional[torch.Tensor] = None,
                             stream=None) -> torch.Tensor:
    """Quantiles of the ragged segments of ``segment_stats_ragged`` ([nq, nseg] float32, as
    ``segment_quantiles_strided``); every segment is read by its own retained length, a
    segment with ``seg_len < 0`` is skipped (its outputs untouched)."""
    pm = permille_array(permille)
    nseg = _check_ragged(ns, seg_off, seg_len)
    out = _quantile_outputs(len(pm), max(nseg, 0), ns.device, out, num)
    N.call("nvrx_segment_quantiles_ragged", ns.data_ptr(), seg_off.data_ptr(), N.ptr(seg_len),
           max(nseg, 0), max_len, cap, int(aligned16), pm, len(pm), out.data_ptr(), N.ptr(num),
           _stream(stream))
    return out


def _histogram_request(out, accumulate):
    # checked first: no tensor is looked at
    if accumulate and out is None:
        raise ValueError("accumulate=True needs out, the counts to add to")


def _histogram_outputs(nseg, device, out, num):
    if out is None:
        out = torch.empty((nseg, N.HIST_BINS), dtype=torch.int32, device=device)
    N.require_device(out, "out")
    if (out.dtype != torch.int32 or tuple(out.shape) != (nseg, N.HIST_BINS) or
            not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError("out must be a contiguous, 16-byte aligned int32 tensor of shape [nseg, 240]")
    _num_output(num, nseg)
    return out


def segment_histogram_strided(ns: torch.Tensor, nseg: int, seg_stride: int, seg_begin: int,
                              seg_len: int, cap: int = 0, out: Optional[torch.Tensor] = None,
                              num: Optional[torch.Tensor] = None, accumulate: bool = False,
                              stream=None) -> torch.Tensor:
    """Fixed-bucket duration histograms of the segments of ``segment_stats_strided`` (same
    addressing, same ring retention): an int32 [nseg, 240] tensor of counts over the buckets of
    ``histograms`` (the same edges for every segment, so counts add over ranks and reports).
    ``out``: counts to write, or with ``accumulate=True`` to add to (then required); ``num``
    (int32 [nseg], optional) receives the retained lengths.  An empty segment counts nothing."""
    _histogram_request(out, accumulate)
    _check_strided(ns, nseg, seg_stride, seg_begin, seg_len)
    out = _histogram_outputs(max(nseg, 0), ns.device, out, num)
    N.call("nvrx_segment_histogram_strided", ns.data_ptr(), nseg, seg_stride, seg_begin, seg_len,
           cap, int(bool(accumulate)), out.data_ptr(), N.ptr(num), _stream(stream))
    return out


def segment_histogram_ragged(ns: torch.Tensor, seg_off: torch.Tensor, seg_len: Optional[torch.Tensor],
                             max_len: int, cap: int = 0, aligned16: bool = False,
                             out: Optional[torch.Tensor] = None, num: Optional[torch.Tensor] = None,
                             accumulate: bool = False, stream=None) -> torch.Tensor:
    """Histograms of the ragged segments of ``segment_stats_ragged`` (int32 [nseg, 240], as
    ``segment_histogram_strided``); a segment with ``seg_len < 0`` is skipped (its outputs
    untouched)."""
    _histogram_request(out, accumulate)
    nseg = _check_ragged(ns, seg_off, seg_len)
    out = _histogram_outputs(max(nseg, 0), ns.device, out, num)
    N.call("nvrx_segment_histogram_ragged", ns.data_ptr(), seg_off.data_ptr(), N.ptr(seg_len),
           max(nseg, 0), max_len, cap, int(aligned16), int(bool(accumulate)), out.data_ptr(),
           N.ptr(num), _stream(stream))
    return out


def _tail_counts(counts):
    """counts of the tail-score calls: a contiguous, 16-byte aligned int32 device tensor
    [R, K, 240] (u32 counts, as the histogram calls write them); returns (R, K)."""
    N.require_device(counts, "counts")
    if (counts.dtype not in (torch.int32, torch.uint32) or counts.dim() != 3 or
            counts.shape[2] != N.HIST_BINS or not counts.is_contiguous() or counts.data_ptr() % 16):
        raise ValueError("counts must be a contiguous, 16-byte aligned int32 tensor of shape [R, K, 240]")
    return counts.shape[0], counts.shape[1]


def _tail_tensor(t, name, dtype, shape):
    N.require_device(t, name)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {list(shape)}")
    return t


def tail_permille(permille) -> int:
    """The one permille of the tail-score calls: an int in [0, 1000]; ValueError if not."""
    if isinstance(permille, bool) or not isinstance(permille, numbers.Integral) or \
            not 0 <= permille <= 1000:
        raise ValueError(f"permille must be an int in [0, 1000], got {permille!r}")
    return int(permille)


def histogram_sum(counts: torch.Tensor, out: Optional[torch.Tensor] = None,
                  accumulate: bool = False, stream=None) -> torch.Tensor:
    """The fleet histogram: the sum over the R rows of ``counts`` ([R, K, 240] int32 holding u32
    counts) as an int64 [K, 240] tensor (u64 on the device), exact.  ``out``: the tensor to write,
    or with ``accumulate=True`` to add to (then required) -- a run-long fleet.  What
    ``counts.sum(0, dtype=torch.int64)`` computes, in one pass of 16-byte loads with the rows
    split over the grid."""
    _histogram_request(out, accumulate)
    R, K = _tail_counts(counts)
    if out is None:
        out = torch.empty((K, N.HIST_BINS), dtype=torch.int64, device=counts.device)
    _tail_tensor(out, "out", torch.int64, (K, N.HIST_BINS))
    if R == 0 and not accumulate:
        out.zero_()  # the sum of no rows (the C call launches nothing)
    N.call("nvrx_histogram_sum", counts.data_ptr(), R, K, int(bool(accumulate)), out.data_ptr(),
           _stream(stream))
    return out


def histogram_tail_threshold(fleet: torch.Tensor, permille: int, col_valid=None,
                             thr: Optional[torch.Tensor] = None,
                             fleet_sums: Optional[torch.Tensor] = None, stream=None):
    """Per kernel of a fleet histogram (int64 [K, 240]) the threshold bucket of the tail scores:
    ``thr`` int32 [K], the bucket of the fleet's sample of 0-based rank ``(permille * (N - 1)) //
    1000`` (-1: no samples, or ``col_valid[k] == 0``), and ``fleet_sums`` int64 [2] = the fleet's
    weighted {tail, total} ns over the kernels taken.  Returns (thr, fleet_sums)."""
    pm = tail_permille(permille)
    N.require_device(fleet, "fleet")
    if fleet.dim() != 2:
        raise ValueError("fleet must be a contiguous int64 tensor of shape [K, 240]")
    K = fleet.shape[0]
    _tail_tensor(fleet, "fleet", torch.int64, (K, N.HIST_BINS))
    if thr is None:
        thr = torch.empty(K, dtype=torch.int32, device=fleet.device)
    if fleet_sums is None:
        fleet_sums = torch.zeros(2, dtype=torch.int64, device=fleet.device)
    _tail_tensor(thr, "thr", torch.int32, (K,))
    _tail_tensor(fleet_sums, "fleet_sums", torch.int64, (2,))
    if col_valid is not None:
        _tail_tensor(col_valid, "col_valid", col_valid.dtype, (K,))
        if col_valid.element_size() != 1:
            raise ValueError("col_valid must be a uint8 / bool tensor of shape [K]")
    N.call("nvrx_histogram_tail_threshold", fleet.data_ptr(), K, pm, N.ptr(col_valid),
           thr.data_ptr(), fleet_sums.data_ptr(), _stream(stream))
    return thr, fleet_sums


@dataclass
class TailScores:
    """Per row of ``histogram_tail_scores`` (device tensors): score [R] float64, tail_ns /
    total_ns [R] int64 (u64 on the device), strag [R] uint8 (score < score_thr), tail_calls
    [R, K] int32 (u32; None when not requested)."""

    score: torch.Tensor
    tail_ns: torch.Tensor
    total_ns: torch.Tensor
    strag: torch.Tensor
    tail_calls: Optional[torch.Tensor] = None


def histogram_tail_scores(counts: torch.Tensor, thr: torch.Tensor, fleet_sums: torch.Tensor, *,
                          score_thr: float = 0.75, thr_index: Optional[torch.Tensor] = None,
                          tail_calls=False, out: Optional[TailScores] = None,
                          stream=None) -> TailScores:
    """Tail score per row of ``counts`` ([R, K, 240]) against the threshold buckets ``thr`` and the
    fleet's ``fleet_sums`` of ``histogram_tail_threshold``: ``score = (1 - tail_ns / total_ns) /
    (1 - fleet_tail / fleet_total)`` with ``tail_ns`` the row's weighted counts above the threshold
    buckets (NaN for a row without weighted samples; never flagged).  Column k uses
    ``thr[thr_index[k]]`` when ``thr_index`` (int32 [K]) is given; a negative index skips the
    kernel.  ``tail_calls=True`` (or an int32 [R, K] tensor) also counts, per row and kernel, the
    calls above the threshold bucket.  ``out``: preallocated outputs."""
    R, K = _tail_counts(counts)
    d = counts.device
    N.require_device(thr, "thr")
    if thr.dtype != torch.int32 or thr.dim() != 1 or not thr.is_contiguous():
        raise ValueError("thr must be a contiguous int32 tensor")
    if thr_index is None:
        if thr.numel() != K:
            raise ValueError("thr must hold K entries (or pass thr_index)")
    else:
        _tail_tensor(thr_index, "thr_index", torch.int32, (K,))
    _tail_tensor(fleet_sums, "fleet_sums", torch.int64, (2,))
    if out is None:
        out = TailScores(torch.empty(R, dtype=torch.float64, device=d),
                         torch.empty(R, dtype=torch.int64, device=d),
                         torch.empty(R, dtype=torch.int64, device=d),
                         torch.empty(R, dtype=torch.uint8, device=d))
    _tail_tensor(out.score, "out.score", torch.float64, (R,))
    _tail_tensor(out.tail_ns, "out.tail_ns", torch.int64, (R,))
    _tail_tensor(out.total_ns, "out.total_ns", torch.int64, (R,))
    if out.strag is not None:
        _tail_tensor(out.strag, "out.strag", torch.uint8, (R,))
    calls = None
    if tail_calls is True:
        calls = out.tail_calls
        if calls is None:
            calls = torch.empty((R, K), dtype=torch.int32, device=d)
    elif tail_calls is not False and tail_calls is not None:
        calls = tail_calls
    if calls is not None:
        _tail_tensor(calls, "tail_calls", torch.int32, (R, K))
    a = N.TailArgs(R, K, counts.data_ptr(), thr.data_ptr(), N.ptr(thr_index), fleet_sums.data_ptr(),
                   out.tail_ns.data_ptr(), out.total_ns.data_ptr(), out.score.data_ptr(),
                   N.ptr(calls), N.ptr(out.strag), float(score_thr))
    N.call("nvrx_histogram_tail_scores", ctypes.byref(a), _stream(stream))
    return TailScores(out.score, out.tail_ns, out.total_ns, out.strag, calls)


def _segment_rows(ns, seg_off, seg_len, K):
    """The ragged triple of the segment tail calls, segment r * K + k being row r, column k;
    returns R."""
    if isinstance(K, bool) or not isinstance(K, numbers.Integral) or K < 0:
        raise ValueError(f"K must be a non-negative int, got {K!r}")
    nseg = _check_ragged(ns, seg_off, seg_len)
    if not seg_off.is_contiguous() or (seg_len is not None and not seg_len.is_contiguous()):
        raise ValueError("seg_off and seg_len must be contiguous")
    if seg_len is not None and seg_len.numel() != nseg:
        raise ValueError("seg_off and seg_len must hold one entry per segment")
    if K == 0:
        if nseg > 0:
            raise ValueError("K = 0 takes no segments")
        return 0
    if nseg < 0 or nseg % K:
        raise ValueError(f"the segments must be R * K = a multiple of {K}, got {nseg}")
    return nseg // K


def segment_fleet_histogram_ragged(ns: torch.Tensor, seg_off: torch.Tensor,
                                   seg_len: Optional[torch.Tensor], K: int, max_len: int,
                                   cap: int = 0, aligned16: bool = False,
                                   out: Optional[torch.Tensor] = None, accumulate: bool = False,
                                   stream=None) -> torch.Tensor:
    """The fleet histogram straight from the ragged segments of ``segment_histogram_ragged``
    (segment r * K + k: row r, kernel k), without the [R, K, 240] counts: int64 [K, 240] (u64 on
    the device), equal to ``histogram_sum(segment_histogram_ragged(...))`` into zeroed counts.
    ``out``: the tensor to write, or with ``accumulate=True`` to add to (then required)."""
    _histogram_request(out, accumulate)
    R = _segment_rows(ns, seg_off, seg_len, K)
    if out is None:
        out = torch.empty((K, N.HIST_BINS), dtype=torch.int64, device=ns.device)
    _tail_tensor(out, "out", torch.int64, (K, N.HIST_BINS))
    if R == 0 and not accumulate:
        out.zero_()  # the sum of no rows (the C call launches nothing)
    N.call("nvrx_segment_fleet_histogram_ragged", ns.data_ptr(), seg_off.data_ptr(), N.ptr(seg_len),
           R, K, max_len, cap, int(aligned16), int(bool(accumulate)), out.data_ptr(),
           _stream(stream))
    return out


def segment_tail_scores_ragged(ns: torch.Tensor, seg_off: torch.Tensor,
                               seg_len: Optional[torch.Tensor], K: int, max_len: int,
                               thr: torch.Tensor, fleet_sums: torch.Tensor, *, cap: int = 0,
                               aligned16: bool = False, score_thr: float = 0.75,
                               thr_index: Optional[torch.Tensor] = None, tail_calls=False,
                               out: Optional[TailScores] = None, stream=None) -> TailScores:
    """Tail score per row straight from the ragged segments (segment r * K + k: row r, kernel k),
    equal to ``histogram_tail_scores`` on the counts ``segment_histogram_ragged`` would write into
    a zeroed [R, K, 240] tensor; ``thr``, ``fleet_sums``, ``thr_index``, ``score_thr``,
    ``tail_calls`` and ``out`` as there."""
    R = _segment_rows(ns, seg_off, seg_len, K)
    d = ns.device
    N.require_device(thr, "thr")
    if thr.dtype != torch.int32 or thr.dim() != 1 or not thr.is_contiguous():
        raise ValueError("thr must be a contiguous int32 tensor")
    if thr_index is None:
        if thr.numel() != K:
            raise ValueError("thr must hold K entries (or pass thr_index)")
    else:
        _tail_tensor(thr_index, "thr_index", torch.int32, (K,))
    _tail_tensor(fleet_sums, "fleet_sums", torch.int64, (2,))
    if out is None:
        out = TailScores(torch.empty(R, dtype=torch.float64, device=d),
                         torch.empty(R, dtype=torch.int64, device=d),
                         torch.empty(R, dtype=torch.int64, device=d),
                         torch.empty(R, dtype=torch.uint8, device=d))
    _tail_tensor(out.score, "out.score", torch.float64, (R,))
    _tail_tensor(out.tail_ns, "out.tail_ns", torch.int64, (R,))
    _tail_tensor(out.total_ns, "out.total_ns", torch.int64, (R,))
    if out.strag is not None:
        _tail_tensor(out.strag, "out.strag", torch.uint8, (R,))
    calls = None
    if tail_calls is True:
        calls = out.tail_calls
        if calls is None:
            calls = torch.empty((R, K), dtype=torch.int32, device=d)
    elif tail_calls is not False and tail_calls is not None:
        calls = tail_calls
    if calls is not None:
        _tail_tensor(calls, "tail_calls", torch.int32, (R, K))
    a = N.SegTailArgs(R, K, ns.data_ptr(), seg_off.data_ptr(), N.ptr(seg_len), max_len, cap,
                      int(aligned16), thr.data_ptr(), N.ptr(thr_index), fleet_sums.data_ptr(),
                      out.tail_ns.data_ptr(), out.total_ns.data_ptr(), out.score.data_ptr(),
                      N.ptr(calls), N.ptr(out.strag), float(score_thr))
    N.call("nvrx_segment_tail_scores_ragged", ctypes.byref(a), _stream(stream))
    return TailScores(out.score, out.tail_ns, out.total_ns, out.strag, calls)


@dataclass
class HistoryTailScores:
    """Per row of ``histogram_history_scores`` (device tensors): score [R] float64, tail_ns /
    total_ns / base_tail_ns / base_total_ns [R] int64 (u64 on the device), strag [R] uint8
    (score < score_thr), tail_calls [R, K] int32 (u32; None when not requested).  Every field is
    None after an update-only call without ``out``."""

    score: Optional[torch.Tensor] = None
    tail_ns: Optional[torch.Tensor] = None
    total_ns: Optional[torch.Tensor] = None
    base_tail_ns: Optional[torch.Tensor] = None
    base_total_ns: Optional[torch.Tensor] = None
    strag: Optional[torch.Tensor] = None
    tail_calls: Optional[torch.Tensor] = None

    @classmethod
    def empty(cls, R: int, device) -> "HistoryTailScores":
        i = lambda: torch.empty(R, dtype=torch.int64, device=device)  # noqa: E731
        return cls(torch.empty(R, dtype=torch.float64, device=device), i(), i(), i(), i(),
                   torch.empty(R, dtype=torch.uint8, device=device))

    @classmethod
    def packed(cls, buf: torch.Tensor, R: int, folded: bool = False):
        """Views of the outputs at the head of one 8-byte aligned uint8 buffer, so that one copy
        moves them all: [score][tail_ns][total_ns][base_tail_ns][base_total_ns]([folded]) of 8 R
        bytes each, then strag -- 41 R bytes, 49 R with the ``folded`` counts of the compact
        entries.  Returns (outputs, the int64 [R] folded view or None); ``unpack`` reads it back."""
        n = 6 if folded else 5
        q = buf[:8 * n * R].view(torch.int64).view(n, R)
        return (cls(q[0].view(torch.float64), q[1], q[2], q[3], q[4], buf[8 * n * R:(8 * n + 1) * R]),
                q[5] if folded else None)

    @staticmethod
    def unpack(host: np.ndarray, R: int, folded: bool = False):
        """The host copy of a ``packed`` buffer as numpy arrays [R]: (score f64, tail_ns,
        total_ns, base_tail_ns, base_total_ns u64, strag bool, folded u64 or None)."""
        n = 6 if folded else 5
        q = host[:8 * n * R].view(np.uint64).reshape(n, R).copy()
        return (q[0].view(np.float64), q[1], q[2], q[3], q[4],
                host[8 * n * R:(8 * n + 1) * R].astype(bool), q[5] if folded else None)


def _u8_vector(t, name, n):
    if t is not None:
        _tail_tensor(t, name, t.dtype, (n,))
        if t.element_size() != 1:
            raise ValueError(f"{name} must be a uint8 / bool tensor of shape [{n}]")
    return t


def _history_request(fn, permille, score, update):
    """(pm, mode) of an individual-score call; ``fn`` prefixes the message."""
    pm = tail_permille(permille)
    if not (score or update):
        raise ValueError(f"{fn}: at least one of score and update")
    return pm, (N.NVRX_HTAIL_SCORE if score else 0) | (N.NVRX_HTAIL_UPDATE if update else 0)


def _history_slots(R, K, history, hist_stride, hist_index, col_valid, skip_rows=None, *, compact):
    """Checks the history of R rows x K columns -- dense ``hist`` or compact ``chist`` -- and what
    addresses it; returns the stride."""
    stride = int(hist_stride)
    if stride < 0 or (stride and hist_index is None and stride < K):
        raise ValueError("hist_stride must be 0 (= K) or, without hist_index, at least K")
    if compact:
        N.require_device(history, "chist")
        if history.dtype != torch.uint8 or history.data_ptr() % 16:
            raise ValueError("chist must be a contiguous, 16-byte aligned uint8 tensor")
        _tail_tensor(history, "chist", torch.uint8, (R, stride or K, N.CHIST_BYTES))
    else:
        N.require_device(history, "hist")
        if history.dtype not in (torch.int32, torch.uint32) or history.data_ptr() % 16:
            raise ValueError("hist must be a contiguous, 16-byte aligned int32 tensor")
        _tail_tensor(history, "hist", history.dtype, (R, stride or K, N.HIST_BINS))
    if hist_index is not None:
        _tail_tensor(hist_index, "hist_index", torch.int32, (K,))
    _u8_vector(col_valid, "col_valid", K)
    _u8_vector(skip_rows, "skip_rows", R)
    return stride


def _history_outputs(R, K, d, score, out, tail_calls):
    """(out, calls): the checked (or new) outputs of an individual score and its tail_calls."""
    calls = None
    if score:
        if out is None:
            out = HistoryTailScores.empty(R, d)
        _tail_tensor(out.score, "out.score", torch.float64, (R,))
        for n in ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns"):
            _tail_tensor(getattr(out, n), "out." + n, torch.int64, (R,))
        if out.strag is not None:
            _tail_tensor(out.strag, "out.strag", torch.uint8, (R,))
        if tail_calls is True:
            calls = out.tail_calls
            if calls is None:
                calls = torch.empty((R, K), dtype=torch.int32, device=d)
        elif tail_calls is not False and tail_calls is not None:
            calls = tail_calls
        if calls is not None:
            _tail_tensor(calls, "tail_calls", torch.int32, (R, K))
    elif out is None:
        out = HistoryTailScores()
    return out, calls


def _folded(R, d, update, folded):
    if not update:
        return None
    if folded is None:
        folded = torch.empty(R, dtype=torch.int64, device=d)
    _tail_tensor(folded, "folded", torch.int64, (R,))
    return folded


def histogram_history_scores(counts: torch.Tensor, hist: torch.Tensor, *, permille: int,
                             score: bool = True, update: bool = True,
                             hist_index: Optional[torch.Tensor] = None, hist_stride: int = 0,
                             col_valid: Optional[torch.Tensor] = None,
                             skip_rows: Optional[torch.Tensor] = None, score_thr: float = 0.75,
                             tail_calls=False, out: Optional[HistoryTailScores] = None,
                             stream=None) -> HistoryTailScores:
    """Individual tail score per row of ``counts`` ([R, K, 240]) against the row's own history
    ``hist`` (int32 [R, hist_stride or K, 240] holding u32 counts, changed in place), in one fused
    pass: per (row, kernel) the threshold bucket T is the bucket of the history's sample of rank
    ``(permille * (N - 1)) // 1000``, and

        score = (1 - tail_ns / total_ns) / (1 - base_tail_ns / base_total_ns)

    with ``tail_ns`` / ``base_tail_ns`` the current / historic weighted counts above T, over the
    kernels with a history slot, ``col_valid``, history and current samples (NaN without any: a
    first interval is never flagged).  ``update`` then folds the counts into the history,
    ``min(H + C, 2**32 - 1)``, except in the rows ``skip_rows`` (uint8 [R]) marks; with both, the
    score is taken against the history from before the update.  Column k uses slot
    ``hist_index[k]`` (int32 [K]; negative: no slot, the kernel is left out).  Two columns must not
    share a slot and ``counts`` must not overlap ``hist`` (neither is checked).
    ``tail_calls=True`` (or an int32 [R, K] tensor) also counts the calls above T per row and
    kernel.  ``score=False`` touches no score output.  ``out``: preallocated outputs."""
    pm, mode = _history_request("histogram_history_scores", permille, score, update)
    R, K = _tail_counts(counts)
    d = counts.device
    stride = _history_slots(R, K, hist, hist_stride, hist_index, col_valid, skip_rows, compact=False)
    out, calls = _history_outputs(R, K, d, score, out, tail_calls)
    a = N.HistTailArgs(R, K, counts.data_ptr(), hist.data_ptr(), stride, N.ptr(hist_index),
                       N.ptr(col_valid), N.ptr(skip_rows), pm, mode, float(score_thr),
                       N.ptr(out.tail_ns), N.ptr(out.total_ns), N.ptr(out.base_tail_ns),
                       N.ptr(out.base_total_ns), N.ptr(out.score), N.ptr(out.strag), N.ptr(calls))
    N.call("nvrx_histogram_history_scores", ctypes.byref(a), _stream(stream))
    return HistoryTailScores(out.score, out.tail_ns, out.total_ns, out.base_tail_ns,
                             out.base_total_ns, out.strag, calls)


def segment_history_scores_ragged(ns: torch.Tensor, seg_off: torch.Tensor,
                                  seg_len: Optional[torch.Tensor], K: int, max_len: int,
                                  hist: torch.Tensor, *, permille: int, score: bool = True,
                                  update: bool = True, cap: int = 0, aligned16: bool = False,
                                  hist_index: Optional[torch.Tensor] = None, hist_stride: int = 0,
                                  col_valid: Optional[torch.Tensor] = None,
                                  skip_rows: Optional[torch.Tensor] = None, score_thr: float = 0.75,
                                  tail_calls=False, out: Optional[HistoryTailScores] = None,
                                  stream=None) -> HistoryTailScores:
    """Individual tail score per row straight from the ragged segments (segment r * K + k: row r,
    kernel k; the last ``cap`` samples retained, a length <= 0 an empty element) against the row's
    own history ``hist``: what ``histogram_history_scores`` gives, and does to ``hist``, on the
    counts ``segment_histogram_ragged`` would write into a zeroed [R, K, 240] tensor -- without
    that tensor.  An element without retained samples is not scored and leaves its history slot as
    it is.  ``hist`` keeps its format, so one history can be continued by either function; every
    other argument and ``out`` as in ``histogram_history_scores``."""
    pm, mode = _history_request("segment_history_scores_ragged", permille, score, update)
    R = _segment_rows(ns, seg_off, seg_len, K)
    d = ns.device
    stride = _history_slots(R, K, hist, hist_stride, hist_index, col_valid, skip_rows, compact=False)
    out, calls = _history_outputs(R, K, d, score, out, tail_calls)
    a = N.SegHistArgs(R, K, ns.data_ptr(), seg_off.data_ptr(), N.ptr(seg_len), max_len, cap,
                      int(aligned16), hist.data_ptr(), stride, N.ptr(hist_index), N.ptr(col_valid),
                      N.ptr(skip_rows), pm, mode, float(score_thr), N.ptr(out.tail_ns),
                      N.ptr(out.total_ns), N.ptr(out.base_tail_ns), N.ptr(out.base_total_ns),
                      N.ptr(out.score), N.ptr(out.strag), N.ptr(calls))
    N.call("nvrx_segment_history_scores_ragged", ctypes.byref(a), _stream(stream))
    return HistoryTailScores(out.score, out.tail_ns, out.total_ns, out.base_tail_ns,
                             out.base_total_ns, out.strag, calls)


def segment_history_scores_compact_ragged(ns: torch.Tensor, seg_off: torch.Tensor,
                                          seg_len: Optional[torch.Tensor], K: int, max_len: int,
                                          chist: torch.Tensor, *, permille: int, score: bool = True,
                                          update: bool = True, cap: int = 0, aligned16: bool = False,
                                          hist_index: Optional[torch.Tensor] = None,
                                          hist_stride: int = 0,
                                          col_valid: Optional[torch.Tensor] = None,
                                          skip_rows: Optional[torch.Tensor] = None,
                                          score_thr: float = 0.75, tail_calls=False,
                                          out: Optional[HistoryTailScores] = None,
                                          folded: Optional[torch.Tensor] = None, stream=None):
    """``segment_history_scores_ragged`` against a compact history ``chist`` (uint8
    [R, hist_stride or K, 64], changed in place): 64 bytes per (row, kernel) -- u32 count[12], u8
    bucket[12], u32 n, the used buckets ascending -- in place of 960.  The score is the dense
    entry's against the element's dense expansion; ``update`` admits an interval's new buckets in
    ascending order while the element has free entries and folds every other sample into the
    nearest kept bucket at or below it.  Returns ``(HistoryTailScores, folded)``: ``folded`` (int64
    [R], u64 on the device; None without ``update``) counts the folded samples per row -- while it
    stays 0 the history expands (``histograms.compact_to_dense``) to exactly the dense entry's and
    every output equals that entry's bit for bit.  A zeroed ``chist`` is the empty history.  Every
    other argument and ``out`` as in ``segment_history_scores_ragged``."""
    pm, mode = _history_request("segment_history_scores_compact_ragged", permille, score, update)
    R = _segment_rows(ns, seg_off, seg_len, K)
    d = ns.device
    stride = _history_slots(R, K, chist, hist_stride, hist_index, col_valid, skip_rows, compact=True)
    out, calls = _history_outputs(R, K, d, score, out, tail_calls)
    folded = _folded(R, d, update, folded)
    a = N.SegCHistArgs(R, K, ns.data_ptr(), seg_off.data_ptr(), N.ptr(seg_len), max_len, cap,
                       int(aligned16), chist.data_ptr(), stride, N.ptr(hist_index),
                       N.ptr(col_valid), N.ptr(skip_rows), pm, mode, float(score_thr),
                       N.ptr(out.tail_ns), N.ptr(out.total_ns), N.ptr(out.base_tail_ns),
                       N.ptr(out.base_total_ns), N.ptr(out.score), N.ptr(out.strag), N.ptr(calls),
                       N.ptr(folded))
    N.call("nvrx_segment_history_scores_compact_ragged", ctypes.byref(a), _stream(stream))
    return HistoryTailScores(out.score, out.tail_ns, out.total_ns, out.base_tail_ns,
                             out.base_total_ns, out.strag, calls), folded


def histogram_history_scores_compact(counts: torch.Tensor, chist: torch.Tensor, *, permille: int,
                                     score: bool = True, update: bool = True,
                                     hist_index: Optional[torch.Tensor] = None, hist_stride: int = 0,
                                     col_valid: Optional[torch.Tensor] = None,
                                     skip_rows: Optional[torch.Tensor] = None,
                                     score_thr: float = 0.75, tail_calls=False,
                                     out: Optional[HistoryTailScores] = None,
                                     folded: Optional[torch.Tensor] = None, stream=None):
    """``histogram_history_scores`` against a compact history ``chist`` (uint8
    [R, hist_stride or K, 64], changed in place; the format of
    ``segment_history_scores_compact_ragged``, so one history can be continued by either): the
    score of ``counts`` ([R, K, 240]) is the dense entry's against every element's dense
    expansion; ``update`` admits the interval's new buckets in ascending order while the element
    has free entries and folds every other count into the nearest kept bucket at or below it, the
    sums taken in 64 bits and saturating.  An element whose counts are all zero is neither scored
    nor written.  Returns ``(HistoryTailScores, folded)``: ``folded`` (int64 [R], u64 on the
    device; None without ``update``) counts the folded samples per row -- while it stays 0 the
    history expands (``compact_history_to_dense``) to exactly the dense entry's and every output
    equals that entry's bit for bit.  ``counts`` must not overlap ``chist``.  Every other argument
    and ``out`` as in ``histogram_history_scores``; ``histograms.compact_history_scores`` is the
    host twin."""
    pm, mode = _history_request("histogram_history_scores_compact", permille, score, update)
    R, K = _tail_counts(counts)
    d = counts.device
    stride = _history_slots(R, K, chist, hist_stride, hist_index, col_valid, skip_rows, compact=True)
    out, calls = _history_outputs(R, K, d, score, out, tail_calls)
    folded = _folded(R, d, update, folded)
    a = N.HistCHistArgs(R, K, counts.data_ptr(), chist.data_ptr(), stride, N.ptr(hist_index),
                        N.ptr(col_valid), N.ptr(skip_rows), pm, mode, float(score_thr),
                        N.ptr(out.tail_ns), N.ptr(out.total_ns), N.ptr(out.base_tail_ns),
                        N.ptr(out.base_total_ns), N.ptr(out.score), N.ptr(out.strag), N.ptr(calls),
                        N.ptr(folded))
    N.call("nvrx_histogram_history_scores_compact", ctypes.byref(a), _stream(stream))
    return HistoryTailScores(out.score, out.tail_ns, out.total_ns, out.base_tail_ns,
                             out.base_total_ns, out.strag, calls), folded


def _dense_history(hist, name="hist"):
    N.require_device(hist, name)
    if (hist.dtype not in (torch.int32, torch.uint32) or hist.dim() != 3 or
            hist.shape[2] != N.HIST_BINS or not hist.is_contiguous() or hist.data_ptr() % 16):
        raise ValueError(f"{name} must be a contiguous, 16-byte aligned int32 tensor of shape [R, S, 240]")
    return hist.shape[0], hist.shape[1]


def _compact_history(chist, name="chist"):
    N.require_device(chist, name)
    if (chist.dtype != torch.uint8 or chist.dim() != 3 or chist.shape[2] != N.CHIST_BYTES or
            not chist.is_contiguous() or chist.data_ptr() % 16):
        raise ValueError(f"{name} must be a contiguous, 16-byte aligned uint8 tensor of shape [R, S, 64]")
    return chist.shape[0], chist.shape[1]


def compact_history_from_dense(hist: torch.Tensor, out: Optional[torch.Tensor] = None,
                               folded=None, stream=None):
    """The compact history (uint8 [R, S, 64], ``out`` or a new tensor) of a dense one ``hist``
    (int32 [R, S, 240] holding u32 counts, unchanged): per element the 12 lowest used buckets, the
    counts above them folded into the 12th (64-bit sums, saturating) -- the ``update`` of an empty
    element with those counts, ``histograms.compact_from_dense`` on the host.  Every element of
    ``out`` is written in full, so it needs no clear; the two tensors must not overlap (not
    checked).  Returns ``(out, folded)``: ``folded`` (int64 [R], u64 on the device, cleared on the
    stream first; a tensor given is used) counts the folded samples per row; ``folded=False``
    passes NULL and returns None for it."""
    R, S = _dense_history(hist)
    if out is None:
        out = torch.empty((R, S, N.CHIST_BYTES), dtype=torch.uint8, device=hist.device)
    if _compact_history(out, "out") != (R, S):
        raise ValueError(f"out must have shape [{R}, {S}, 64]")
    if folded is False:
        folded = None
    else:
        if folded is None:
            folded = torch.empty(R, dtype=torch.int64, device=hist.device)
        _tail_tensor(folded, "folded", torch.int64, (R,))
    N.call("nvrx_compact_history_from_dense", hist.data_ptr(), out.data_ptr(), R, S, N.ptr(folded),
           _stream(stream))
    return out, folded


def compact_history_to_dense(chist: torch.Tensor, out: Optional[torch.Tensor] = None,
                             stream=None) -> torch.Tensor:
    """The dense expansion (int32 [R, S, 240] holding u32 counts, ``out`` or a new tensor) of a
    canonical compact history ``chist`` (uint8 [R, S, 64], unchanged): ``H[bucket[i]] = count[i]``
    for the used entries, zero elsewhere (``histograms.compact_to_dense`` on the host).  All 240
    bins of every element are written, so ``out`` needs no clear; the two tensors must not overlap
    (not checked)."""
    R, S = _compact_history(chist)
    if out is None:
        out = torch.empty((R, S, N.HIST_BINS), dtype=torch.int32, device=chist.device)
    if _dense_history(out, "out") != (R, S):
        raise ValueError(f"out must have shape [{R}, {S}, 240]")
    N.call("nvrx_compact_history_to_dense", chist.data_ptr(), out.data_ptr(), R, S, _stream(stream))
    return out


def age_shift(shift) -> int:
    """The shift of the aging calls: an int in [1, 31]; ValueError if not."""
    if isinstance(shift, bool) or not isinstance(shift, numbers.Integral) or not 1 <= shift <= 31:
        raise ValueError(f"shift must be an int in [1, 31], got {shift!r}")
    return int(shift)


def compact_history_age(chist: torch.Tensor, shift: int = 1, evicted: Optional[torch.Tensor] = None,
                        full: Optional[torch.Tensor] = None, counts: bool = True, stream=None):
    """Age a compact history ``chist`` (uint8 [R, S, 64], changed in place): every count of every
    slot becomes ``count >> shift`` (halved for ``shift`` = 1), the entries that reach zero are
    evicted, and the element is re-packed to canonical form -- the kept entries in their order at
    the front, everything behind them zero -- so that the freed entries can admit new buckets.  An
    element that loses every entry is the empty history again; an empty element is not written.
    Returns ``(evicted, full)``, int64 [R] device tensors (u64 on the device, cleared first, or the
    tensors given): the entries freed per row and the elements per row that still hold 12 entries
    afterwards.  ``counts=False`` passes NULL for both and returns ``(None, None)``.  The dense
    expansion of the result is ``histogram_history_age`` of the expansion
    (``histograms.compact_age`` on the host)."""
    s = age_shift(shift)
    R, S = _compact_history(chist)
    if counts:
        if evicted is None:
            evicted = torch.empty(R, dtype=torch.int64, device=chist.device)
        if full is None:
            full = torch.empty(R, dtype=torch.int64, device=chist.device)
        _tail_tensor(evicted, "evicted", torch.int64, (R,))
        _tail_tensor(full, "full", torch.int64, (R,))
    elif evicted is not None or full is not None:
        raise ValueError("compact_history_age: evicted / full given with counts=False")
    N.call("nvrx_compact_history_age", chist.data_ptr(), R, S, s, N.ptr(evicted), N.ptr(full),
           _stream(stream))
    return evicted, full


def histogram_history_age(hist: torch.Tensor, shift: int = 1, stream=None) -> torch.Tensor:
    """Age a dense history ``hist`` (int32 [R, S, 240] holding u32 counts, changed in place and
    returned): every word becomes ``word >> shift`` (``histograms.history_age`` on the host)."""
    s = age_shift(shift)
    R, S = _dense_history(hist)
    N.call("nvrx_histogram_history_age", hist.data_ptr(), R, S, s, _stream(stream))
    return hist


def histogram_tail_base(fleet: torch.Tensor, thr: torch.Tensor, out: Optional[torch.Tensor] = None,
                        stream=None) -> torch.Tensor:
    """Per kernel of a fleet histogram (int64 [K, 240]) its weighted {tail, total} ns over the
    threshold bucket ``thr[k]`` (int32 [K], from ``histogram_tail_threshold``) as int64 [K, 2] (u64
    on the device; {0, 0} where ``thr[k] < 0``): the base of the relative tail attribution, the
    per-kernel terms ``histogram_tail_threshold`` adds up into ``fleet_sums``."""
    N.require_device(fleet, "fleet")
    if fleet.dim() != 2:
        raise ValueError("fleet must be a contiguous int64 tensor of shape [K, 240]")
    K = fleet.shape[0]
    _tail_tensor(fleet, "fleet", torch.int64, (K, N.HIST_BINS))
    _tail_tensor(thr, "thr", torch.int32, (K,))
    if out is None:
        out = torch.empty((K, 2), dtype=torch.int64, device=fleet.device)
    _tail_tensor(out, "out", torch.int64, (K, 2))
    if out.data_ptr() % 16:
        raise ValueError("out must be 16-byte aligned")
    N.call("nvrx_histogram_tail_base", fleet.data_ptr(), K, thr.data_ptr(), out.data_ptr(),
           _stream(stream))
    return out


@dataclass
class TailAttribution:
    """Per row of ``histogram_tail_attribution`` (device tensors), the ``top`` kernels with the
    largest excess tail time, largest first: idx [R, top] int32 column (-1: fewer kernels taken),
    loss [R, top] float64 ns (NaN where idx is -1), tail_ns / total_ns [R, top] int64 (u64 on the
    device), tail_calls [R, top] int32 (u32), thr_bucket [R, top] int32, base_share [R, top]
    float64, and the dense loss_all [R, K] float64 (NaN where the kernel is not taken)."""

    idx: torch.Tensor
    loss: torch.Tensor
    tail_ns: torch.Tensor
    total_ns: torch.Tensor
    tail_calls: torch.Tensor
    thr_bucket: torch.Tensor
    base_share: torch.Tensor
    loss_all: torch.Tensor

    # bytes of one (row, j) slot of the packed form: loss, tail_ns, total_ns, base_share (8 each),
    # idx, tail_calls, thr_bucket (4 each)
    PACKED = 44

    @classmethod
    def empty(cls, R: int, K: int, top: int, device) -> "TailAttribution":
        return cls.packed(torch.empty(cls.PACKED * R * top, dtype=torch.uint8, device=device), R, top,
                          torch.empty((R, K), dtype=torch.float64, device=device))

    @classmethod
    def packed(cls, buf: torch.Tensor, R: int, top: int, loss_all: torch.Tensor) -> "TailAttribution":
        """Views of the [R, top] outputs in one 8-byte aligned uint8 buffer of PACKED * R * top
        bytes (8-byte fields first), so that one copy moves them all; ``unpack`` reads it back."""
        n = R * top
        q = buf[:32 * n].view(torch.int64).view(4, R, top)
        d = buf[32 * n:44 * n].view(torch.int32).view(3, R, top)
        return cls(d[0], q[0].view(torch.float64), q[1], q[2], d[1], d[2], q[3].view(torch.float64),
                   loss_all)

    @staticmethod
    def unpack(host: np.ndarray, R: int, top: int):
        """The host copy of a ``packed`` buffer as numpy arrays [R, top]: (idx i32, loss f64,
        tail_ns u64, total_ns u64, tail_calls u32, thr_bucket i32, base_share f64)."""
        n = R * top
        q = host[:32 * n].view(np.uint64).reshape(4, R, top).copy()
        d = host[32 * n:44 * n].view(np.int32).reshape(3, R, top).copy()
        return (d[0], q[0].view(np.float64), q[1], q[2], d[1].view(np.uint32), d[2],
                q[3].view(np.float64))


def _attribution_outputs(R, K, top, d, out):
    """The checked (or new) outputs of a tail attribution."""
    if out is None:
        out = TailAttribution.empty(R, K, top, d)
    for name, dt in (("idx", torch.int32), ("loss", torch.float64), ("tail_ns", torch.int64),
                     ("total_ns", torch.int64), ("tail_calls", torch.int32),
                     ("thr_bucket", torch.int32), ("base_share", torch.float64)):
        _tail_tensor(getattr(out, name), "out." + name, dt, (R, top))
    _tail_tensor(out.loss_all, "out.loss_all", torch.float64, (R, K))
    return out


def _relative_base(thr, base, thr_index, K):
    """Checks the fleet base of a relative attribution: thr, base [., 2] and the optional index."""
    N.require_device(thr, "thr")
    if thr.dtype != torch.int32 or thr.dim() != 1 or not thr.is_contiguous():
        raise ValueError("thr must be a contiguous int32 tensor")
    _tail_tensor(base, "base", torch.int64, (thr.numel(), 2))
    if thr_index is None:
        if thr.numel() != K:
            raise ValueError("thr must hold K entries (or pass thr_index)")
    else:
        _tail_tensor(thr_index, "thr_index", torch.int32, (K,))


def histogram_tail_attribution(counts: torch.Tensor, *, top: int, kind: str,
                               thr: Optional[torch.Tensor] = None,
                               thr_index: Optional[torch.Tensor] = None,
                               base: Optional[torch.Tensor] = None,
                               hist: Optional[torch.Tensor] = None,
                               hist_index: Optional[torch.Tensor] = None, hist_stride: int = 0,
                               col_valid: Optional[torch.Tensor] = None,
                               permille: Optional[int] = None,
                               out: Optional[TailAttribution] = None,
                               stream=None) -> TailAttribution:
    """The kernels behind a tail score: per row of ``counts`` ([R, K, 240]) the ``top`` (1..16)
    kernels with the largest excess tail time ``loss = tail - total * (btail / btotal)`` in ns,
    where ``tail`` / ``total`` are the (row, kernel)'s weighted counts above its threshold bucket T
    / in all buckets and ``btail`` / ``btotal`` the base's (include/nvrx_straggler.h).
    kind="relative": the base is the fleet -- ``thr`` (int32, ``histogram_tail_threshold``) and
    ``base`` (int64 [., 2], ``histogram_tail_base``), column k using entry ``thr_index[k]`` (int32
    [K]; negative: left out).  kind="individual": the base is the row's own history ``hist`` (int32
    [R, hist_stride or K, 240], read only) with T at ``permille`` of the history, over the elements
    ``histogram_history_scores`` scores (``hist_index``, ``col_valid``).  Two launches, no scratch;
    ``out``: preallocated outputs (``out.loss_all`` is also the workspace)."""
    top, kind_code = attribution_request(top, kind)
    R, K = _tail_counts(counts)
    d = counts.device
    stride, pm = 0, 0
    if kind_code == N.NVRX_ATTR_RELATIVE:
        if thr is None or base is None:
            raise ValueError("kind='relative' needs thr and base")
        _relative_base(thr, base, thr_index, K)
        hist = hist_index = col_valid = None
    else:
        if hist is None or permille is None:
            raise ValueError("kind='individual' needs hist and permille")
        pm = tail_permille(permille)
        stride = _history_slots(R, K, hist, hist_stride, hist_index, col_valid, compact=False)
        thr = thr_index = base = None
    out = _attribution_outputs(R, K, top, d, out)
    a = N.TailAttrArgs(R, K, counts.data_ptr(), kind_code, top, N.ptr(thr), N.ptr(thr_index),
                       N.ptr(base), N.ptr(hist), stride, N.ptr(hist_index), N.ptr(col_valid), pm,
                       out.idx.data_ptr(), out.loss.data_ptr(), out.tail_ns.data_ptr(),
                       out.total_ns.data_ptr(), out.tail_calls.data_ptr(),
                       out.thr_bucket.data_ptr(), out.base_share.data_ptr(),
                       out.loss_all.data_ptr())
    N.call("nvrx_histogram_tail_attribution", ctypes.byref(a), _stream(stream))
    return out


def segment_tail_attribution_ragged(ns: torch.Tensor, seg_off: torch.Tensor,
                                    seg_len: Optional[torch.Tensor], K: int, max_len: int,
                                    thr: torch.Tensor, base: torch.Tensor, *, top: int,
                                    cap: int = 0, aligned16: bool = False,
                                    thr_index: Optional[torch.Tensor] = None,
                                    out: Optional[TailAttribution] = None,
                                    stream=None) -> TailAttribution:
    """The kernels behind a tail score straight from the ragged segments (segment r * K + k: row
    r, kernel k), equal to ``histogram_tail_attribution(kind="relative")`` on the counts
    ``segment_histogram_ragged`` would write into a zeroed [R, K, 240] tensor: ``thr`` (int32,
    ``histogram_tail_threshold`` on the fleet of ``segment_fleet_histogram_ragged``), ``base``
    (int64 [., 2], ``histogram_tail_base``), ``thr_index``, ``top`` and ``out`` as there.  Two
    launches, no scratch; ``out.loss_all`` is also the workspace."""
    top, _ = attribution_request(top, "relative")
    R = _segment_rows(ns, seg_off, seg_len, K)
    d = ns.device
    _relative_base(thr, base, thr_index, K)
    out = _attribution_outputs(R, K, top, d, out)
    a = N.SegTailAttrArgs(R, K, ns.data_ptr(), seg_off.data_ptr(), N.ptr(seg_len), max_len, cap,
                          int(aligned16), top, thr.data_ptr(), N.ptr(thr_index), base.data_ptr(),
                          out.idx.data_ptr(), out.loss.data_ptr(), out.tail_ns.data_ptr(),
                          out.total_ns.data_ptr(), out.tail_calls.data_ptr(),
                          out.thr_bucket.data_ptr(), out.base_share.data_ptr(),
                          out.loss_all.data_ptr())
    N.call("nvrx_segment_tail_attribution_ragged", ctypes.byref(a), _stream(stream))
    return out


def segment_history_attribution_ragged(ns: torch.Tensor, seg_off: torch.Tensor,
                                       seg_len: Optional[torch.Tensor], K: int, max_len: int,
                                       hist: torch.Tensor, *, permille: int, top: int,
                                       cap: int = 0, aligned16: bool = False,
                                       hist_index: Optional[torch.Tensor] = None,
                                       hist_stride: int = 0,
                                       col_valid: Optional[torch.Tensor] = None,
                                       out: Optional[TailAttribution] = None,
                                       stream=None) -> TailAttribution:
    """The kernels behind an individual tail score straight from the ragged segments (segment
    r * K + k: row r, kernel k; the last ``cap`` samples retained, a length <= 0 an empty
    element), equal to ``histogram_tail_attribution(kind="individual")`` on the counts
    ``segment_histogram_ragged`` would write into a zeroed [R, K, 240] tensor -- without that
    tensor.  ``hist`` (read only), ``hist_index``, ``hist_stride``, ``col_valid`` and ``permille``
    as in ``segment_history_scores_ragged``: between its score and its update call this sees the
    history the score saw.  ``top`` and ``out`` as in ``histogram_tail_attribution``.  Two
    launches, no scratch; ``out.loss_all`` is also the workspace."""
    top, _ = attribution_request(top, "individual")
    pm = tail_permille(permille)
    R = _segment_rows(ns, seg_off, seg_len, K)
    d = ns.device
    stride = _history_slots(R, K, hist, hist_stride, hist_index, col_valid, compact=False)
    out = _attribution_outputs(R, K, top, d, out)
    a = N.SegHistAttrArgs(R, K, ns.data_ptr(), seg_off.data_ptr(), N.ptr(seg_len), max_len, cap,
                          int(aligned16), top, hist.data_ptr(), stride, N.ptr(hist_index),
                          N.ptr(col_valid), pm, out.idx.data_ptr(), out.loss.data_ptr(),
                          out.tail_ns.data_ptr(), out.total_ns.data_ptr(),
                          out.tail_calls.data_ptr(), out.thr_bucket.data_ptr(),
                          out.base_share.data_ptr(), out.loss_all.data_ptr())
    N.call("nvrx_segment_history_attribution_ragged", ctypes.byref(a), _stream(stream))
    return out


def segment_history_attribution_compact_ragged(ns: torch.Tensor, seg_off: torch.Tensor,
                                               seg_len: Optional[torch.Tensor], K: int,
                                               max_len: int, chist: torch.Tensor, *, permille: int,
                                               top: int, cap: int = 0, aligned16: bool = False,
                                               hist_index: Optional[torch.Tensor] = None,
                                               hist_stride: int = 0,
                                               col_valid: Optional[torch.Tensor] = None,
                                               out: Optional[TailAttribution] = None,
                                               stream=None) -> TailAttribution:
    """``segment_history_attribution_ragged`` against a compact history ``chist`` (uint8
    [R, hist_stride or K, 64], read only; the layout of ``segment_history_scores_compact_ragged``):
    every output equals, bit for bit, that entry's on the dense expansion of ``chist``
    (``histograms.compact_to_dense``) -- without the 960 bytes per element.  Between the score and
    the update call of ``segment_history_scores_compact_ragged`` this sees the history the score
    saw.  Every other argument and ``out`` as in ``segment_history_attribution_ragged``.  Two
    launches, no scratch; ``out.loss_all`` is also the workspace."""
    top, _ = attribution_request(top, "individual")
    pm = tail_permille(permille)
    R = _segment_rows(ns, seg_off, seg_len, K)
    d = ns.device
    stride = _history_slots(R, K, chist, hist_stride, hist_index, col_valid, compact=True)
    out = _attribution_outputs(R, K, top, d, out)
    a = N.SegCHistAttrArgs(R, K, ns.data_ptr(), seg_off.data_ptr(), N.ptr(seg_len), max_len, cap,
                           int(aligned16), top, chist.data_ptr(), stride, N.ptr(hist_index),
                           N.ptr(col_valid), pm, out.idx.data_ptr(), out.loss.data_ptr(),
                           out.tail_ns.data_ptr(), out.total_ns.data_ptr(),
                           out.tail_calls.data_ptr(), out.thr_bucket.data_ptr(),
                           out.base_share.data_ptr(), out.loss_all.data_ptr())
    N.call("nvrx_segment_history_attribution_compact_ragged", ctypes.byref(a), _stream(stream))
    return out


def histogram_history_attribution_compact(counts: torch.Tensor, chist: torch.Tensor, *,
                                          permille: int, top: int,
                                          hist_index: Optional[torch.Tensor] = None,
                                          hist_stride: int = 0,
                                          col_valid: Optional[torch.Tensor] = None,
                                          out: Optional[TailAttribution] = None,
                                          stream=None) -> TailAttribution:
    """``histogram_tail_attribution(kind="individual")`` against a compact history ``chist``
    (uint8 [R, hist_stride or K, 64], read only; the layout of
    ``histogram_history_scores_compact``): every output equals, bit for bit, that entry's on the
    dense expansion of ``chist`` (``histograms.compact_to_dense``) -- without the 960 bytes per
    element (``histograms.compact_history_attribution`` on the host).  Between the score and the
    update call of ``histogram_history_scores_compact`` this sees the history the score saw.
    ``counts``, ``hist_index``, ``hist_stride``, ``col_valid``, ``permille``, ``top`` and ``out``
    as in ``histogram_tail_attribution``.  Two launches, no scratch; ``out.loss_all`` is also the
    workspace."""
    top, _ = attribution_request(top, "individual")
    pm = tail_permille(permille)
    R, K = _tail_counts(counts)
    N.require_device(chist, "chist")
    if chist.dtype != torch.uint8 or chist.dim() != 3 or chist.shape[2] != N.CHIST_BYTES:
        raise ValueError("chist must be a contiguous, 16-byte aligned uint8 tensor of shape "
                         "[R, S, 64] (a dense history goes to histogram_tail_attribution)")
    stride = _history_slots(R, K, chist, hist_stride, hist_index, col_valid, compact=True)
    out = _attribution_outputs(R, K, top, counts.device, out)
    a = N.HistCHistAttrArgs(R, K, counts.data_ptr(), top, chist.data_ptr(), stride,
                            N.ptr(hist_index), N.ptr(col_valid), pm, out.idx.data_ptr(),
                            out.loss.data_ptr(), out.tail_ns.data_ptr(), out.total_ns.data_ptr(),
                            out.tail_calls.data_ptr(), out.thr_bucket.data_ptr(),
                            out.base_share.data_ptr(), out.loss_all.data_ptr())
    N.call("nvrx_histogram_history_attribution_compact", ctypes.byref(a), _stream(stream))
    return out


@dataclass
class RankAttribution:
    """Per column (kernel) of ``rank_attribution`` (device tensors), the ``top`` rows (ranks) with
    the largest loss, largest first: idx [K, top] int32 row (-1: fewer rows taken), loss [K, top]
    float64 with the input's bits (NaN where idx is -1), taken [K] int32 rows taken, positive [K]
    int32 taken rows whose loss is > 0."""

    idx: torch.Tensor
    loss: torch.Tensor
    taken: torch.Tensor
    positive: torch.Tensor

    @staticmethod
    def nbytes(K: int, top: int) -> int:
        """Bytes of the packed form: loss (8), idx (4) per (column, j); taken, positive (4 each)."""
        return 12 * K * top + 8 * K

    @classmethod
    def empty(cls, K: int, top: int, device) -> "RankAttribution":
        return cls.packed(torch.empty(cls.nbytes(K, top), dtype=torch.uint8, device=device), K, top)

    @classmethod
    def packed(cls, buf: torch.Tensor, K: int, top: int) -> "RankAttribution":
        """Views of the outputs in one 8-byte aligned uint8 buffer of ``nbytes(K, top)`` bytes (the
        f64 field first), so that one copy moves them all; ``unpack`` reads it back."""
        n = K * top
        d = buf[8 * n:12 * n + 8 * K].view(torch.int32)
        return cls(d[:n].view(K, top), buf[:8 * n].view(torch.float64).view(K, top),
                   d[n:n + K], d[n + K:n + 2 * K])

    @staticmethod
    def unpack(host: np.ndarray, K: int, top: int):
        """The host copy of a ``packed`` buffer as numpy arrays: (idx [K, top] i32, loss [K, top]
        f64, taken [K] i32, positive [K] i32)."""
        n = K * top
        d = host[8 * n:12 * n + 8 * K].view(np.int32).copy()
        return (d[:n].reshape(K, top), host[:8 * n].view(np.float64).reshape(K, top).copy(),
                d[n:n + K], d[n + K:n + 2 * K])


def rank_attribution_plan(R: int, K: int, top: int):
    """(tiles, splits, work_bytes) of ``rank_attribution`` on an [R, K] matrix: workgroups along K
    (64 columns each) and along R, and the bytes of ``work`` it needs (0 with one split, where one
    kernel writes the outputs; more splits add a merge kernel).  Pure host code."""
    t, s, w = N.i64(), N.i64(), N.i64()
    N.call("nvrx_rank_attribution_plan", R, K, top, ctypes.byref(t), ctypes.byref(s), ctypes.byref(w))
    return t.value, s.value, w.value


def _rank_loss(loss):
    """loss of ``rank_attribution``: a float64 device tensor [R, K] whose rows are contiguous and a
    whole number of elements apart (a row stride above K is allowed); returns (R, K, ld)."""
    N.require_device(loss, "loss")
    if loss.dtype != torch.float64 or loss.dim() != 2:
        raise ValueError("loss must be a float64 device tensor of shape [R, K]")
    R, K = loss.shape
    ld = K
    if R > 0 and K > 0:
        if K > 1 and loss.stride(1) != 1:
            raise ValueError("loss must have contiguous rows (stride 1 along K)")
        if R > 1:
            ld = loss.stride(0)
            if ld < K:
                raise ValueError("loss must have a row stride of at least K elements")
        if R * ld >= 1 << 31:
            raise ValueError("R * row stride must be below 2^31")
    return R, K, ld


def rank_attribution(loss: torch.Tensor, top: int = 8, rows: Optional[torch.Tensor] = None,
                     out: Optional[RankAttribution] = None, work: Optional[torch.Tensor] = None,
                     stream=None) -> RankAttribution:
    """The ranks behind a kernel's tail loss (no reference counterpart): per column of ``loss``
    (float64 [R, K] on the device, e.g. the ``loss_all`` of any tail attribution; rows contiguous,
    a row stride above K allowed) the ``top`` (1..16) rows with the largest loss.  A NaN is not
    taken, nor is any element of a row with ``rows[r] == 0`` (``rows``: uint8 / bool [R], e.g. a
    score call's ``strag``).  Ties go to the lower row, -0.0 and +0.0 tie, and ``out.loss`` holds
    the input's bits (``histograms.rank_attribution`` is the host twin).  ``work`` (uint8, 8-byte
    aligned, at least ``rank_attribution_plan(R, K, top)[2]`` bytes) is allocated when the plan
    needs one and none is given.  One or two launches, the matrix read once; no scratch."""
    top, _ = attribution_request(top, "relative")
    R, K, ld = _rank_loss(loss)
    d = loss.device
    _u8_vector(rows, "rows", R)
    if out is None:
        out = RankAttribution.empty(K, top, d)
    _tail_tensor(out.idx, "out.idx", torch.int32, (K, top))
    _tail_tensor(out.loss, "out.loss", torch.float64, (K, top))
    _tail_tensor(out.taken, "out.taken", torch.int32, (K,))
    _tail_tensor(out.positive, "out.positive", torch.int32, (K,))
    need = rank_attribution_plan(R, K, top)[2]
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=d) if need else None
    else:
        N.require_device(work, "work")
        if (work.dtype != torch.uint8 or not work.is_contiguous() or work.numel() < need or
                work.data_ptr() % 8):
            raise ValueError(f"work must be a contiguous, 8-byte aligned uint8 tensor of at least "
                             f"{need} bytes (rank_attribution_plan)")
    a = N.RankAttrArgs(R, K, loss.data_ptr(), ld, N.ptr(rows), top, out.idx.data_ptr(),
                       out.loss.data_ptr(), out.taken.data_ptr(), out.positive.data_ptr(),
                       N.ptr(work))
    N.call("nvrx_rank_attribution", ctypes.byref(a), _stream(stream))
    return out


def kernel_ref(num: torch.Tensor, med: torch.Tensor, ref: Optional[torch.Tensor] = None,
               scratch: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """ref[k] = min_r med[r, k] if every row has k (num > 0), else NaN (reporting.py:255-296)."""
    R, K = med.shape
    if ref is None:
        ref = torch.empty(K, dtype=torch.float32, device=med.device)
    if scratch is None:
        scratch = torch.empty(2 * K, dtype=torch.int32, device=med.device)
    N.call("nvrx_kernel_ref", num.data_ptr(), med.data_ptr(), R, K, ref.data_ptr(),
           scratch.data_ptr(), _stream(stream))
    return ref


def pack_min_times(med: torch.Tensor, ids: torch.Tensor, total: int,
                   out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """times = -1; times[ids[i]] = float32(med[i]): the _all_reduce_times pack (reporting.py:269-279)."""
    if out is None:
        out = torch.empty(max(total, 1), dtype=torch.float32, device=med.device)
    N.call("nvrx_pack_min_times", med.data_ptr(), ids.data_ptr(), med.numel(), out.data_ptr(),
           total, _stream(stream))
    return out


def scores(num, med, avg, *, col_valid=None, ref=None, ref_index=None, ref_missing=None,
           hist=None, hist_index=None, hist_stride=0, partials=None, err=None,
           finalize: Optional[dict] = None, done=None, reset_col_ref=None, stream=None):
    """Per-row partial sums {sum s*w, sum w, n} for rel and indiv (reporting.py:219-253).
    finalize = dict(gpu_rel=, gpu_ind=, strag_rel=, strag_ind=, thr_rel=, thr_ind=,
    round_f32=) finishes the scores in the same kernel (single shard).  done (2 int32, zero
    before the first call): self-resetting epilogue -- err is stored, not OR-ed (no zeroing
    needed), and reset_col_ref ([2*K'] int32) is re-initialised for the next statistics call
    (segment_stats_strided(colref_ready=True))."""
    R, K = med.shape
    if partials is None and finalize is None:
        partials = torch.empty((R, 6), dtype=torch.float64, device=med.device)
    f64 = med.dtype == torch.float64
    if avg.dtype != med.dtype or (hist is not None and hist.dtype != med.dtype):
        raise TypeError("med, avg and hist must share one float dtype")
    fz = finalize or {}
    a = N.ScoreArgs(R, K, int(f64), num.data_ptr(), med.data_ptr(), avg.data_ptr(),
                    N.ptr(col_valid), N.ptr(ref), N.ptr(ref_index), N.ptr(ref_missing),
                    N.ptr(hist), N.ptr(hist_index), hist_stride, N.ptr(partials), N.ptr(err),
                    int(fz.get("round_f32", False)), float(fz.get("thr_rel", 0.75)),
                    float(fz.get("thr_ind", 0.75)), N.ptr(fz.get("gpu_rel")),
                    N.ptr(fz.get("gpu_ind")), N.ptr(fz.get("strag_rel")), N.ptr(fz.get("strag_ind")),
                    N.ptr(done), N.ptr(reset_col_ref),
                    reset_col_ref.numel() // 2 if reset_col_ref is not None else 0)
    N.call("nvrx_scores", ctypes.byref(a), _stream(stream))
    return partials


ATTRIBUTION_KINDS = {"relative": N.NVRX_ATTR_RELATIVE, "individual": N.NVRX_ATTR_INDIVIDUAL}


@dataclass
class ScoreAttribution:
    """Per row, the `top` kernels with the largest loss w*(1 - s) (device tensors):
    idx [R, top] int32 column (-1: fewer kernels than top), loss / score [R, top] float64
    (NaN where idx is -1), wsum [R] float64 total weight of the kernels taken."""

    idx: torch.Tensor
    loss: torch.Tensor
    score: torch.Tensor
    wsum: torch.Tensor


def attribution_request(top, kind):
    """(top, kind code) as the C ABI takes them: top an int in [1, NVRX_MAX_ATTRIBUTION], kind
    "relative" or "individual"; ValueError if not."""
    if isinstance(top, bool) or not isinstance(top, numbers.Integral) or \
            not 1 <= top <= N.NVRX_MAX_ATTRIBUTION:
        raise ValueError(f"top must be an int in [1, {N.NVRX_MAX_ATTRIBUTION}], got {top!r}")
    if not isinstance(kind, str) or kind not in ATTRIBUTION_KINDS:
        raise ValueError(f"kind must be one of {sorted(ATTRIBUTION_KINDS)}, got {kind!r}")
    return int(top), ATTRIBUTION_KINDS[kind]


def score_attribution(num, med, avg, *, top, kind, col_valid=None, ref=None, ref_index=None,
                      ref_missing=None, hist=None, hist_index=None, hist_stride=0, err=None,
                      out: Optional[ScoreAttribution] = None, stream=None) -> ScoreAttribution:
    """The kernels behind a score (no reference counterpart).  Inputs as ``scores``; per row the
    `top` (1..16) largest ``loss = NUM*AVG * (1 - base/MED)`` with base the relative reference
    (kind="relative": ref / ref_index / ref_missing) or the individual history as the report's
    ``scores`` call left it (kind="individual": hist / hist_index / hist_stride; read only).
    ``1 - score == loss.sum() / wsum`` over all of a row's kernels.  err (int32 [1], optional) is
    OR-ed with 1 when an eligible MED is 0 (that kernel is left out); out: preallocated outputs."""
    top, kind_code = attribution_request(top, kind)
    for name, t in (("num", num), ("med", med), ("avg", avg)):
        N.require_device(t, name)
    R, K = med.shape
    if avg.dtype != med.dtype or (hist is not None and hist.dtype != med.dtype):
        raise TypeError("med, avg and hist must share one float dtype")
    if kind_code == N.NVRX_ATTR_RELATIVE and ref is None:
        raise ValueError("kind='relative' needs ref")
    if kind_code == N.NVRX_ATTR_INDIVIDUAL and hist is None:
        raise ValueError("kind='individual' needs hist")
    if out is None:
        d = med.device
        out = ScoreAttribution(torch.empty((R, top), dtype=torch.int32, device=d),
                               torch.empty((R, top), dtype=torch.float64, device=d),
                               torch.empty((R, top), dtype=torch.float64, device=d),
                               torch.empty(R, dtype=torch.float64, device=d))
    elif (out.idx.numel() != R * top or out.loss.numel() != R * top or
          out.score.numel() != R * top or out.wsum.numel() != R):
        raise ValueError("score_attribution: preallocated outputs do not match [R, top]")
    a = N.AttributionArgs(R, K, int(med.dtype == torch.float64), num.data_ptr(), med.data_ptr(),
                          avg.data_ptr(), N.ptr(col_valid), N.ptr(ref), N.ptr(ref_index),
                          N.ptr(ref_missing), N.ptr(hist), N.ptr(hist_index), hist_stride,
                          kind_code, top, out.idx.data_ptr(), out.loss.data_ptr(),
                          out.score.data_ptr(), out.wsum.data_ptr(), N.ptr(err))
    N.call("nvrx_score_attribution", ctypes.byref(a), _stream(stream))
    return out


@dataclass
class ScoreRankAttribution:
    """Per column (kernel) of ``score_rank_attribution`` (device tensors), the ``top`` rows (ranks)
    with the largest loss w*(1 - s), largest first: idx [K, top] int32 row (-1: fewer rows taken),
    loss / score [K, top] float64 (NaN where idx is -1), taken [K] int32 rows taken, positive [K]
    int32 taken rows whose loss is > 0."""

    idx: torch.Tensor
    loss: torch.Tensor
    score: torch.Tensor
    taken: torch.Tensor
    positive: torch.Tensor

    @staticmethod
    def nbytes(K: int, top: int) -> int:
        """Bytes of the packed form: loss, score (8 each), idx (4) per (column, j); taken, positive
        (4 each)."""
        return 20 * K * top + 8 * K

    @classmethod
    def empty(cls, K: int, top: int, device) -> "ScoreRankAttribution":
        return cls.packed(torch.empty(cls.nbytes(K, top), dtype=torch.uint8, device=device), K, top)

    @classmethod
    def packed(cls, buf: torch.Tensor, K: int, top: int) -> "ScoreRankAttribution":
        """Views of the outputs in one 8-byte aligned uint8 buffer of ``nbytes(K, top)`` bytes (the
        f64 fields first), so that one copy moves them all; ``unpack`` reads it back."""
        n = K * top
        f = buf[:16 * n].view(torch.float64)
        d = buf[16 * n:20 * n + 8 * K].view(torch.int32)
        return cls(d[:n].view(K, top), f[:n].view(K, top), f[n:].view(K, top),
                   d[n:n + K], d[n + K:n + 2 * K])

    @staticmethod
    def unpack(host: np.ndarray, K: int, top: int):
        """The host copy of a ``packed`` buffer as numpy arrays: (idx [K, top] i32, loss [K, top]
        f64, score [K, top] f64, taken [K] i32, positive [K] i32)."""
        n = K * top
        f = host[:16 * n].view(np.float64).copy()
        d = host[16 * n:20 * n + 8 * K].view(np.int32).copy()
        return (d[:n].reshape(K, top), f[:n].reshape(K, top), f[n:].reshape(K, top),
                d[n:n + K], d[n + K:n + 2 * K])


def score_rank_attribution(num, med, avg, *, top, kind, col_valid=None, ref=None, ref_index=None,
                           ref_missing=None, hist=None, hist_index=None, hist_stride=0, rows=None,
                           err=None, out: Optional[ScoreRankAttribution] = None,
                           work: Optional[torch.Tensor] = None, stream=None) -> ScoreRankAttribution:
    """The ranks behind a kernel's score loss (no reference counterpart): the converse of
    ``score_attribution``.  Inputs as ``score_attribution``; per column the ``top`` (1..16) rows
    with the largest ``loss = NUM*AVG * (1 - base/MED)`` among the elements ``score_attribution``
    would take, exactly what ``rank_attribution`` gives for the matrix of those losses (NaN where
    not taken) -- which is never built -- plus the winners' ``s``.  ``rows`` (uint8 / bool [R]):
    a row with 0 is not taken.  err (int32 [1], optional) is OR-ed with 1 when an eligible MED of
    a row that is on is 0.  ``work`` as for ``rank_attribution``: sized by
    ``rank_attribution_plan(R, K, top)``, allocated when the plan needs one and none is given.
    ``histograms.score_rank_attribution`` is the host twin."""
    top, kind_code = attribution_request(top, kind)
    for name, t in (("num", num), ("med", med), ("avg", avg)):
        N.require_device(t, name)
    if med.dim() != 2 or num.shape != med.shape or avg.shape != med.shape:
        raise ValueError("num, med and avg must share one shape [R, K]")
    R, K = med.shape
    if num.dtype != torch.int32 or med.dtype not in (torch.float32, torch.float64):
        raise TypeError("num must be int32, med and avg float32 or float64")
    if avg.dtype != med.dtype or (hist is not None and hist.dtype != med.dtype):
        raise TypeError("med, avg and hist must share one float dtype")
    if not (num.is_contiguous() and med.is_contiguous() and avg.is_contiguous()):
        raise ValueError("num, med and avg must be contiguous")
    if kind_code == N.NVRX_ATTR_RELATIVE and ref is None:
        raise ValueError("kind='relative' needs ref")
    if kind_code == N.NVRX_ATTR_INDIVIDUAL and hist is None:
        raise ValueError("kind='individual' needs hist")
    if hist_index is not None and hist_stride <= 0:
        raise ValueError("hist_index needs hist_stride")
    if R >= 1 << 31 or K >= 1 << 31:
        raise ValueError("R and K must be below 2^31")
    d = med.device
    _u8_vector(rows, "rows", R)
    if out is not None:
        _tail_tensor(out.idx, "out.idx", torch.int32, (K, top))
        _tail_tensor(out.loss, "out.loss", torch.float64, (K, top))
        _tail_tensor(out.score, "out.score", torch.float64, (K, top))
        _tail_tensor(out.taken, "out.taken", torch.int32, (K,))
        _tail_tensor(out.positive, "out.positive", torch.int32, (K,))
    need = rank_attribution_plan(R, K, top)[2]
    if work is not None:
        N.require_device(work, "work")
        if (work.dtype != torch.uint8 or not work.is_contiguous() or work.numel() < need or
                work.data_ptr() % 8):
            raise ValueError(f"work must be a contiguous, 8-byte aligned uint8 tensor of at least "
                             f"{need} bytes (rank_attribution_plan)")
    # every refusal is above: nothing has been allocated yet
    if out is None:
        out = ScoreRankAttribution.empty(K, top, d)
    if work is None and need:
        work = torch.empty(need, dtype=torch.uint8, device=d)
    a = N.ScoreRankArgs(R, K, int(med.dtype == torch.float64), num.data_ptr(), med.data_ptr(),
                        avg.data_ptr(), N.ptr(col_valid), N.ptr(ref), N.ptr(ref_index),
                        N.ptr(ref_missing), N.ptr(hist), N.ptr(hist_index), hist_stride,
                        kind_code, top, N.ptr(rows), out.idx.data_ptr(), out.loss.data_ptr(),
                        out.score.data_ptr(), out.taken.data_ptr(), out.positive.data_ptr(),
                        N.ptr(err), N.ptr(work))
    N.call("nvrx_score_rank_attribution", ctypes.byref(a), _stream(stream))
    return out


def finalize_scores(partials: torch.Tensor, R: int, nshards: int = 1, round_f32: bool = False,
                    thr_rel: float = 0.75, thr_ind: float = 0.75, rel=True, ind=True, err=None,
                    out: Optional[dict] = None, stream=None):
    """Scores + straggler masks from [nshards][R][6] partials (shards summed in order)."""
    dev = partials.device
    o = out or {}
    gr = o.get("gpu_rel", torch.empty(R, dtype=torch.float64, device=dev) if rel else None)
    gi = o.get("gpu_ind", torch.empty(R, dtype=torch.float64, device=dev) if ind else None)
    sr = o.get("strag_rel", torch.empty(R, dtype=torch.uint8, device=dev) if rel else None)
    si = o.get("strag_ind", torch.empty(R, dtype=torch.uint8, device=dev) if ind else None)
    N.call("nvrx_finalize_scores", partials.data_ptr(), R, nshards, int(round_f32),
           float(thr_rel), float(thr_ind), N.ptr(gr), N.ptr(gi), N.ptr(sr), N.ptr(si),
           N.ptr(err), _stream(stream))
    return gr, gi, sr, si


def section_scores(med: torch.Tensor, present: torch.Tensor, *, ref_in=None, ref_index=None,
                   hist=None, round_f32=False, rel=True, ind=True, err=None, stream=None):
    R, S = med.shape
    dev = med.device
    out_rel = torch.empty((R, S), dtype=torch.float64, device=dev) if rel else None
    out_ind = torch.empty((R, S), dtype=torch.float64, device=dev) if ind else None
    ref_work = torch.empty(S, dtype=torch.float32, device=dev) if (rel and ref_in is None) else None
    N.call("nvrx_section_scores", med.data_ptr(), present.data_ptr(), R, S, N.ptr(ref_in),
           N.ptr(ref_index), N.ptr(ref_work), N.ptr(hist), int(round_f32), N.ptr(out_rel),
           N.ptr(out_ind), N.ptr(err), _stream(stream))
    return out_rel, out_ind


def section_stats(values: torch.Tensor, off: torch.Tensor, max_len: int, stream=None):
    """Per-section (num, min, max, med, avg, std) of float64 ms timings (straggler.py:171-197)."""
    nsec = off.numel() - 1
    dev = values.device
    num = torch.empty(nsec, dtype=torch.int32, device=dev)
    out = torch.empty((5, nsec), dtype=torch.float64, device=dev)
    N.call("nvrx_section_stats", values.data_ptr(), off.data_ptr(), nsec, max_len, num.data_ptr(),
           *(out[i].data_ptr() for i in range(5)), _stream(stream))
    return num, out


def stragglers(score: torch.Tensor, thr: float, out: Optional[torch.Tensor] = None, stream=None):
    if out is None:
        out = torch.empty(score.numel(), dtype=torch.uint8, device=score.device)
    N.call("nvrx_stragglers", score.data_ptr(), score.numel(), float(thr), out.data_ptr(),
           _stream(stream))
    return out


def records_bucket_capacity(n: int, nstreams: int, nslots: int) -> int:
    return int(N.lib().nvrx_records_bucket_capacity(n, nstreams, nslots))


def records_bucket(recs: torch.Tensor, rec_off: torch.Tensor, nslots: int, cap: int, stream=None,
                   out=None):
    """recs: [n, 2] uint32/int32 {slot, ns}; rec_off: [nstreams+1] int64 (device).
    Returns (seg_off int64 [nstreams*nslots], seg_len int32, out_ns, counts int32); `out`
    may pass that tuple preallocated (out_ns >= records_bucket_capacity(...) elements)."""
    nstreams = rec_off.numel() - 1
    dev = recs.device
    n = recs.shape[0]
    cap_ns = records_bucket_capacity(n, nstreams, nslots)
    if out is None:
        seg_off = torch.empty(nstreams * nslots, dtype=torch.int64, device=dev)
        seg_len = torch.empty(nstreams * nslots, dtype=torch.int32, device=dev)
        counts = torch.empty(nstreams * nslots, dtype=torch.int32, device=dev)
        out_ns = torch.empty(max(cap_ns, 1), dtype=torch.int32, device=dev)
    else:
        seg_off, seg_len, out_ns, counts = out
        if (seg_off.numel() < nstreams * nslots or seg_len.numel() < nstreams * nslots or
                counts.numel() < nstreams * nslots or out_ns.numel() < cap_ns):
            raise ValueError("records_bucket: preallocated outputs too small")
    N.call("nvrx_records_bucket", recs.data_ptr(), rec_off.data_ptr(), nstreams, nslots, cap,
           seg_off.data_ptr(), seg_len.data_ptr(), out_ns.data_ptr(), counts.data_ptr(),
           _stream(stream))
    return seg_off, seg_len, out_ns, counts


def records_stats(recs: torch.Tensor, rec_off: torch.Tensor, nslots: int, cap: int, max_len: int,
                  mode: int = STATS_FAST, out: Optional[SegmentStats] = None, bucket=None,
                  col_ref: Optional[torch.Tensor] = None, stream=None) -> SegmentStats:
    """Per-(stream, slot) statistics of push-ordered record streams (ring retention of the
    last `cap` + computeStats): bucketing, then the length-classed segment kernels.  `bucket` may pass the
    (seg_off, seg_len, out_ns, counts) work tensors preallocated (counts may be None: the pushes
    per bucket are then not written); col_ref ([2*nslots] int32) receives the per-slot reference
    (min over streams of MED | missing)."""
    nstreams = rec_off.numel() - 1
    dev = recs.device
    n = recs.shape[0]
    cap_ns = records_bucket_capacity(n, nstreams, nslots)
    if bucket is None:
        bucket = (torch.empty(nstreams * nslots, dtype=torch.int64, device=dev),
                  torch.empty(nstreams * nslots, dtype=torch.int32, device=dev),
                  torch.empty(max(cap_ns, 1), dtype=torch.int32, device=dev),
                  torch.empty(nstreams * nslots, dtype=torch.int32, device=dev))
    seg_off, seg_len, out_ns, counts = bucket
    if out_ns.numel() < cap_ns or seg_off.numel() < nstreams * nslots:
        raise ValueError("records_stats: preallocated work tensors too small")
    if out is None:
        out = SegmentStats.empty(nstreams * nslots, dev)
    soa = out.soa()
    N.call("nvrx_records_stats", recs.data_ptr(), rec_off.data_ptr(), nstreams, nslots, cap, mode,
           max_len, seg_off.data_ptr(), seg_len.data_ptr(), out_ns.data_ptr(), N.ptr(counts),
           ctypes.byref(soa), N.ptr(col_ref), _stream(stream))
    return out
