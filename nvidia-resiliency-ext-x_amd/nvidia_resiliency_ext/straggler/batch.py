"""Batched scoring of many (simulated) ranks resident in HBM -- the hot path at scale.

``MatrixReporter`` runs the whole report for R ranks x K kernels in one pass over a
u32 duration-key matrix ``[R][K][S_push]`` (``_native.duration_keys``: the integer ns below
3.76 s; raw u32 ns reaching 3.76 s must go through ``ops.encode_ns_u32_`` first) (the last ``cap`` samples of every (rank, kernel)
retained, as the reference's per-kernel rings keep them), or over R push-ordered record
streams ``{slot, ns}`` (``compute_stats_records``: bucket by slot keeping the last ``cap``
of each, then length-classed segment statistics -- configs[3]):

  segment_stats (HIP) -> per-kernel reference = min over ranks (HIP)
  -> per-rank weighted relative / individual partial sums (HIP)
  -> [multi-GPU: one RCCL all_gather of the partials]
  -> scores + straggler masks (HIP) -> host.

It is the same arithmetic the reference ReportGenerator performs once per rank
(reporting.py:421-554) on the stats computeStats produced (CuptiProfiler.cpp:44-74),
batched over ranks.  Multi-GPU: the kernel columns are sharded by hash(kernel name) %
world size; every GPU holds all R ranks for its kernels, so the per-kernel reference
and the history are shard-local and the only exchange is the [R][6] f64 partials.
"""
from __future__ import annotations

import weakref
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import histograms, ops
from .host_wait import (SPIN_BOUND_US, SYNC_MODES, _wait, set_sync_mode,  # noqa: F401
                        sync_mode, wait_event)


def __getattr__(name: str):  # report_graphs imports this module: its names resolve on first use
    if name in ("ReportGraph", "PipelinedReports", "PIPE_ALT_MAX_BYTES", "TIMED_SPIN_CYCLES", "STAGGER_FRAC"):
        from . import report_graphs
        return getattr(report_graphs, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# The per-kernel reference (min over ranks of MED) is fused into the stats epilogue as one
# global atomicMin per segment.  Those atomics serialise per column: with R rows every
# column address takes R of them, which costs more than a separate column reduction
# (kernel_ref: 64 rows per thread, R/64 atomics per column) once R is in the hundreds
# (measured on MI355X: 885k segments on 54 columns, 0.6 ms -> 4.3 ms fused).
FUSED_REF_MAX_ROWS = 256


@dataclass
class BatchResult:
    gpu_relative: Optional[np.ndarray]     # [R] f64 (NaN: no common kernel)
    gpu_individual: Optional[np.ndarray]   # [R] f64
    stragglers_relative: Optional[np.ndarray]   # [R] bool, score < thr_rel
    stragglers_individual: Optional[np.ndarray]  # [R] bool, score < thr_ind
    err: int = 0


@dataclass
class BatchAttribution:
    """MatrixReporter.attribute: per rank the `top` kernels that cost it most of its score."""
    kernel: np.ndarray    # [R, top] i32 kernel column, largest loss first (-1: no further kernel)
    loss_us: np.ndarray   # [R, top] f64 NUM*AVG * (1 - base/MED), NaN where kernel is -1
    score: np.ndarray     # [R, top] f64 base/MED of that kernel
    share: np.ndarray     # [R, top] f64 loss_us / wsum: the kernel's part of 1 - score
    wsum: np.ndarray      # [R] f64 total weight of the rank's scored kernels
    err: int = 0          # 1: some scored MED was 0 (that kernel is left out)


@dataclass
class BatchTailAttribution:
    """``tail_scores(attribute=top)`` / ``individual_tail_scores(attribute=top)``: per rank the
    `top` kernels with the largest excess tail time, largest first (ties: the lower column)."""
    kernel: np.ndarray            # [R, top] i32 kernel column (-1: no further kernel taken)
    loss_ns: np.ndarray           # [R, top] f64 tail_ns - total_ns * base_share, NaN where kernel is -1
    tail_ns: np.ndarray           # [R, top] u64 the kernel's weighted counts above its threshold bucket
    total_ns: np.ndarray          # [R, top] u64 all its weighted counts
    tail_calls: np.ndarray        # [R, top] u32 its calls above the threshold bucket
    threshold_bucket: np.ndarray  # [R, top] i32 (-1 where kernel is -1)
    base_share: np.ndarray        # [R, top] f64 the tail's share of the base's time on that kernel
    loss_all: Optional[torch.Tensor] = None  # [R, K] f64 on the device: every kernel's loss (NaN: not taken)

    @classmethod
    def unpack(cls, host: np.ndarray, R: int, top: int, loss_all) -> "BatchTailAttribution":
        """From the host copy of ``ops.TailAttribution.packed``'s buffer."""
        return cls(*ops.TailAttribution.unpack(host, R, top), loss_all)


@dataclass
class BatchKernelRanks:
    """``MatrixReporter.kernel_ranks``: per kernel the `top` ranks with the largest excess tail time,
    largest first (ties: the lower rank)."""
    rank: np.ndarray      # [K, top] i32 rank (-1: no further rank taken)
    loss_ns: np.ndarray   # [K, top] f64 the matrix's element, bit for bit; NaN where rank is -1
    taken: np.ndarray     # [K] i32 ranks taken: not NaN, and flagged when ``flagged`` is given
    positive: np.ndarray  # [K] i32 taken ranks that lost time on the kernel at all (loss > 0)


@dataclass
class BatchScoreKernelRanks:
    """``MatrixReporter.score_kernel_ranks``: per kernel the `top` ranks with the largest loss
    ``NUM*AVG * (1 - base/MED)`` behind the median scores, largest first (ties: the lower rank)."""
    rank: np.ndarray      # [K, top] i32 rank (-1: no further rank taken)
    loss_us: np.ndarray   # [K, top] f64 the rank's loss on the kernel, NaN where rank is -1
    score: np.ndarray     # [K, top] f64 base/MED of that rank on the kernel
    taken: np.ndarray     # [K] i32 ranks taken: scored on the kernel, and flagged when ``flagged`` is given
    positive: np.ndarray  # [K] i32 taken ranks that lose on the kernel at all (loss > 0)
    err: int = 0          # 1: some scored MED was 0 (that element is left out)


def _flagged_rows(flagged, R: int, device):
    """``flagged`` of the kernel-ranks calls as a tensor (None: every rank): bool / uint8 [R], a
    numpy array or a tensor on the host or on ``device``; ValueError if not."""
    if flagged is None:
        return None
    rows = flagged if isinstance(flagged, torch.Tensor) else torch.from_numpy(np.asarray(flagged))
    if rows.dtype not in (torch.bool, torch.uint8) or tuple(rows.shape) != (R,):
        raise ValueError(f"flagged must be a bool / uint8 array or tensor of shape [{R}]")
    if rows.is_cuda and rows.device != device:
        raise ValueError("flagged must be on the host or on the reporter's device")
    return rows


def _rows_on_device(rows, scratch: torch.Tensor):
    """The checked ``flagged`` as the uint8 device vector the kernels read: itself when it is
    already one, else copied into ``scratch`` (uint8 [R] on the device)."""
    if rows is None:
        return None
    if rows.is_cuda and rows.is_contiguous():
        return rows.view(torch.uint8) if rows.dtype == torch.bool else rows
    scratch.copy_(rows.view(torch.uint8) if rows.dtype == torch.bool else rows)
    return scratch


@dataclass
class BatchTailScores:
    """MatrixReporter.tail_scores: per rank a score from the tails of the fleet's histograms."""
    score: np.ndarray             # [R] f64, about 1 healthy, lower = more time in the tail; NaN: no samples
    tail_ns: np.ndarray           # [R] u64 weighted counts above the threshold buckets (ns, lower bound)
    total_ns: np.ndarray          # [R] u64 all weighted counts
    fleet_share: float            # fleet_tail / fleet_total: the tail's share of the fleet's time
    stragglers: np.ndarray        # [R] bool, score < threshold (NaN never)
    threshold_bucket: np.ndarray  # [K] i32 bucket T_k of the fleet's quantile (-1: kernel skipped)
    tail_calls: Optional[torch.Tensor] = None  # [R, K] int32 on the device, on request
    attribution: Optional[BatchTailAttribution] = None  # with attribute > 0


@dataclass
class BatchIndividualTailScores:
    """MatrixReporter.individual_tail_scores: per rank a score from the tail of its histograms
    against its own history."""
    score: np.ndarray             # [R] f64, about 1 healthy, lower = more time in its own tail; NaN: no history
    tail_ns: np.ndarray           # [R] u64 weighted counts above the history's threshold buckets
    total_ns: np.ndarray          # [R] u64 weighted counts of the kernels scored
    history_share: np.ndarray     # [R] f64 base_tail / base_total: the tail's share of the history's time
    stragglers: np.ndarray        # [R] bool, score < threshold (NaN never)
    base_tail_ns: np.ndarray      # [R] u64
    base_total_ns: np.ndarray     # [R] u64
    tail_calls: Optional[torch.Tensor] = None  # [R, K] int32 on the device, on request
    folded: Optional[np.ndarray] = None  # [R] u64 samples folded, with history="compact"
    attribution: Optional[BatchTailAttribution] = None  # with attribute > 0


@dataclass
class TailHistoryAging:
    """MatrixReporter.age_tail_history: what the age pass did to the compact history (both None
    when the reporter has no compact history or it was not aged)."""
    evicted: Optional[np.ndarray] = None  # [R] u64 entries freed per rank
    full: Optional[np.ndarray] = None     # [R] u64 elements per rank that still hold 12 entries


ABSORB_MODES = ("healthy", "always", "never")
HISTORY_KINDS = ("dense", "compact", "both")


@dataclass(eq=False)
class _ReportBuffers:
    """The device buffers of one report: segment statistics, the per-kernel reference the
    statistics epilogue produces ([min bits | missing]; + its f32 form for the column reduction),
    the scores epilogue's completion counter, the packed results, on N GPUs the shard's partials
    and their gathered copy, and the record-stream bucketing scratch (allocated and grown by
    compute_stats_records).  clean: col_ref holds the initial reference (set by the scores
    epilogue).  A MatrixReporter owns one set; PipelinedReports adds one per further report in
    flight.  The class also owns the packed-result layout -- one device-to-host copy per report:
    [gpu_rel f64 R][gpu_ind f64 R][strag_rel u8 R][strag_ind u8 R][pad][err i32]"""
    R: int
    relative: bool
    individual: bool
    stats: ops.SegmentStats
    col_ref: torch.Tensor
    ref_f32: torch.Tensor
    # self-resetting scores epilogue (nvrx_score_args.done, zero before the first report): the
    # scores kernel's last workgroup stores the error bits and re-initialises col_ref for the next
    # report, so a report is two launches (statistics, scores) with no initialising fill in between
    done: torch.Tensor
    out: torch.Tensor
    partials: torch.Tensor
    gathered: Optional[torch.Tensor]
    bucket: Optional[tuple] = None
    clean: bool = False

    def __post_init__(self):
        self.err = self.err_of(self.out)

    @classmethod
    def new(cls, rep: "MatrixReporter") -> "_ReportBuffers":
        """A fresh set for a reporter: results and completion counter zeroed, the column
        reference uninitialised (its first statistics phase initialises it), no scratch yet."""
        R, K, d = rep.R, rep.K, rep.device
        return cls(R, rep.relative, rep.individual,
                   stats=ops.SegmentStats.empty(R * K, d),
                   col_ref=torch.empty(2 * max(K, 1), dtype=torch.int32, device=d),
                   ref_f32=torch.empty(max(K, 1), dtype=torch.float32, device=d),
                   done=torch.zeros(2, dtype=torch.int32, device=d),
                   out=torch.zeros(cls.nbytes(R), dtype=torch.uint8, device=d),
                   partials=torch.empty((R, 6), dtype=torch.float64, device=d),
                   gathered=(torch.empty((rep.world, R, 6), dtype=torch.float64, device=d)
                             if rep.exchange else None))

    @staticmethod
    def nbytes(R: int) -> int:
        return (18 * R + 7) // 8 * 8 + 8

    def _split(self, b):
        """The byte ranges of a packed buffer (a uint8 tensor or numpy array)."""
        R, e = self.R, self.nbytes(self.R) - 8
        return b[0:8 * R], b[8 * R:16 * R], b[16 * R:17 * R], b[17 * R:18 * R], b[e:e + 4]

    def views(self, buf: Optional[torch.Tensor] = None) -> dict:
        """The result arrays inside a packed buffer (default: this set's)."""
        gr, gi, sr, si, _ = self._split(self.out if buf is None else buf)
        return dict(gpu_rel=gr.view(torch.float64) if self.relative else None,
                    gpu_ind=gi.view(torch.float64) if self.individual else None,
                    strag_rel=sr if self.relative else None,
                    strag_ind=si if self.individual else None)

    def err_of(self, buf: torch.Tensor) -> torch.Tensor:
        return self._split(buf)[4].view(torch.int32)

    def unpack(self, buf: torch.Tensor) -> BatchResult:
        """Host copies of the results in a packed host buffer."""
        gr, gi, sr, si, err = self._split(buf.numpy())
        return BatchResult(gr.view(np.float64).copy() if self.relative else None,
                           gi.view(np.float64).copy() if self.individual else None,
                           sr.astype(bool) if self.relative else None,
                           si.astype(bool) if self.individual else None,
                           int(err.view(np.int32)[0]))


def _half_life(half_life) -> Optional[int]:
    """``half_life=`` of the individual tail scores: None or an int >= 1; ValueError if not."""
    if half_life is None:
        return None
    if isinstance(half_life, bool) or not isinstance(half_life, (int, np.integer)) or half_life < 1:
        raise ValueError(f"half_life must be None or an int >= 1, got {half_life!r}")
    return int(half_life)


class _FleetTailLayout:
    """The packed results of the fleet's tail scores (``tail_scores``, ``tail_scores_records``), one
    device-to-host copy per call:
    [score f64 R][tail_ns i64 R][total_ns i64 R][fleet_sums i64 2][thr i32 K+pad][strag u8 R]"""

    def __init__(self, R: int, K: int):
        self.R, self.K = R, K
        self.thr = 8 * (3 * R + 2)                      # the 8-byte fields end, thr begins
        self.strag = self.thr + 4 * ((K + 1) // 2 * 2)  # (thr padded to 8 bytes)
        self.nbytes = self.strag + R

    def views(self, buf: torch.Tensor):
        """(outputs, thr [K], fleet_sums [2]): the device views of a packed buffer."""
        R = self.R
        i64 = buf[:self.thr].view(torch.int64)
        out = ops.TailScores(i64[:R].view(torch.float64), i64[R:2 * R], i64[2 * R:3 * R],
                             buf[self.strag:self.nbytes])
        return out, buf[self.thr:self.strag].view(torch.int32)[:self.K], i64[3 * R:]

    def unpack(self, host: np.ndarray, tail_calls, attribution) -> BatchTailScores:
        """The results in the host copy of a packed buffer."""
        R = self.R
        h64 = host[:self.thr].view(np.uint64)
        ftail, ftotal = int(h64[3 * R]), int(h64[3 * R + 1])
        return BatchTailScores(h64[:R].view(np.float64).copy(), h64[R:2 * R].copy(),
                               h64[2 * R:3 * R].copy(),
                               float(ftail) / float(ftotal) if ftotal else float("nan"),
                               host[self.strag:self.nbytes].astype(bool),
                               host[self.thr:self.strag].view(np.int32)[:self.K].copy(),
                               tail_calls, attribution)


class _HistoryTailLayout:
    """The packed results of the individual tail scores, one device-to-host copy per call
    (``ops.HistoryTailScores.packed``; ``folded`` with the compact history only):
    [score f64 R][tail_ns][total_ns][base_tail_ns][base_total_ns i64 R]([folded i64 R])[strag u8 R]"""

    def __init__(self, R: int, folded: bool):
        self.R, self.folded = R, folded
        self.nbytes = 49 * R if folded else 41 * R

    def views(self, buf: torch.Tensor):
        """(outputs, folded [R] or None): the device views of a packed buffer."""
        return ops.HistoryTailScores.packed(buf, self.R, self.folded)

    def unpack(self, host: np.ndarray, tail_calls, attribution) -> BatchIndividualTailScores:
        """The results in the host copy of a packed buffer."""
        score, tail, total, btail, btotal, strag, folded = ops.HistoryTailScores.unpack(
            host, self.R, self.folded)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(btotal != 0, btail.astype(np.float64) / btotal.astype(np.float64), np.nan)
        return BatchIndividualTailScores(score, tail, total, share, strag, btail, btotal, tail_calls,
                                         folded=folded, attribution=attribution)


class _CountsSource:
    """An interval given as histogram counts [R, K, 240], for the tail-score drivers: each
    operation is the ``ops`` entry that takes counts.  ``_BucketSource`` is its twin."""

    def __init__(self, counts: torch.Tensor):
        self.counts = counts

    def fleet_histogram(self, out):
        ops.histogram_sum(self.counts, out=out)

    def fleet_scores(self, thr, sums, **kw):
        return ops.histogram_tail_scores(self.counts, thr, sums, **kw)

    def fleet_attribution(self, thr, base, **kw):
        ops.histogram_tail_attribution(self.counts, kind="relative", thr=thr, base=base, **kw)

    def history_scores(self, hist, compact: bool, **kw):
        """Score against / update the dense history, or the compact one (``folded=`` in kw)."""
        if compact:
            return ops.histogram_history_scores_compact(self.counts, hist, **kw)[0]
        return ops.histogram_history_scores(self.counts, hist, **kw)

    def history_attribution(self, hist, **kw):
        ops.histogram_tail_attribution(self.counts, kind="individual", hist=hist, **kw)

    def compact_history_attribution(self, chist, **kw):
        ops.histogram_history_attribution_compact(self.counts, chist, **kw)


class _BucketSource:
    """An interval given as the buckets a record-stream call laid out (``records_bucket``: every
    bucket written out, trimmed to ``cap``, the starts padded to 16 bytes), for the tail-score
    drivers: each operation is the ragged ``ops`` entry, without the counts."""

    def __init__(self, out_ns, seg_off, seg_len, K: int, max_len: int):
        self.segs = (out_ns, seg_off, seg_len, K, max_len)

    def fleet_histogram(self, out):
        ops.segment_fleet_histogram_ragged(*self.segs, aligned16=True, out=out)

    def fleet_scores(self, thr, sums, **kw):
        return ops.segment_tail_scores_ragged(*self.segs, thr, sums, aligned16=True, **kw)

    def fleet_attribution(self, thr, base, **kw):
        ops.segment_tail_attribution_ragged(*self.segs, thr, base, aligned16=True, **kw)

    def history_scores(self, hist, compact: bool, **kw):
        if compact:
            return ops.segment_history_scores_compact_ragged(*self.segs, hist, aligned16=True, **kw)[0]
        return ops.segment_history_scores_ragged(*self.segs, hist, aligned16=True, **kw)

    def history_attribution(self, hist, **kw):
        ops.segment_history_attribution_ragged(*self.segs, hist, aligned16=True, **kw)

    def compact_history_attribution(self, chist, **kw):
        ops.segment_history_attribution_compact_ragged(*self.segs, chist, aligned16=True, **kw)


class MatrixReporter:
    def __init__(self, R: int, K: int, *, cap: int = 8192, relative: bool = True,
                 individual: bool = True, thr_rel: float = 0.75, thr_ind: float = 0.75,
                 col_valid: Optional[torch.Tensor] = None, mode: int = ops.STATS_FAST,
                 round_f32: bool = False, group=None, device=None, exchange: Optional[bool] = None):
        self.R, self.K, self.cap = R, K, cap
        self.relative, self.individual = relative, individual
        self.thr_rel, self.thr_ind = thr_rel, thr_ind
        self.mode, self.round_f32 = mode, round_f32
        self.group = group
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        d = self.device
        self.world = 1
        self.gloo = False
        if group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(group)
            self.gloo = torch.distributed.get_backend(group) == torch.distributed.Backend.GLOO
        # exchange: the multi-GPU scoring (partials -> all_gather -> finalize) even in a world
        # of one -- how a one-GPU box runs the RCCL branch (tests); default: world > 1
        self.exchange = self.world > 1 if exchange is None else bool(exchange)
        if self.exchange and not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            raise RuntimeError("MatrixReporter(exchange=True) needs an initialized process group")
        self.col_valid = col_valid
        # the reporter's own buffer set: what every phase below uses unless it is given another
        # (bufs=); the history and the pinned result buffer are shared by all sets
        self.own = _ReportBuffers.new(self)
        self.hist = torch.full((R, K), float("inf"), dtype=torch.float32, device=d) if individual else None
        self.h_out = torch.empty(_ReportBuffers.nbytes(R), dtype=torch.uint8, pin_memory=True)
        self._pipes = weakref.WeakSet()  # PipelinedReports over this reporter
        self._attr_ref = None  # attribute(): its own column reference and packed outputs per top
        self._attr_out = {}
        self._tail = None  # tail_scores(): fleet histogram and packed outputs, allocated at first use
        self._htail = None  # individual_tail_scores(): [R][K][240] history and packed outputs, likewise
        self._rtail = None  # tail_scores_records(): bucketing work tensors, fleet histogram, packed outputs
        self._ctail = None  # the compact methods (history="compact"): [R][K][64] history, packed outputs
        self._kranks = {}  # kernel_ranks(): packed outputs, work space and row mask per top
        self._sranks = {}  # score_kernel_ranks(): likewise, plus the error word
        # half_life=: absorbing calls per history since its last aging or reset_tail_history
        self._absorbed = {"dense": 0, "compact": 0}

    @property
    def stats(self) -> ops.SegmentStats:
        """The segment statistics of the reporter's own buffer set."""
        return self.own.stats

    def _order_after_inflight(self, exclude=None) -> None:
        """The caller's stream waits for every pipelined report still in flight on this reporter.
        Those reports run on private streams and use slot 0's buffers (the reporter's own
        statistics, reference and results) and the shared history, so an eager report, a graph
        replay or a history reset issued between submit() and collect() queues behind them
        instead of racing them.  A no-op while a graph is being captured (the captures pair
        their phases themselves) and with nothing in flight."""
        if not self._pipes or torch.cuda.is_current_stream_capturing():
            return
        cur = torch.cuda.current_stream(self.device)
        for p in list(self._pipes):
            if p is not exclude:
                for k, _ in p.pending:
                    cur.wait_event(p.done[k])

    def reset_history(self):
        if self.hist is not None:
            self._order_after_inflight()
            self.hist.fill_(float("inf"))

    # -- device phases, separately callable (bench times the stats kernel) --
    def _fuse_ref(self) -> bool:
        return self.relative and self.R <= FUSED_REF_MAX_ROWS

    # (bufs: the buffer set a phase reads and writes; None: the reporter's own)
    def _column_ref(self, bufs: Optional[_ReportBuffers] = None):
        """Per-kernel reference by a separate column reduction into the col_ref layout."""
        b = self.own if bufs is None else bufs
        if self.relative and not self._fuse_ref():
            st = b.stats.view(self.R, self.K)
            ops.kernel_ref(st.num, st.med, ref=b.ref_f32, scratch=b.col_ref)

    def compute_stats(self, ns: torch.Tensor, s_push: int,
                      bufs: Optional[_ReportBuffers] = None) -> ops.SegmentStats:
        # (inside a graph capture the flag describes the device state when the graph replays:
        # the captured sequences always pair a statistics call with the scores that follow)
        b = self.own if bufs is None else bufs
        self._order_after_inflight()
        st = ops.segment_stats_strided(ns.view(-1), self.R * self.K, s_push, 0, s_push,
                                       cap=self.cap, mode=self.mode, out=b.stats,
                                       col_ref=b.col_ref if self._fuse_ref() else None,
                                       ncols=self.K, colref_ready=b.clean)
        b.clean = False
        self._column_ref(b)
        return st

    def _bucket_scratch(self, have: Optional[tuple], n: int, pushes: bool) -> tuple:
        """The record-stream bucketing scratch for ``n`` records -- (seg_off i64, seg_len i32,
        bucketed ns i32, per-bucket push counts i32 or None) -- ``have`` where it holds them."""
        need = ops.records_bucket_capacity(n, self.R, self.K)
        if have is not None and have[2].numel() >= need:
            return have
        d, nseg = self.device, self.R * self.K
        return (torch.empty(nseg, dtype=torch.int64, device=d),
                torch.empty(nseg, dtype=torch.int32, device=d),
                torch.empty(max(need, 1), dtype=torch.int32, device=d),
                torch.empty(nseg, dtype=torch.int32, device=d) if pushes else None)

    def compute_stats_records(self, recs: torch.Tensor, rec_off: torch.Tensor,
                              bufs: Optional[_ReportBuffers] = None) -> ops.SegmentStats:
        """recs [n, 2] int32 {slot, ns} of R streams (rec_off [R+1] int64, device): the
        reference's ring pushes (CuptiProfiler.cpp:168-203) + getStats, for every rank."""
        b = self.own if bufs is None else bufs
        self._order_after_inflight()
        n = recs.shape[0]
        # (no per-bucket push counts: a report needs the kept records only)
        b.bucket = self._bucket_scratch(b.bucket, n, pushes=False)
        max_len = min(self.cap, n) if self.cap > 0 else n
        b.clean = False
        return ops.records_stats(recs, rec_off, self.K, self.cap, max(max_len, 1), mode=self.mode,
                                 out=b.stats, bucket=b.bucket,
                                 col_ref=b.col_ref if self.relative else None)

    def report_records(self, recs: torch.Tensor, rec_off: torch.Tensor) -> BatchResult:
        """One full report from record streams resident in HBM."""
        self.compute_stats_records(recs, rec_off)
        self.compute_scores()
        return self.land()

    def _scores(self, b: _ReportBuffers, err: torch.Tensor, **into) -> None:
        """The scores kernel over set b's statistics and reference; into: finalize= (1 GPU) or
        partials= (N GPUs)."""
        K = self.K
        st = b.stats.view(self.R, K)
        # the self-resetting epilogue where the per-kernel reference is fused into the
        # statistics (R <= FUSED_REF_MAX_ROWS): one completion counter per report, whose
        # same-address atomics would cost ~0.15 / 1 ms at 4,096 / 16,384 rows
        fused = self._fuse_ref()
        if not fused:
            err.zero_()
        ops.scores(st.num, st.med, st.avg, col_valid=self.col_valid,
                   ref=b.col_ref.view(torch.float32)[:K] if self.relative else None,
                   ref_missing=b.col_ref[K:2 * K] if self.relative else None,
                   hist=self.hist, err=err, done=b.done if fused else None,
                   reset_col_ref=b.col_ref[:2 * K] if fused else None, **into)
        b.clean = fused

    def compute_scores(self, out_buf: Optional[torch.Tensor] = None,
                       bufs: Optional[_ReportBuffers] = None) -> None:
        """Scores + straggler masks into the packed buffer (one kernel on 1 GPU; partials ->
        RCCL all_gather -> finalize on N GPUs).  out_buf: another packed buffer of the same
        layout (1 GPU), e.g. pinned host memory the kernel writes directly (no copy)."""
        b = self.own if bufs is None else bufs
        self._order_after_inflight()
        if not self.exchange:
            self._scores(b, b.err if out_buf is None else b.err_of(out_buf),
                         finalize=dict(b.views(out_buf), thr_rel=self.thr_rel, thr_ind=self.thr_ind,
                                       round_f32=self.round_f32))
            return
        self._scores_partials(b)
        self._exchange(b)
        self._finalize(b)

    # -- the N-GPU scoring in three phases: per-rank partials of this shard's kernels (HIP), the
    # all_gather of the partials (RCCL / gloo), the combine in shard order (HIP) --
    def _scores_partials(self, bufs: Optional[_ReportBuffers] = None) -> None:
        b = self.own if bufs is None else bufs
        self._scores(b, b.err, partials=b.partials)

    def _exchange(self, bufs: Optional[_ReportBuffers] = None) -> None:
        b = self.own if bufs is None else bufs
        R = self.R
        flat = b.gathered.view(self.world * R, 6)
        if self.gloo:  # gloo collectives take host tensors
            hg = torch.empty((self.world * R, 6), dtype=torch.float64)
            torch.distributed.all_gather_into_tensor(hg, b.partials.cpu(), group=self.group)
            flat.copy_(hg)
        else:          # RCCL over xGMI, device to device
            torch.distributed.all_gather_into_tensor(flat, b.partials, group=self.group)

    def _finalize(self, bufs: Optional[_ReportBuffers] = None) -> None:
        b = self.own if bufs is None else bufs
        ops.finalize_scores(b.gathered, self.R, self.world, self.round_f32, self.thr_rel,
                            self.thr_ind, rel=self.relative, ind=self.individual, err=b.err,
                            out=b.views())

    def _copy_out(self, host: torch.Tensor, bufs: Optional[_ReportBuffers] = None) -> None:
        """The one device-to-host copy of a set's packed results, into a pinned buffer."""
        host.copy_((self.own if bufs is None else bufs).out, non_blocking=True)

    def land(self, bufs: Optional[_ReportBuffers] = None) -> BatchResult:
        """The one device-to-host copy of the packed results, then host views."""
        self._copy_out(self.h_out, bufs)
        _wait(self.device)
        return self.own.unpack(self.h_out)

    def report(self, ns: torch.Tensor, s_push: int) -> BatchResult:
        """One full report: samples resident in HBM -> scores + straggler sets on host."""
        self.compute_stats(ns, s_push)
        self.compute_scores()
        return self.land()

    def histograms(self, ns: torch.Tensor, s_push: int, out: Optional[torch.Tensor] = None,
                   accumulate: bool = False) -> torch.Tensor:
        """Duration histograms of the matrix ``compute_stats`` takes, over the same retained
        windows (the last ``cap`` of ``s_push`` samples per rank and kernel): an int32 device
        tensor [R, K, 240] over the fixed buckets of ``straggler.histograms``.  ``out``: the
        tensor to write, or with ``accumulate=True`` to add this interval's counts to.  The
        buckets are shared, so the sum over ranks (``ops.histogram_sum``) is the world's histogram
        per kernel, and ``tail_scores`` turns the counts into a score per rank.  It reads ``ns`` only and changes none of the report's buffers; the call queues
        behind reports still in flight.  Beyond the reference."""
        self._order_after_inflight()
        R, K = self.R, self.K
        flat = None if out is None else out.view(R * K, histograms.BINS)
        c = ops.segment_histogram_strided(ns.view(-1), R * K, s_push, 0, s_push, cap=self.cap,
                                          out=flat, accumulate=accumulate)
        return c.view(R, K, histograms.BINS)

    def _tail_attr_buffers(self, t: dict, base_len: int) -> int:
        """The packed buffer of a tail-score call with ``attribute > 0``: the call's own packed
        outputs (``base_len`` bytes) followed by the attribution of up to NVRX_MAX_ATTRIBUTION
        kernels per rank, and the dense loss workspace; allocated once per reporter.  Returns the
        attribution's offset."""
        off = (base_len + 7) // 8 * 8
        if t.get("abuf") is None:
            n = self.R * ops.N.NVRX_MAX_ATTRIBUTION
            t["abuf"] = torch.zeros(off + ops.TailAttribution.PACKED * n, dtype=torch.uint8,
                                    device=self.device)
            t["loss_all"] = torch.empty((self.R, self.K), dtype=torch.float64, device=self.device)
        return off

    def tail_scores(self, counts: torch.Tensor, permille: int = 990,
                    threshold: Optional[float] = None, tail_calls: bool = False,
                    attribute: int = 0) -> BatchTailScores:
        """A tail score per rank from the histograms ``histograms()`` returned (int32 device
        tensor [R, K, 240], possibly accumulated over reports): what the median-based scores
        cannot see, a rank that is slow on every n-th call.  The fleet is the sum over ranks, T_k
        the bucket of its ``permille`` quantile per kernel (kernels filtered by ``col_valid`` or
        without samples are skipped), ``w(b)`` a bucket's lower edge in ns, and

            score[r] = (1 - tail_ns[r] / total_ns[r]) / (1 - fleet_tail / fleet_total)

        with ``tail_ns`` the rank's weighted counts above T_k: about 1 for a healthy rank, lower
        for one that spends more of its time in the fleet's tail, on the scale of the GPU scores;
        ``stragglers`` is ``score < threshold`` (None: the reporter's relative threshold).  Exact
        integer sums on the device (include/nvrx_straggler.h).  A slowdown below one bucket
        (12.5 %) may not cross T_k, and ``permille`` must leave more room than the slow rank's own
        share of the fleet's samples (8 ranks, every 10th call slow: use 950, not 990).
        ``tail_calls=True`` also returns, on the device, the int32 [R, K] calls above T_k.
        ``attribute=top`` (1..16) adds ``.attribution``: per rank the `top` kernels with the largest
        excess tail time ``tail - total * fleet_share_k`` in ns (``histograms.tail_attribution``),
        computed on the device and packed into the same device-to-host copy.  It
        queues behind reports in flight and changes none of the report's buffers; its own buffers
        are allocated once per reporter, and the results come in one device-to-host copy.  Beyond
        the reference."""
        pm = ops.tail_permille(permille)
        top = ops.attribution_request(attribute, "relative")[0] if attribute else 0
        self._refuse_exchange("tail_scores")
        R, K = self.R, self.K
        if tuple(counts.shape) != (R, K, histograms.BINS):
            raise ValueError(f"counts must have shape [{R}, {K}, {histograms.BINS}]")
        self._order_after_inflight()
        if self._tail is None:
            self._tail = self._fleet_tail_work()
        return self._fleet_tail_scores(self._tail, _CountsSource(counts), pm, threshold, tail_calls, top)

    def _refuse_exchange(self, method: str) -> None:
        if self.exchange:
            raise NotImplementedError(f"MatrixReporter.{method}: tail scores across kernel shards "
                                      "(exchange=True) are not supported")

    def _tail_work(self, layout, **tensors) -> dict:
        """The work of one tail-score family: its packed-result layout, buffer (zeroed) and the
        layout's views of it (made once: every call without ``attribute`` uses them), the
        ``tail_calls`` matrix (allocated on request) and the family's own tensors."""
        buf = torch.zeros(layout.nbytes, dtype=torch.uint8, device=self.device)
        return dict(layout=layout, buf=buf, views=layout.views(buf), calls=None, **tensors)

    def _fleet_tail_work(self, **more) -> dict:
        """The fleet histogram and packed outputs (``_FleetTailLayout``) of ``tail_scores``; the
        record-stream methods keep a set of their own."""
        return self._tail_work(_FleetTailLayout(self.R, self.K), **more,
                               fleet=torch.empty((self.K, histograms.BINS), dtype=torch.int64,
                                                 device=self.device))

    def _bucket(self, recs: torch.Tensor, rec_off: torch.Tensor, owner: str, pm: int) -> _BucketSource:
        """Bucket the record streams into the tail work tensors of the record-stream methods
        (``_rtail``: what ``tail_scores`` keeps and the bucketing scratch, allocated at first use
        and grown on demand) and return the buckets as a source.  records_bucket writes every
        bucket out (records_stats reduces the tiny ones in LDS and marks them seg_len < 0); the
        windows are already trimmed to ``cap``, their starts padded to 16 bytes.  ``owner`` names
        the path that buckets: a compact call leaves its buckets and permille for
        ``compact_tail_attribution``, which must know later that they are still that call's."""
        if self._rtail is None:
            self._rtail = self._fleet_tail_work(bucket=None, owner=None)
        t = self._rtail
        t["owner"] = owner
        n = recs.shape[0]
        t["bucket"] = self._bucket_scratch(t["bucket"], n, pushes=True)
        seg_off, seg_len, out_ns, _ = ops.records_bucket(recs, rec_off, self.K, self.cap, out=t["bucket"])
        src = _BucketSource(out_ns, seg_off, seg_len, self.K,
                            max(min(self.cap, n) if self.cap > 0 else n, 1))
        if owner == "compact":
            t["compact_call"] = (src, pm)
        return src

    def _tail_call(self, t: dict, top: int, tail_calls: bool):
        """(buf, views, aoff, calls) of one call on the work ``t``: the packed buffer and the
        layout's views of it -- with ``top`` the same layout at the head of a longer buffer, the
        attribution at ``aoff`` -- and what to pass as ``tail_calls=``."""
        buf, views, aoff = t["buf"], t["views"], None
        if top:
            aoff = self._tail_attr_buffers(t, t["layout"].nbytes)
            buf = t["abuf"][:aoff + ops.TailAttribution.PACKED * self.R * top]
            views = t["layout"].views(buf)
        if tail_calls and t["calls"] is None:
            t["calls"] = torch.empty((self.R, self.K), dtype=torch.int32, device=self.device)
        return buf, views, aoff, t["calls"] if tail_calls else False

    def _tail_land(self, t: dict, buf: torch.Tensor, aoff, top: int, res):
        """The one device-to-host copy of a tail-score call, then the layout's results."""
        host = buf.cpu().numpy()  # the one device-to-host transfer (synchronizes)
        attribution = (BatchTailAttribution.unpack(host[aoff:], self.R, top, t["loss_all"])
                       if top else None)
        return t["layout"].unpack(host, res.tail_calls, attribution)

    def _fleet_tail_scores(self, t: dict, src, pm: int, threshold, tail_calls: bool,
                           top: int) -> BatchTailScores:
        """The fleet's tail scores of the interval ``src`` on the work ``t``: fleet histogram ->
        threshold buckets -> scores -> (fleet base -> attribution) -> one copy."""
        buf, (out, thr, sums), aoff, calls = self._tail_call(t, top, tail_calls)
        if top and t.get("base") is None:
            t["base"] = torch.empty((self.K, 2), dtype=torch.int64, device=self.device)
        src.fleet_histogram(t["fleet"])
        ops.histogram_tail_threshold(t["fleet"], pm, col_valid=self.col_valid, thr=thr, fleet_sums=sums)
        res = src.fleet_scores(thr, sums, out=out,
                               score_thr=self.thr_rel if threshold is None else threshold,
                               tail_calls=calls)
        if top:
            ops.histogram_tail_base(t["fleet"], thr, out=t["base"])
            src.fleet_attribution(thr, t["base"], top=top, out=ops.TailAttribution.packed(
                buf[aoff:], self.R, top, t["loss_all"]))
        return self._tail_land(t, buf, aoff, top, res)

    def _history_tail_work(self, clear: bool = True) -> dict:
        """The history and packed outputs (``_HistoryTailLayout``) of the individual tail scores
        (both methods continue the one history), allocated at first use; ``clear=False`` leaves
        the history uninitialised for a caller that overwrites it in full."""
        if self._htail is None:
            new = torch.zeros if clear else torch.empty
            self._htail = self._tail_work(
                _HistoryTailLayout(self.R, folded=False),
                hist=new((self.R, self.K, histograms.BINS), dtype=torch.int32, device=self.device))
        return self._htail

    def tail_scores_records(self, recs: torch.Tensor, rec_off: torch.Tensor, permille: int = 990,
                            threshold: Optional[float] = None, tail_calls: bool = False,
                            attribute: int = 0) -> BatchTailScores:
        """The tail scores of ``tail_scores`` for the record streams ``report_records`` takes
        (recs [n, 2] int32 {slot, ns}, rec_off [R + 1] int64, device), over the windows that
        report retains (the last ``cap`` records of every rank and kernel) -- without the
        [R, K, 240] counts, which for record streams would be several times the records
        themselves.  The streams are bucketed with every bucket written out, then two passes
        over the buckets (``ops.segment_fleet_histogram_ragged``, ``ops.histogram_tail_threshold``,
        ``ops.segment_tail_scores_ragged``) give, bit for bit, what ``tail_scores`` gives on the
        counts of those buckets (``histograms.segment_tail_scores`` on the host).  It queues
        behind reports in flight and touches none of the report's buffers: the bucketing goes
        into work tensors of its own, allocated at first use and grown on demand; the results
        come in one device-to-host copy.  ``attribute=top`` (1..16) adds ``.attribution`` as
        ``tail_scores(attribute=)`` does -- per rank the `top` kernels with the largest excess tail
        time, ``histograms.segment_tail_attribution`` on the host -- again without the counts:
        ``ops.histogram_tail_base`` on the call's fleet, then
        ``ops.segment_tail_attribution_ragged`` on the call's own buckets, packed behind the
        call's outputs in the same device-to-host copy; its buffers are allocated once per
        reporter.  Without it ``.attribution`` stays None.  Beyond the reference."""
        pm = ops.tail_permille(permille)
        top = ops.attribution_request(attribute, "relative")[0] if attribute else 0
        self._refuse_exchange("tail_scores_records")
        if rec_off.numel() != self.R + 1:
            raise ValueError(f"rec_off must hold {self.R + 1} offsets")
        self._order_after_inflight()
        src = self._bucket(recs, rec_off, "relative", pm)
        return self._fleet_tail_scores(self._rtail, src, pm, threshold, tail_calls, top)

    def individual_tail_scores(self, counts: torch.Tensor, permille: int = 990,
                               threshold: Optional[float] = None, absorb: str = "healthy",
                               tail_calls: bool = False, attribute: int = 0,
                               half_life: Optional[int] = None,
                               history: str = "dense") -> BatchIndividualTailScores:
        """A tail score per rank against the rank's OWN history, from the histograms
        ``histograms()`` returned for this interval (int32 device tensor [R, K, 240]): the
        individual leg of ``tail_scores``.  It sees what a comparison with the fleet cannot -- a
        world of one, a degradation that hits every rank together, a large share of the ranks slow
        on every n-th call.  Per (rank, kernel) T is the bucket of the ``permille`` quantile of the
        history (kernels filtered by ``col_valid``, without history or without samples in this
        interval are skipped), ``w(b)`` a bucket's lower edge in ns, and

            score[r] = (1 - tail_ns[r] / total_ns[r]) / (1 - base_tail[r] / base_total[r])

        with ``tail_ns`` / ``base_tail`` the interval's / the history's weighted counts above T:
        about 1 for a rank that behaves as it did, lower for one that spends more of its time above
        its own past's quantile.  ``stragglers`` is ``score < threshold`` (None: the reporter's
        individual threshold).  The first interval has no history: NaN, never flagged.  ``absorb``
        says which intervals join the history (saturating u32 counts): ``"always"`` -- one fused
        score-and-update launch; ``"never"`` -- score only; ``"healthy"`` (default) -- a score
        launch, then an update launch that skips the flagged ranks on the device (no host round
        trip), so a flagged interval does not teach the history that slow is normal.  Exact integer
        sums on the device (include/nvrx_straggler.h).  The reporter owns the history, R * K * 960
        bytes of device memory allocated at first use (``reset_tail_history`` clears it), and the
        packed outputs; the results come in one device-to-host copy, and the call queues behind
        reports in flight and changes none of the report's buffers.  ``tail_calls=True`` also
        returns, on the device, the int32 [R, K] calls above T.  ``attribute=top`` (1..16) adds
        ``.attribution``: per rank the `top` kernels with the largest excess tail time ``tail -
        total * history_share_k`` in ns (``histograms.history_attribution``), packed into the same
        device-to-host copy.  The order on the device is score, attribution, update, so the
        attribution sees the history the score saw: ``absorb="always"`` then runs a score-only
        launch, the attribution and an update-only launch -- by the definition the same bits as the
        fused launch.  ``half_life=N`` (an int >= 1) lets the history forget: the reporter counts
        the calls with ``absorb != "never"`` on the dense history (this method's and
        ``individual_tail_scores_records``'s alike) since its last aging or ``reset_tail_history``,
        and a call that finds N of them first halves every count of the history on its stream
        (``ops.histogram_history_age``, shift 1) and restarts the count: age, score,
        (attribution), update.  An interval then weighs half as much after N absorbing calls, a
        quarter after 2 N.  ``None`` (default): no aging and no further launch.
        ``history="compact"`` scores against, and folds the interval into, the compact history of
        64 bytes per (rank, kernel) in place of 960 -- the SAME one
        ``individual_tail_scores_records(history="compact")`` keeps (``compact_tail_history()``
        returns it; the two compact methods continue one history as the two dense methods do):
        ``ops.histogram_history_scores_compact`` with the same ``absorb`` logic, ``half_life``
        counted on the compact history.  ``.folded`` (u64 [R], in the same device-to-host copy)
        counts the samples folded in this call; while it stays 0 every result equals
        ``history="dense"``'s bit for bit (``histograms.compact_history_scores`` on the host).
        ``attribute`` is not taken together with the compact history (NotImplementedError): ask
        ``compact_tail_attribution(counts=counts)`` after this call, which explains the counts
        against the compact history on request (``ops.histogram_history_attribution_compact``).
        The call does not touch the bucketing work tensors, so a pending
        ``compact_tail_attribution()`` stays valid.  ``history="dense"``
        (default) is the path described above, untouched.  ``convert_tail_history`` moves a
        reporter from one history to the other.  Beyond the reference."""
        pm, top, half_life = self._individual_request(
            "individual_tail_scores", permille, attribute, absorb, half_life, history,
            instead="; call compact_tail_attribution(counts=...) after the scores")
        R, K = self.R, self.K
        if tuple(counts.shape) != (R, K, histograms.BINS):
            raise ValueError(f"counts must have shape [{R}, {K}, {histograms.BINS}]")
        self._order_after_inflight()
        res = self._individual_tail_scores(lambda: _CountsSource(counts), history, pm, threshold,
                                           absorb, tail_calls, top, half_life)
        if history == "compact":
            self._ctail["counts_permille"] = pm  # what compact_tail_attribution(counts=) defaults to
        return res

    def _individual_request(self, method: str, permille, attribute, absorb, half_life, history,
                            instead: str = ""):
        """The request checks both individual tail-score methods start with, in their order;
        returns (permille, top, half_life).  ``instead``: what the refusal of ``attribute`` with the
        compact history points to."""
        pm = ops.tail_permille(permille)
        top = ops.attribution_request(attribute, "individual")[0] if attribute else 0
        if absorb not in ABSORB_MODES:
            raise ValueError(f"absorb must be one of {ABSORB_MODES}, got {absorb!r}")
        half_life = _half_life(half_life)
        if history not in ("dense", "compact"):
            raise ValueError(f"history must be 'dense' or 'compact', got {history!r}")
        self._refuse_exchange(method)
        if history == "compact" and top:
            raise NotImplementedError(f"MatrixReporter.{method}: attribute= is not available with "
                                      f"the compact history{instead}")
        return pm, top, half_life

    def _individual_tail_scores(self, source, history: str, pm: int, threshold, absorb: str,
                                tail_calls: bool, top: int,
                                half_life: Optional[int]) -> BatchIndividualTailScores:
        """The individual tail scores of one interval against the ``history`` ("dense" /
        "compact") the reporter keeps: age -> score -> (attribution) -> update -> one copy.
        ``source()`` gives the interval; it is asked after the age pass, so the bucketing it may
        launch keeps its place.  ``absorb="always"`` is one fused score-and-update launch unless
        ``top`` puts the attribution between the two, where it sees the history the score saw."""
        compact = history == "compact"
        t = self._compact_tail_work() if compact else self._history_tail_work()
        self._age_before(history, half_life, absorb)
        src = source()
        buf, (out, folded), aoff, calls = self._tail_call(t, top, tail_calls)
        hist = t["chist" if compact else "hist"]
        kw = dict(permille=pm, col_valid=self.col_valid, **({"folded": folded} if compact else {}))
        res = src.history_scores(hist, compact, update=absorb == "always" and not top,
                                 score_thr=self.thr_ind if threshold is None else threshold,
                                 tail_calls=calls, out=out, **kw)
        if top:  # (the dense history only: the request checks refuse it with the compact one)
            src.history_attribution(hist, permille=pm, top=top, col_valid=self.col_valid,
                                    out=ops.TailAttribution.packed(buf[aoff:], self.R, top,
                                                                   t["loss_all"]))
        if absorb == "healthy" or (absorb == "always" and top):
            src.history_scores(hist, compact, score=False,
                               skip_rows=out.strag if absorb == "healthy" else None, **kw)
        elif compact and absorb == "never":
            folded.zero_()  # no update: nothing folded
        return self._tail_land(t, buf, aoff, top, res)

    def individual_tail_scores_records(self, recs: torch.Tensor, rec_off: torch.Tensor,
                                       permille: int = 990, threshold: Optional[float] = None,
                                       absorb: str = "healthy", tail_calls: bool = False,
                                       attribute: int = 0, history: str = "dense",
                                       half_life: Optional[int] = None) -> BatchIndividualTailScores:
        """The individual tail scores of ``individual_tail_scores`` for the record streams
        ``report_records`` takes (recs [n, 2] int32 {slot, ns}, rec_off [R + 1] int64, device),
        over the windows that report retains (the last ``cap`` records of every rank and kernel)
        -- without the [R, K, 240] counts of the interval.  The streams are bucketed with every
        bucket written out into the work tensors ``tail_scores_records`` uses, then
        ``ops.segment_history_scores_ragged`` scores the buckets against, and folds them into, the
        SAME history ``individual_tail_scores`` keeps: the two methods continue one history
        (``reset_tail_history`` clears it), and the results are, bit for bit, what
        ``individual_tail_scores`` gives on the histograms of those buckets
        (``histograms.segment_history_scores`` on the host).  A (rank, kernel) without records in
        the interval is not scored and leaves its history as it is.  ``absorb`` as there:
        ``"healthy"`` -- a score launch, then an update launch that skips the flagged ranks on the
        device; ``"always"`` -- one fused launch; ``"never"`` -- score only.  It queues behind
        reports in flight and touches none of the report's buffers; the results come in one
        device-to-host copy.  ``attribute=top`` (1..16) adds ``.attribution`` as
        ``individual_tail_scores(attribute=)`` does -- per rank the `top` kernels with the largest
        excess tail time against the rank's own history, ``histograms.segment_history_attribution``
        on the host -- again without the counts: ``ops.segment_history_attribution_ragged`` on the
        call's own buckets, between the score and the update so that it sees the history the score
        saw (``absorb="always"`` then runs a score-only launch, the attribution and an update-only
        launch), packed behind the call's outputs in the same device-to-host copy.  Without it
        ``.attribution`` stays None and the launches are what they were.
        ``history="compact"`` scores against, and folds the interval into, a SEPARATE compact
        history of 64 bytes per (rank, kernel) in place of 960 (uint8 [R, K, 64], allocated at
        first use; ``compact_tail_history()`` returns it, ``reset_tail_history`` clears both):
        ``ops.segment_history_scores_compact_ragged`` with the same ``absorb`` logic.  An element
        keeps at most 12 used buckets and folds what does not fit into the nearest kept bucket
        below; ``.folded`` (u64 [R], in the same device-to-host copy) counts the samples folded in
        this call, and while it stays 0 every result equals ``history="dense"``'s bit for bit
        (``histograms.segment_compact_history_scores`` on the host).  ``attribute`` is not
        taken together with the compact history (NotImplementedError): ask
        ``compact_tail_attribution()`` after this call, which explains it on request.
        ``history="dense"`` (default) is the path described above, untouched.
        ``half_life=N`` (an int >= 1) as in ``individual_tail_scores``, per history: a call that
        finds N calls with ``absorb != "never"`` on ITS history since that history's last aging or
        ``reset_tail_history`` first halves the history's counts on its stream
        (``ops.histogram_history_age`` / ``ops.compact_history_age``, shift 1, without the row
        outputs) and restarts the count: age, score, (attribution), update.  In the compact
        history the entries that reach zero are evicted, so a full element admits new buckets
        again and ``.folded`` returns to 0.  ``None`` (default): no aging and no further launch.
        Beyond the reference."""
        pm, top, half_life = self._individual_request(
            "individual_tail_scores_records", permille, attribute, absorb, half_life, history,
            instead="; call compact_tail_attribution() after the scores")
        if rec_off.numel() != self.R + 1:
            raise ValueError(f"rec_off must hold {self.R + 1} offsets")
        self._order_after_inflight()
        return self._individual_tail_scores(lambda: self._bucket(recs, rec_off, history, pm), history,
                                            pm, threshold, absorb, tail_calls, top, half_life)

    def _compact_tail_work(self, clear: bool = True) -> dict:
        """The compact history and packed outputs (``_HistoryTailLayout`` with ``folded``) of the
        two compact methods (they continue the one history), allocated at first use;
        ``clear=False`` leaves the history uninitialised for a caller that overwrites it in full."""
        if self._ctail is None:
            new = torch.zeros if clear else torch.empty
            self._ctail = self._tail_work(
                _HistoryTailLayout(self.R, folded=True),
                chist=new((self.R, self.K, histograms.CHIST_BYTES), dtype=torch.uint8,
                          device=self.device))
        return self._ctail

    def compact_tail_history(self) -> Optional[torch.Tensor]:
        """The compact history of ``individual_tail_scores_records(history="compact")`` (uint8
        [R, K, 64] on the device; ``histograms.compact_to_dense`` expands a host copy), or None
        before its first use."""
        return None if self._ctail is None else self._ctail["chist"]

    def compact_tail_attribution(self, top: int = 8, *, permille: Optional[int] = None,
                                 counts: Optional[torch.Tensor] = None) -> BatchTailAttribution:
        """The kernels behind the individual tail scores against the compact history, on request
        (as ``attribute()`` explains the last report): per rank the `top` (1..16) kernels with the
        largest excess tail time ``tail - total * history_share_k`` in ns, for the buckets the
        reporter's last ``individual_tail_scores_records(history="compact")`` call laid out,
        against the compact history AS IT STANDS when this method runs
        (``ops.segment_history_attribution_compact_ragged``;
        ``histograms.segment_compact_history_attribution`` on the host).  ``permille=None`` means
        that call's permille.  For every rank that call did not absorb -- the flagged ranks under
        the default ``absorb="healthy"``, every rank under ``"never"``: the ranks one asks about --
        this is the history the score saw, and the result equals, bit for bit, what
        ``individual_tail_scores_records(attribute=top)`` gives against the dense history while
        nothing was folded.  For a rank the call absorbed (healthy ranks under ``"healthy"``, every
        rank under ``"always"``) it is the UPDATED history, the interval included.  The method
        does not bucket again, touches no report buffer and leaves the history bit-identical; it
        queues behind reports in flight, and the results come in one device-to-host copy
        (``loss_all`` stays on the device).  RuntimeError if no compact record-stream call has run,
        or if another record-stream method has re-used the bucketing work tensors since.
        ``counts=`` (int32 device tensor [R, K, 240], the histograms ``histograms()`` returned)
        explains THOSE counts in place of the last record-stream call's buckets, against the
        compact history as it stands (``ops.histogram_history_attribution_compact``;
        ``histograms.compact_history_attribution`` on the host): the way to name the kernels behind
        ``individual_tail_scores(counts, history="compact")``, equal bit for bit to
        ``individual_tail_scores(counts, attribute=top)`` against the dense history for every rank
        that call did not absorb, while nothing was folded.  It neither needs nor touches the
        bucketing work tensors, so a pending record-stream ``compact_tail_attribution()`` stays
        valid across it.  ``permille=None`` then means the permille of the reporter's last
        ``individual_tail_scores(history="compact")`` call.  ValueError for a wrong shape;
        RuntimeError if the reporter has no compact history yet, or if ``permille`` is None and no
        such call has run.  Beyond the reference."""
        top, _ = ops.attribution_request(top, "individual")
        self._refuse_exchange("compact_tail_attribution")
        if counts is not None:
            return self._compact_counts_attribution(counts, top, permille)
        w, t = self._rtail, self._ctail
        if t is None or w is None or w.get("compact_call") is None:
            raise RuntimeError("MatrixReporter.compact_tail_attribution: no "
                               "individual_tail_scores_records(history=\"compact\") call to explain")
        if w["owner"] != "compact":
            raise RuntimeError("MatrixReporter.compact_tail_attribution: another record-stream "
                               "method has re-used the buckets of the last compact call")
        src, pm = w["compact_call"]
        if permille is not None:
            pm = ops.tail_permille(permille)
        R = self.R
        self._order_after_inflight()
        aoff = self._tail_attr_buffers(t, 0)
        buf = t["abuf"][aoff:aoff + ops.TailAttribution.PACKED * R * top]
        src.compact_history_attribution(
            t["chist"], permille=pm, top=top, col_valid=self.col_valid,
            out=ops.TailAttribution.packed(buf, R, top, t["loss_all"]))
        host = buf.cpu().numpy()  # the one device-to-host transfer (synchronizes)
        return BatchTailAttribution.unpack(host, R, top, t["loss_all"])

    def _compact_counts_attribution(self, counts: torch.Tensor, top: int,
                                    permille: Optional[int]) -> BatchTailAttribution:
        """``compact_tail_attribution(counts=)``: shape check -> the compact history must exist ->
        behind the reports in flight -> the entry into the packed buffer -> one copy."""
        R, K = self.R, self.K
        if tuple(counts.shape) != (R, K, histograms.BINS):
            raise ValueError(f"counts must have shape [{R}, {K}, {histograms.BINS}]")
        t = self._ctail
        if t is None:
            raise RuntimeError("MatrixReporter.compact_tail_attribution: the reporter has no "
                               "compact history to explain the counts against")
        pm = t.get("counts_permille") if permille is None else ops.tail_permille(permille)
        if pm is None:
            raise RuntimeError("MatrixReporter.compact_tail_attribution: permille=None and no "
                               "individual_tail_scores(history=\"compact\") call to take it from")
        self._order_after_inflight()
        aoff = self._tail_attr_buffers(t, 0)
        buf = t["abuf"][aoff:aoff + ops.TailAttribution.PACKED * R * top]
        _CountsSource(counts).compact_history_attribution(
            t["chist"], permille=pm, top=top, col_valid=self.col_valid,
            out=ops.TailAttribution.packed(buf, R, top, t["loss_all"]))
        host = buf.cpu().numpy()  # the one device-to-host transfer (synchronizes)
        return BatchTailAttribution.unpack(host, R, top, t["loss_all"])

    def kernel_ranks(self, loss_all: torch.Tensor, top: int = 8, flagged=None) -> BatchKernelRanks:
        """The ranks behind a kernel's tail loss, the converse of ``attribute=``: per kernel the
        `top` (1..16) ranks with the largest excess tail time in ``loss_all``, how many ranks are
        taken and how many of them lose time on the kernel at all (loss > 0).  ``loss_all`` is the
        float64 [R, K] device tensor of any ``...attribution.loss_all`` of this reporter
        (``tail_scores``, ``individual_tail_scores``, the record-stream methods,
        ``compact_tail_attribution``), or any other such tensor; NaN means not taken.  That tensor
        is the reporter's WORKSPACE: the next ``attribute=`` call of the same family overwrites
        it, so ask before that call.  ``flagged`` (bool / uint8 [R], a numpy array or a tensor,
        e.g. a result's ``stragglers``) restricts the ranking to those ranks.  Ties go to the
        lower rank, -0.0 and +0.0 tie, and ``loss_ns`` holds the matrix's own bits
        (``ops.rank_attribution``: the matrix is read once on the device, never copied to the
        host; ``histograms.rank_attribution`` is the host twin).  It queues behind reports in
        flight and touches none of the report's buffers; its outputs and work space are allocated
        once per reporter and `top`, and the results come in one device-to-host copy.  ValueError
        for a wrong shape, dtype or device, before anything is allocated or launched.  It does
        not look at ``exchange``: the matrix is whatever the caller holds.  Beyond the
        reference."""
        top, _ = ops.attribution_request(top, "relative")
        R, K = self.R, self.K
        if not isinstance(loss_all, torch.Tensor) or not loss_all.is_cuda or \
                (self.device.index is not None and loss_all.device != self.device):
            raise ValueError("loss_all must be a tensor on the reporter's device")
        if loss_all.dtype != torch.float64 or tuple(loss_all.shape) != (R, K):
            raise ValueError(f"loss_all must be a float64 tensor of shape [{R}, {K}]")
        ops._rank_loss(loss_all)
        rows = _flagged_rows(flagged, R, loss_all.device)
        d = loss_all.device
        t = self._kranks.get(top)
        if t is None:
            need = ops.rank_attribution_plan(R, K, top)[2]
            t = self._kranks[top] = dict(
                buf=torch.zeros(ops.RankAttribution.nbytes(K, top), dtype=torch.uint8, device=d),
                work=torch.empty(need, dtype=torch.uint8, device=d) if need else None,
                rows=torch.empty(R, dtype=torch.uint8, device=d))
        self._order_after_inflight()
        rows = _rows_on_device(rows, t["rows"])
        ops.rank_attribution(loss_all, top, rows=rows, out=ops.RankAttribution.packed(t["buf"], K, top),
                             work=t["work"])
        host = t["buf"].cpu().numpy()  # the one device-to-host transfer (synchronizes)
        return BatchKernelRanks(*ops.RankAttribution.unpack(host, K, top))

    def convert_tail_history(self, to: str) -> Optional[np.ndarray]:
        """Move the reporter from one history of the individual tail scores to the other, on the
        device: ``to="compact"`` converts the dense history into the compact one
        (``ops.compact_history_from_dense``: per element the 12 lowest used buckets, the rest
        folded into the 12th), ``to="dense"`` expands the compact history
        (``ops.compact_history_to_dense``).  The target is allocated if needed and overwritten in
        full; the source is released, so its memory (960 bytes per rank and kernel for the dense
        history) goes back to the allocator, and the source's ``half_life=`` count moves to the
        target.  The calls that follow continue with ``history=to``.  It queues behind reports in
        flight.  Returns for ``"compact"`` the samples folded per rank (u64 [R], one
        device-to-host copy; all zero when no element used more than 12 buckets, and then the
        scores that follow equal the dense history's bit for bit), for ``"dense"`` None (nothing
        synchronizes).  A pending ``compact_tail_attribution()`` does not survive
        ``to="dense"``.  RuntimeError if the source history was never allocated.  Beyond the
        reference."""
        if to not in ("compact", "dense"):
            raise ValueError(f"to must be 'compact' or 'dense', got {to!r}")
        self._refuse_exchange("convert_tail_history")
        src = self._htail if to == "compact" else self._ctail
        if src is None:
            raise RuntimeError(f"MatrixReporter.convert_tail_history: no "
                               f"{'dense' if to == 'compact' else 'compact'} history to convert")
        self._order_after_inflight()
        if to == "compact":  # (the target uninitialised: either conversion writes all of it)
            t = self._compact_tail_work(clear=False)
            folded = t["views"][1]
            ops.compact_history_from_dense(src["hist"], out=t["chist"], folded=folded)
            host = folded.cpu().numpy().view(np.uint64).copy()  # the one device-to-host transfer
            self._htail = None
            self._absorbed = {"dense": 0, "compact": self._absorbed["dense"]}
            return host
        ops.compact_history_to_dense(src["chist"], out=self._history_tail_work(clear=False)["hist"])
        self._ctail = None
        self._absorbed = {"dense": self._absorbed["compact"], "compact": 0}
        return None

    def reset_tail_history(self) -> None:
        """Forget the histories of ``individual_tail_scores`` (dense and compact): the next
        interval scores NaN."""
        if self._htail is not None or self._ctail is not None:
            self._order_after_inflight()
        if self._htail is not None:
            self._htail["hist"].zero_()
        if self._ctail is not None:
            self._ctail["chist"].zero_()
        self._absorbed = {"dense": 0, "compact": 0}

    def _age_before(self, kind: str, half_life: Optional[int], absorb: str) -> None:
        """``half_life=`` at the start of a call on history ``kind`` (allocated by now): the age
        pass on the current stream when ``half_life`` absorbing calls have been counted, then this
        call's own count."""
        if half_life is not None and self._absorbed[kind] >= half_life:
            if kind == "dense":
                ops.histogram_history_age(self._htail["hist"], 1)
            else:  # the row outputs stay NULL: the packed buffers keep their layout
                ops.compact_history_age(self._ctail["chist"], 1, counts=False)
            self._absorbed[kind] = 0
        if absorb != "never":
            self._absorbed[kind] += 1

    def age_tail_history(self, shift: int = 1, history: str = "both") -> TailHistoryAging:
        """Let the histories of the individual tail scores forget: every count of the dense
        history (``history="dense"``), of the compact history (``"compact"``) or of whichever of
        the two the reporter has (``"both"``, default) becomes ``count >> shift`` (``shift`` in
        1..31; halved for 1), on the device (``ops.histogram_history_age``,
        ``ops.compact_history_age``; ``histograms.history_age`` / ``compact_age`` on the host).  In
        the compact history the entries that reach zero are evicted and the elements re-packed, so
        an element stuck with 12 stale buckets admits new ones again.  Where no element ever
        folded the two histories stay bit-identical through aging.  It queues behind reports in
        flight; a history that was never allocated is skipped, not allocated.  Returns
        ``TailHistoryAging``: for the compact history ``evicted`` / ``full`` (u64 [R]: the entries
        freed per rank, the elements per rank still holding 12 entries), in one device-to-host
        copy; both None when no compact history was aged (then nothing synchronizes).  The
        ``half_life=`` counts of the aged histories restart.  Beyond the reference."""
        s = ops.age_shift(shift)
        if history not in HISTORY_KINDS:
            raise ValueError(f"history must be one of {HISTORY_KINDS}, got {history!r}")
        self._refuse_exchange("age_tail_history")
        dense = self._htail if history in ("dense", "both") else None
        compact = self._ctail if history in ("compact", "both") else None
        if dense is None and compact is None:
            return TailHistoryAging()
        self._order_after_inflight()
        if dense is not None:
            ops.histogram_history_age(dense["hist"], s)
            self._absorbed["dense"] = 0
        if compact is None:
            return TailHistoryAging()
        R = self.R
        if compact.get("age") is None:  # [evicted i64 R][full i64 R]
            compact["age"] = torch.zeros(2 * R, dtype=torch.int64, device=self.device)
        out = compact["age"]
        ops.compact_history_age(compact["chist"], s, evicted=out[:R], full=out[R:])
        self._absorbed["compact"] = 0
        host = out.cpu().numpy().view(np.uint64)  # the one device-to-host transfer (synchronizes)
        return TailHistoryAging(host[:R].copy(), host[R:].copy())

    def attribute(self, top: int = 8, kind: str = "relative") -> BatchAttribution:
        """Which kernels made each rank's score what it is: per rank the `top` (1..16) kernels
        with the largest loss ``NUM*AVG * (1 - base/MED)``, base being the per-kernel reference
        (kind="relative") or the rank's own history (kind="individual"); the losses of all of a
        rank's kernels sum to ``(1 - score) * wsum``.  It explains the statistics in the reporter's
        own buffer set -- the last report(), report_records() or own-set graph replay -- and
        changes none of the report's buffers.  Beyond the reference (it reports the score only)."""
        top, _ = ops.attribution_request(top, kind)
        if self.exchange:
            raise NotImplementedError("MatrixReporter.attribute: attribution across kernel shards "
                                      "(exchange=True) is not supported")
        if not (self.relative if kind == "relative" else self.individual):
            raise RuntimeError(f"MatrixReporter.attribute: the reporter was built without "
                               f"{kind} scores")
        self._order_after_inflight()
        R, K, d = self.R, self.K, self.device
        st = self.own.stats.view(R, K)
        n = R * top
        buf = self._attr_out.get(top)
        if buf is None:  # packed: [loss f64 n][score f64 n][wsum f64 R][idx i32 n][err i32]
            buf = self._attr_out[top] = torch.zeros(8 * (2 * n + R) + 4 * (n + 1),
                                                    dtype=torch.uint8, device=d)
        f64, i32 = buf[:8 * (2 * n + R)].view(torch.float64), buf[8 * (2 * n + R):].view(torch.int32)
        out = ops.ScoreAttribution(i32[:n], f64[:n], f64[n:2 * n], f64[2 * n:])
        err = i32[n:]
        err.zero_()
        ref = None
        if kind == "relative":
            # the report's scores epilogue has reset col_ref by now: the reference is recomputed
            # into buffers of attribute's own, the same way for every R
            if self._attr_ref is None:
                self._attr_ref = (torch.empty(max(K, 1), dtype=torch.float32, device=d),
                                  torch.empty(2 * max(K, 1), dtype=torch.int32, device=d))
            ref = ops.kernel_ref(st.num, st.med, ref=self._attr_ref[0], scratch=self._attr_ref[1])
        ops.score_attribution(st.num, st.med, st.avg, top=top, kind=kind, col_valid=self.col_valid,
                              ref=ref, hist=self.hist if kind == "individual" else None, err=err,
                              out=out)
        host = buf.cpu().numpy()  # the one device-to-host transfer (synchronizes)
        h64 = host[:8 * (2 * n + R)].view(np.float64)
        h32 = host[8 * (2 * n + R):].view(np.int32)
        loss, wsum = h64[:n].reshape(R, top).copy(), h64[2 * n:].copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            share = loss / wsum[:, None]
        return BatchAttribution(h32[:n].reshape(R, top).copy(), loss,
                                h64[n:2 * n].reshape(R, top).copy(), share, wsum, int(h32[n]))

    def score_kernel_ranks(self, top: int = 8, kind: str = "relative",
                           flagged=None) -> BatchScoreKernelRanks:
        """The ranks behind a kernel's score loss, the converse of ``attribute``: per kernel the
        `top` (1..16) ranks with the largest loss ``NUM*AVG * (1 - base/MED)``, how many ranks are
        scored on the kernel and how many of them lose on it at all (loss > 0) -- one bad
        collective on one node, or many unrelated kernels?  It explains the statistics in the
        reporter's own buffer set, exactly as ``attribute`` does (relative: the reference is
        recomputed into ``attribute``'s buffers; individual: the history is read, never written),
        and changes none of the report's buffers.  ``flagged`` (bool / uint8 [R], a numpy array or
        a tensor, e.g. a result's ``stragglers_relative``) restricts the ranking to those ranks.
        Ties go to the lower rank, -0.0 and +0.0 tie (``ops.score_rank_attribution``: the [R, K]
        loss matrix is never built; ``histograms.score_rank_attribution`` is the host twin).  It
        queues behind reports in flight; its outputs and work space are allocated once per
        reporter and `top`, and the results come in one device-to-host copy.  ValueError /
        RuntimeError before anything is allocated or launched.  Beyond the reference."""
        top, _ = ops.attribution_request(top, kind)
        if self.exchange:
            raise NotImplementedError("MatrixReporter.score_kernel_ranks: attribution across "
                                      "kernel shards (exchange=True) is not supported")
        if not (self.relative if kind == "relative" else self.individual):
            raise RuntimeError(f"MatrixReporter.score_kernel_ranks: the reporter was built without "
                               f"{kind} scores")
        R, K, d = self.R, self.K, self.device
        rows = _flagged_rows(flagged, R, self.own.stats.num.device)
        t = self._sranks.get(top)
        if t is None:  # packed outputs, then the error word
            need = ops.rank_attribution_plan(R, K, top)[2]
            nb = ops.ScoreRankAttribution.nbytes(K, top)
            t = self._sranks[top] = dict(
                buf=torch.zeros(nb + 8, dtype=torch.uint8, device=d),
                work=torch.empty(need, dtype=torch.uint8, device=d) if need else None,
                rows=torch.empty(R, dtype=torch.uint8, device=d))
        self._order_after_inflight()
        st = self.own.stats.view(R, K)
        nb = ops.ScoreRankAttribution.nbytes(K, top)
        err = t["buf"][nb:nb + 4].view(torch.int32)
        err.zero_()
        rows = _rows_on_device(rows, t["rows"])
        ref = None
        if kind == "relative":
            if self._attr_ref is None:
                self._attr_ref = (torch.empty(max(K, 1), dtype=torch.float32, device=d),
                                  torch.empty(2 * max(K, 1), dtype=torch.int32, device=d))
            ref = ops.kernel_ref(st.num, st.med, ref=self._attr_ref[0], scratch=self._attr_ref[1])
        ops.score_rank_attribution(st.num, st.med, st.avg, top=top, kind=kind,
                                   col_valid=self.col_valid, ref=ref,
                                   hist=self.hist if kind == "individual" else None, rows=rows,
                                   err=err, out=ops.ScoreRankAttribution.packed(t["buf"][:nb], K, top),
                                   work=t["work"])
        host = t["buf"].cpu().numpy()  # the one device-to-host transfer (synchronizes)
        return BatchScoreKernelRanks(*ops.ScoreRankAttribution.unpack(host[:nb], K, top),
                                     int(host[nb:nb + 4].view(np.int32)[0]))

    def graph(self, ns: torch.Tensor, s_push: int) -> "ReportGraph":
        """The report's device work captured once as HIP graphs, replayed per report (the
        launch sequence -- reference init, stats, scores, result copy -- costs one graph
        launch instead of one host launch per operation).  1 GPU, or the stats phase only
        on N GPUs (the partials exchange stays an eager collective)."""
        from .report_graphs import ReportGraph
        return ReportGraph(self, ns, s_push)

    def graph_records(self, recs: torch.Tensor, rec_off: torch.Tensor) -> "ReportGraph":
        """graph() over record streams resident in HBM (compute_stats_records captured)."""
        from .report_graphs import ReportGraph
        return ReportGraph(self, None, 0, stats=lambda bufs: self.compute_stats_records(
            recs, rec_off, bufs=bufs))

    def pipelined(self, ns, s_push: int, timing: bool = False,
                  mode: Optional[str] = None, depth: int = 2,
                  timing_reps: int = 1) -> "PipelinedReports":
        """Reports replayed two deep: report i+1's device work is queued before report i's
        results are read on the host, each report landing in its own pinned buffer (N GPUs: the
        partials exchange of each report stays an eager collective, issued in report order).
        ns: one input matrix, or a list of them (report i reads ns[i % len(ns)]; len(ns) divides
        depth) -- e.g. a fresh matrix per report in flight.  An input must not be modified while
        a report that reads it is in flight: collect() raises if a torch in-place operation
        changed it (its version counter moved) between that report's submit() and collect()."""
        from .report_graphs import PipelinedReports
        ins = list(ns) if isinstance(ns, (list, tuple)) else [ns]
        return PipelinedReports(
            self, [lambda bufs, x=x: self.compute_stats(x, s_push, bufs=bufs) for x in ins],
            inputs=[(x,) for x in ins], stats_bytes=self._matrix_bytes(s_push), timing=timing,
            mode=mode, depth=depth, timing_reps=timing_reps)

    def _matrix_bytes(self, s_push: int) -> int:
        keep = min(s_push, self.cap) if self.cap > 0 else s_push
        return 4 * self.R * self.K * keep  # 4 B per retained sample

    def pipelined_records(self, recs, rec_off: torch.Tensor, timing: bool = False,
                          mode: Optional[str] = None, depth: int = 2,
                          timing_reps: int = 1) -> "PipelinedReports":
        """pipelined() over record streams resident in HBM (compute_stats_records: bucketing,
        classification and the class kernels -- side-stream fork / join and stream-ordered
        scratch included -- captured into the report graphs).  recs: one record tensor or a list
        of them (same layout, rec_off shared), as ns for pipelined()."""
        from .report_graphs import PipelinedReports
        ins = list(recs) if isinstance(recs, (list, tuple)) else [recs]
        return PipelinedReports(
            self, [lambda bufs, r=r: self.compute_stats_records(r, rec_off, bufs=bufs) for r in ins],
            inputs=[(r, rec_off) for r in ins], stats_bytes=8 * ins[0].shape[0], timing=timing,
            mode=mode, depth=depth, timing_reps=timing_reps)

