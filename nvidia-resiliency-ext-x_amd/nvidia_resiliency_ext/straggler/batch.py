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

import os
import time
import weakref
from dataclasses import dataclass
from functools import partial
from typing import Optional

import numpy as np
import torch

from . import histograms, ops


# The per-kernel reference (min over ranks of MED) is fused into the stats epilogue as one
# global atomicMin per segment.  Those atomics serialise per column: with R rows every
# column address takes R of them, which costs more than a separate column reduction
# (kernel_ref: 64 rows per thread, R/64 atomics per column) once R is in the hundreds
# (measured on MI355X: 885k segments on 54 columns, 0.6 ms -> 4.3 ms fused).
FUSED_REF_MAX_ROWS = 256


# How the host waits for a report's results (they land in pinned host memory):
#   "bounded" (default) -- poll the completion event for at most SPIN_BOUND_US, then block in
#       hipEventSynchronize on a blocking-sync event: a report that lands within the bound
#       skips the driver's wake-up latency, a longer one does not hold a host core (in a
#       training process that calls this API every core belongs to the job; the reference's
#       report path blocks too, straggler.py:234-235, CuptiProfiler.cpp:136-146);
#   "spin" -- poll until done (bench.py: the wake-up latency is part of every timed report);
#   "block" -- block at once.
# NVRX_SYNC selects the mode per process; set_sync_mode() changes it at run time.
SYNC_MODES = ("bounded", "spin", "block")
SPIN_BOUND_US = float(os.environ.get("NVRX_SPIN_US", "50"))
_sync_mode = os.environ.get("NVRX_SYNC", "") or "bounded"
if _sync_mode not in SYNC_MODES:
    raise ValueError(f"NVRX_SYNC={_sync_mode!r}: one of {SYNC_MODES}")


def set_sync_mode(mode: str) -> str:
    """Select how report results are waited for (SYNC_MODES); returns the previous mode."""
    global _sync_mode
    if mode not in SYNC_MODES:
        raise ValueError(f"sync mode {mode!r}: one of {SYNC_MODES}")
    prev, _sync_mode = _sync_mode, mode
    return prev


def sync_mode() -> str:
    return _sync_mode


def wait_event(ev, mode: Optional[str] = None, bound_us: Optional[float] = None) -> None:
    """Wait until a recorded event has completed, in the current (or the given) sync mode.
    `ev` needs query() and synchronize(); the blocking fallback blocks only if the event was
    created with blocking=True (every event this module waits on is)."""
    mode = mode or _sync_mode
    if mode == "block":
        ev.synchronize()
        return
    if mode == "spin":
        while not ev.query():
            pass
        return
    bound = SPIN_BOUND_US if bound_us is None else bound_us
    deadline = time.perf_counter_ns() + int(bound * 1e3)
    while not ev.query():
        if time.perf_counter_ns() >= deadline:
            ev.synchronize()
            return


def _wait(device) -> None:
    """Wait for the device's current stream (wait_event on an event recorded on it)."""
    ev = torch.cuda.Event(blocking=True)
    ev.record(torch.cuda.current_stream(device))
    wait_event(ev)


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

    def compute_stats_records(self, recs: torch.Tensor, rec_off: torch.Tensor,
                              bufs: Optional[_ReportBuffers] = None) -> ops.SegmentStats:
        """recs [n, 2] int32 {slot, ns} of R streams (rec_off [R+1] int64, device): the
        reference's ring pushes (CuptiProfiler.cpp:168-203) + getStats, for every rank."""
        b = self.own if bufs is None else bufs
        self._order_after_inflight()
        n = recs.shape[0]
        need = ops.records_bucket_capacity(n, self.R, self.K)
        if b.bucket is None or b.bucket[2].numel() < need:
            d = self.device
            # (no per-bucket push counts: a report needs the kept records only)
            b.bucket = (torch.empty(self.R * self.K, dtype=torch.int64, device=d),
                        torch.empty(self.R * self.K, dtype=torch.int32, device=d),
                        torch.empty(max(need, 1), dtype=torch.int32, device=d), None)
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
        buckets are shared, so ``out.sum(0, dtype=torch.int64)`` is the world's histogram per
        kernel.  It reads ``ns`` only and changes none of the report's buffers; the call queues
        behind reports still in flight.  Beyond the reference."""
        self._order_after_inflight()
        R, K = self.R, self.K
        flat = None if out is None else out.view(R * K, histograms.BINS)
        c = ops.segment_histogram_strided(ns.view(-1), R * K, s_push, 0, s_push, cap=self.cap,
                                          out=flat, accumulate=accumulate)
        return c.view(R, K, histograms.BINS)

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

    def graph(self, ns: torch.Tensor, s_push: int) -> "ReportGraph":
        """The report's device work captured once as HIP graphs, replayed per report (the
        launch sequence -- reference init, stats, scores, result copy -- costs one graph
        launch instead of one host launch per operation).  1 GPU, or the stats phase only
        on N GPUs (the partials exchange stays an eager collective)."""
        return ReportGraph(self, ns, s_push)

    def graph_records(self, recs: torch.Tensor, rec_off: torch.Tensor) -> "ReportGraph":
        """graph() over record streams resident in HBM (compute_stats_records captured)."""
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
        ins = list(recs) if isinstance(recs, (list, tuple)) else [recs]
        return PipelinedReports(
            self, [lambda bufs, r=r: self.compute_stats_records(r, rec_off, bufs=bufs) for r in ins],
            inputs=[(r, rec_off) for r in ins], stats_bytes=8 * ins[0].shape[0], timing=timing,
            mode=mode, depth=depth, timing_reps=timing_reps)


class ReportGraph:
    """HIP graphs over a MatrixReporter's fixed buffers.  1 GPU: ``full`` is the whole
    report (column-reference init, segment statistics, scores + straggler masks, the
    device-to-host copy of the packed results) and is what ``run()`` replays; the same work
    is also captured as two halves, ``stats`` and ``rest``, for callers that record timing
    events between them (``run_stats()`` + ``run_rest()``).  One graph instead of two saves
    ~12 us per configs[1] report on MI355X (0.685 -> 0.673 ms, tools/ab_report_overhead.py).
    N GPUs: ``stats`` only; the partials exchange stays an eager collective."""

    def __init__(self, rep: MatrixReporter, ns: Optional[torch.Tensor], s_push: int, stats=None):
        self.rep = rep
        own = rep.own  # the graphs run over the reporter's own buffer set
        if stats is None:  # the statistics phase (record streams: MatrixReporter.graph_records)
            stats = lambda bufs: rep.compute_stats(ns, s_push, bufs=bufs)  # noqa: E731
        _warm_up(rep, stats)
        # the captured statistics phase trusts col_ref as the previous report's scores epilogue
        # left it (colref_ready at capture): replays must pair it with the scores (run_rest),
        # which run_stats checks against the reporter's flag -- kept current by every replay
        self._needs_clean = own.clean
        stats, copy_out = partial(stats, own), partial(rep._copy_out, rep.h_out)
        self.stats = _capture(stats)
        self.rest = self.full = None
        if rep.exchange:
            # N GPUs: the shard's partials and the combine (+ the result copy) as graphs too;
            # only the all_gather of the partials between them runs eagerly
            self.partials = _capture(rep._scores_partials)
            self.finalize = _capture(rep._finalize, copy_out)
        else:
            self.rest = _capture(rep.compute_scores, copy_out)
            self.full = _capture(stats, rep.compute_scores, copy_out)

    def _check_clean(self) -> None:
        if self._needs_clean and not self.rep.own.clean:
            raise RuntimeError("ReportGraph: the statistics graph was captured to follow a scores "
                               "phase (its epilogue re-initialises the column reference); the last "
                               "statistics phase was not followed by run_rest()")

    def _finish(self) -> BatchResult:
        """After the scores were replayed: the flag, the wait, the host views."""
        rep = self.rep
        rep.own.clean = rep._fuse_ref()
        _wait(rep.device)
        return rep.own.unpack(rep.h_out)

    def run_stats(self) -> None:
        self._check_clean()
        self.rep._order_after_inflight()
        self.stats.replay()
        self.rep.own.clean = False

    def run_rest(self) -> BatchResult:
        rep = self.rep
        rep._order_after_inflight()
        if self.rest is None:  # N GPUs: partials graph, eager all_gather, combine graph
            self.partials.replay()
            rep._exchange()
            self.finalize.replay()
        else:
            self.rest.replay()
        return self._finish()

    def run(self) -> BatchResult:
        if self.full is None:
            self.run_stats()
            return self.run_rest()
        self._check_clean()
        self.rep._order_after_inflight()
        self.full.replay()
        return self._finish()


def _capture(*phases) -> torch.cuda.CUDAGraph:
    """The phases (callables), run in order on the current stream, captured as one HIP graph."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for phase in phases:
            phase()
    return g


def _warm_up(rep: MatrixReporter, stats, bufs: Optional[_ReportBuffers] = None) -> None:
    """One eager report over a buffer set (None: the reporter's own) on a side stream
    (first-launch setup outside any graph capture); stats(bufs) runs the statistics phase.  The
    individual history is restored afterwards: the warm-up must not fold whatever the inputs hold
    now into it (the graphs' reports advance it exactly as report() does)."""
    d = rep.device
    b = rep.own if bufs is None else bufs
    rep._order_after_inflight()
    saved = rep.hist.clone() if rep.hist is not None else None
    side = torch.cuda.Stream(d)
    side.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(side):
        stats(b)
        if not rep.exchange:
            rep.compute_scores(bufs=b)
        elif rep._fuse_ref():  # N GPUs: leave col_ref initialised without the exchange
            b.col_ref[:rep.K].fill_(0x7F800000)
            b.col_ref[rep.K:2 * rep.K].zero_()
            b.clean = True
        if saved is not None:
            rep.hist.copy_(saved)
    torch.cuda.current_stream(d).wait_stream(side)
    torch.cuda.synchronize(d)


# NVRX_PIPE_MODE (timing A/B; PipelinedReports(mode=...) overrides the default, "auto"): "alt" each
# report on its own stream of two; "side" the statistics phases on one stream, the rest of every
# report on another; "whole" one whole-report graph per report on the caller's stream (round 4)
_PIPE_MODE = os.environ.get("NVRX_PIPE_MODE", "")
# "auto": alt while a report's statistics phase reads at most this many bytes.  Two reports'
# statistics kernels then overlap at their launch boundaries (one launch's ramp and tail, ~15-35
# us) -- configs[1] (4.3 GB) 0.673-0.687 -> 0.638-0.651 ms per report (with the stagger below,
# profiles/r05/pipe_modes.json); a longer phase gains
# nothing there and loses to the two kernels sharing the GPU for their whole duration: configs[2]
# (34 GB) 5.57 ms whole, 5.65 side, 5.79 alt (profiles/r05/pipe_modes.json).  Above it: whole on 1
# GPU, side on N GPUs (the exchange sits between a report's phases, so it needs two streams).
PIPE_ALT_MAX_BYTES = 8 << 30

TIMED_SPIN_CYCLES = 50_000  # ~20-25 us of device spin ahead of a timed report
STAGGER_FRAC = 0.25  # PipelinedReports: a burst's second report starts this much of a phase later


def _spin(cycles: int) -> None:
    """A one-wave device spin on the current stream (torch's private _sleep kernel)."""
    spin = getattr(torch.cuda, "_sleep", None)
    if spin is not None:
        spin(int(cycles))


class PipelinedReports:
    """Full reports as HIP graphs, two in flight.  Each report -- column-reference init,
    statistics, scores + straggler masks -- ends with its packed results landing in one of two
    pinned host buffers, so the host can read report i while report i+1 runs: the GPU sees
    back-to-back reports instead of one report per host round trip.
    mode "alt": report i runs on stream i % 2 with its own set of statistics / reference
    buffers (_ReportBuffers; set 0 is the reporter's own), so report i+1's statistics kernel starts while report i's drains instead of
    after it (the launch-to-launch transition of one stream); report i's scores wait for report
    i-1's, so the individual history advances in submission order.  "side": every statistics
    phase on one stream, every rest on another (buffer sets per report in flight as in alt).
    "whole": one whole-report graph per report on the caller's stream (1 GPU).  "auto" (default):
    alt for statistics phases up to PIPE_ALT_MAX_BYTES, else whole (side on N GPUs); on N GPUs
    the choice takes the largest shard's bytes -- one all_reduce in the constructor, so every
    rank constructs its PipelinedReports at the same point, as it calls report().  With two
    streams the inputs a report reads must not change until it is collected (collect() orders
    the caller's stream after it).  N GPUs (exchange): per report the statistics, the shard's
    partials and the combine (+ result copy) are graphs and the all_gather of the partials is
    issued eagerly between them, in report order on every rank (the gathered buffers are per
    report in flight too).
    timing: submit(timed=True) first lets the reports in flight finish, then replays the
    statistics phase as its own graph between two timing events (ROCm's torch refuses events
    inside a capture) and the rest of the report as another -- a clean measurement of the
    statistics kernel on an otherwise idle device, for a sample of the reports.  timing_reps=n: that
    graph holds the statistics phase n times back to back (same inputs and outputs each time) and
    collect() returns the mean per phase, so the events' own overhead and a graph launch are spread
    over n phases.
    stats: the statistics phase as a callable stats(bufs) over a buffer set, or a list of them,
    one per input set (report i runs stats[i % len(stats)]; MatrixReporter.pipelined and
    pipelined_records build them).  stats_bytes: what one statistics phase reads (the mode
    choice and the stagger).  inputs: per input set, the tensors its statistics phase
    reads; collect() raises if one of them was modified in place by torch while the report was
    in flight.
    Other work on the same reporter (report(), a ReportGraph, compute_stats, reset_history)
    issued before collect() is ordered after the reports in flight
    (MatrixReporter._order_after_inflight)."""

    def __init__(self, rep: MatrixReporter, stats, *, inputs, stats_bytes: int,
                 timing: bool = False, mode: Optional[str] = None, depth: int = 2,
                 timing_reps: int = 1):
        self.mode = mode or _PIPE_MODE or "auto"
        if callable(stats):
            stats = [stats]
        self.inputs = list(inputs)
        if len(self.inputs) != len(stats) or depth % len(stats) != 0:
            raise ValueError(f"pipelined reports: {len(stats)} input sets for depth {depth} "
                             "(one inputs entry per set; the set count divides depth)")
        if self.mode == "auto":
            if rep.exchange and rep.world > 1:  # one mode on every rank (shards differ in size)
                x = torch.tensor([float(stats_bytes)], dtype=torch.float64,
                                 device="cpu" if rep.gloo else rep.device)
                torch.distributed.all_reduce(x, torch.distributed.ReduceOp.MAX, group=rep.group)
                stats_bytes = int(x.item())
            self.mode = ("alt" if stats_bytes <= PIPE_ALT_MAX_BYTES else
                         "side" if rep.exchange else "whole")
        if self.mode not in ("alt", "side", "whole"):
            raise ValueError(f"pipelined reports: mode {self.mode!r} (auto | alt | side | whole)")
        if rep.exchange and self.mode == "whole":
            raise RuntimeError("pipelined reports on N GPUs: two streams only (mode 'whole' is 1 GPU)")
        self.alt = self.mode != "whole"  # two streams, a buffer set per report in flight
        if depth < 2 or (depth > 2 and not self.alt):
            raise ValueError("pipelined reports: depth >= 2 (> 2 with two streams only)")
        self.depth = depth
        self.rep, self.timing = rep, timing
        if timing_reps < 1:
            raise ValueError("timing_reps >= 1")
        self.timing_reps = timing_reps
        self.bufs = [torch.zeros_like(rep.h_out).pin_memory() for _ in range(depth)]

        # the buffer set of each report in flight: with two streams one per report, the first the
        # reporter's own; whole reports on one stream all use the reporter's own
        self.slots = [rep.own] + [_ReportBuffers.new(rep) if self.alt else rep.own
                                  for _ in range(depth - 1)]

        def run_stats(k: int, reps: int = 1):
            b = self.slots[k]
            ready = b.clean
            for _ in range(reps):
                # a repeated phase reads the same inputs: the fused reference the previous one
                # left is the same minimum, so it needs no re-initialisation either
                b.clean = ready
                stats[k % len(stats)](b)

        def run_scores(k: int):
            # the scores kernel writes the pinned buffer itself when its epilogue stores the
            # error word (fused reference, R <= FUSED_REF_MAX_ROWS); otherwise the error word is
            # zeroed on the device first and the results copied
            if rep._fuse_ref():
                rep.compute_scores(out_buf=self.bufs[k], bufs=self.slots[k])
            else:
                rep.compute_scores(bufs=self.slots[k])
                rep._copy_out(self.bufs[k], self.slots[k])

        if self.alt:
            self.stats_g, self.rest_g, self.part_g, self.fin_g, self.stats_t = [], [], [], [], []
            for k, b in enumerate(self.slots):
                _warm_up(rep, stats[k % len(stats)], b)  # initialises this set's column reference too
                ready = b.clean
                self.stats_g.append(_capture(partial(run_stats, k)))
                if timing:  # the timed statistics phase, timing_reps times in one graph,
                    b.clean = ready  # replacing stats_g in a timed report
                    self.stats_t.append(_capture(partial(run_stats, k, self.timing_reps)))
                if rep.exchange:  # N GPUs: partials | eager all_gather | combine + result copy
                    self.part_g.append(_capture(partial(rep._scores_partials, b)))
                    self.fin_g.append(_capture(partial(rep._finalize, b),
                                               partial(rep._copy_out, self.bufs[k], b)))
                else:
                    self.rest_g.append(_capture(partial(run_scores, k)))
            self._needs_clean = rep.own.clean
            self.streams = [torch.cuda.Stream(rep.device) for _ in range(depth)]
            self.hist_done = [torch.cuda.Event() for _ in range(depth)]
            self.stats_done = [torch.cuda.Event() for _ in range(depth)]
        else:
            _warm_up(rep, stats[0])
            self._needs_clean = rep.own.clean  # as ReportGraph: every graph here pairs both phases
            self.full = [_capture(partial(run_stats, k), partial(run_scores, k)) for k in range(2)]
            if timing:
                self.stats = _capture(partial(run_stats, 0, self.timing_reps))
                self.rest = [_capture(partial(run_scores, k)) for k in range(2)]
        if timing:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        # blocking-sync events: wait_event's fallback sleeps instead of polling
        self.done = [torch.cuda.Event(blocking=True) for _ in range(depth)]
        self._versions = [None] * depth  # the inputs' version counters at each slot's submit
        # the one-time stagger of a burst's second report: a quarter of the statistics phase at
        # ~6.5 TB/s (STAGGER_FRAC; NVRX_PIPE_STAGGER=0 disables), in spin cycles of ~2.2 GHz
        frac = float(os.environ.get("NVRX_PIPE_STAGGER", STAGGER_FRAC))
        self.stagger_cycles = int(frac * stats_bytes / 6.5e12 * 2.2e9) if stats_bytes else 0
        self._burst = -2
        self.pending = []  # (slot, statistics phases timed or 0) in flight, oldest first
        self.ready = []    # results collected early (a timed submit drains), oldest first
        self.n = 0
        self.last_input = None
        rep._pipes.add(self)

    def submit(self, timed: bool = False) -> None:
        """Queue the next report (at most `depth` in flight: collect() the oldest first)."""
        if len(self.pending) == self.depth:
            raise RuntimeError(f"{self.depth} reports in flight: collect() one first")
        if self._needs_clean and not self.rep.own.clean:
            raise RuntimeError("PipelinedReports: an unpaired statistics phase (ReportGraph."
                               "run_stats without run_rest) left the column reference in use")
        if timed and not self.timing:
            raise RuntimeError("PipelinedReports(timing=True) is needed for timed reports")
        k = self.n % self.depth
        if timed:
            while self.pending:  # the device idles before the measured statistics phase
                self.ready.append(self._land())
        self.rep._order_after_inflight(exclude=self)  # another pipeline's reports on this reporter
        self._versions[k] = [t._version for t in self.inputs[k % len(self.inputs)]]
        if timed:
            # a short spin keeps the device busy while the host queues the graphs, so the
            # first event fires right before the statistics phase rather than a graph-launch
            # latency ahead of it
            _spin(TIMED_SPIN_CYCLES)
        if self.alt:
            self._submit_two_streams(k, timed)
        else:
            self._submit_whole(k, timed)
        self.rep.own.clean = self.rep._fuse_ref()
        if not self.pending:
            self._burst = self.n  # the first report of a burst (submitted to an empty pipeline)
        self.pending.append((k, self.timing_reps if timed else 0))
        self.n += 1

    def _submit_two_streams(self, k: int, timed: bool) -> None:
        # alt: report i on stream i % 2; side: every statistics phase on stream 0, every rest
        # on stream 1 (slot k's previous report has finished with its buffers: done[k])
        s = self.streams[k] if self.mode == "alt" else self.streams[0]
        # the caller's work so far (inputs; the wait for the collected reports) comes first
        s.wait_stream(torch.cuda.current_stream(self.rep.device))
        s.wait_event(self.done[k])
        if self.mode == "alt" and self.depth > 2:
            # at most two statistics phases at once: report i's starts on the device as soon
            # as report i-2's has finished, with no host round trip in between
            s.wait_event(self.stats_done[(k - 2) % self.depth])
        if (self.mode == "alt" and self.stagger_cycles > 0 and len(self.pending) == 1
                and self.n == self._burst + 1):
            # the second report of a burst (the pipeline was empty when the first was
            # submitted) starts a quarter of a statistics phase after the first: staggered,
            # one report's statistics kernel covers the other's end, scores and the host's
            # next submission; started together, the two stay locked and the device idles at
            # every pair's end
            with torch.cuda.stream(s):
                _spin(self.stagger_cycles)
        with torch.cuda.stream(s):
            if timed:
                self.ev[0].record(s)
            (self.stats_t[k] if timed else self.stats_g[k]).replay()
            if timed:
                self.ev[1].record(s)
        self.stats_done[k].record(s)
        if self.mode == "side":
            s = self.streams[1]
            s.wait_event(self.stats_done[k])
        with torch.cuda.stream(s):
            s.wait_event(self.hist_done[(k - 1) % self.depth])  # report i-1's history update first
            if self.rep.exchange:
                self.part_g[k].replay()
                self.hist_done[k].record(s)
                # the eager all_gather of this slot's partials, ordered after them on s (every
                # rank submits its reports, hence its collectives, in the same order)
                self.rep._exchange(self.slots[k])
                self.fin_g[k].replay()
            else:
                self.rest_g[k].replay()
                self.hist_done[k].record(s)
        self.done[k].record(s)

    def _submit_whole(self, k: int, timed: bool) -> None:
        if timed:
            self.ev[0].record()
            self.stats.replay()
            self.ev[1].record()
            self.rest[k].replay()
        else:
            self.full[k].replay()
        self.done[k].record()

    def _land(self):
        k, timed = self.pending.pop(0)  # timed: the timed statistics phases (0: untimed)
        ev = self.done[k]
        wait_event(ev)
        if self.alt:  # the caller's later work (new inputs, the history) follows this report
            torch.cuda.current_stream(self.rep.device).wait_event(ev)
        self.last_input = k % len(self.inputs)  # the input set the collected report read
        now = [t._version for t in self.inputs[k % len(self.inputs)]]
        if now != self._versions[k]:
            raise RuntimeError("PipelinedReports: an input of this report was modified in place "
                               "while the report was in flight (submit() -> collect()); its "
                               "results are undefined -- modify inputs only after collect()")
        ms = self.ev[0].elapsed_time(self.ev[1]) / timed if timed else None
        return self.slots[k].unpack(self.bufs[k]), ms

    def collect(self):
        """(BatchResult, statistics ms for a timed report or None) of the oldest report, once it
        landed."""
        if self.ready:
            return self.ready.pop(0)
        return self._land()
