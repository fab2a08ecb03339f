"""A MatrixReporter's report as HIP graphs: ReportGraph (one report at a time over the reporter's
own buffers) and PipelinedReports (several in flight); _build_slot captures the graphs of both."""
from __future__ import annotations

import os
from collections import namedtuple
from functools import partial
from typing import Optional

import torch

from .batch import BatchResult, MatrixReporter, _ReportBuffers
from .host_wait import _wait, wait_event


def _capture(*phases) -> torch.cuda.CUDAGraph:
    """The phases (callables), run in order on the current stream, captured as one HIP graph."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for phase in phases:
            phase()
    return g


def _warm_up(rep: MatrixReporter, stats, b: _ReportBuffers) -> None:
    """One eager report over buffer set b on a side stream (first-launch setup outside any graph
    capture); stats(b) runs the statistics phase.  The individual history is restored afterwards:
    whatever the inputs hold now is not folded into it (the graphs' reports advance it as report())."""
    d = rep.device
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


# The HIP graphs of one slot (a buffer set and the pinned buffer its results land in): stats;
# stats_timed, the statistics phase timing_reps times; rest (1 GPU: scores, results to the host) or
# partials | eager all_gather | finalize (N GPUs); full (1 GPU): stats + rest.  None: not captured.
_SlotGraphs = namedtuple("_SlotGraphs", "stats stats_timed rest partials finalize full")


def _build_slot(rep: MatrixReporter, bufs: _ReportBuffers, stats, host: torch.Tensor, *,
                timing_reps: int = 0, full: bool = False,
                scores_write_host: bool = False) -> _SlotGraphs:
    """Warm up over bufs, then capture the slot's graphs.  stats(bufs): the statistics phase;
    host: the pinned buffer the results land in; timing_reps > 0: the timed graph too.
    scores_write_host (1 GPU): the scores kernel writes `host` itself -- it can when its epilogue
    stores the error word (fused reference); else that word is zeroed on the device, results copied."""
    _warm_up(rep, stats, bufs)
    # The invariant behind colref_ready: after any scores phase or warm-up of a buffer set,
    # bufs.clean == rep._fuse_ref() (the statistics phases clear the flag, _scores sets it to
    # `fused`, the N-GPU warm-up sets it only when fused).  A statistics graph bakes the flag in
    # when it is captured and is only ever replayed after a scores phase (_check_paired), so
    # every statistics capture starts from that value, whatever was captured before it.
    fused, ex = rep._fuse_ref(), rep.exchange
    assert bufs.clean == fused

    def run_stats(reps: int = 1):
        for _ in range(reps):
            # (a repeat reads the same inputs: the fused reference it finds is already its minimum)
            bufs.clean = fused
            stats(bufs)

    copy_out = partial(rep._copy_out, host, bufs)
    scores = partial(rep.compute_scores, out_buf=host if scores_write_host else None, bufs=bufs)
    rest = (scores,) if scores_write_host else (scores, copy_out)
    return _SlotGraphs(
        stats=_capture(run_stats),
        stats_timed=_capture(partial(run_stats, timing_reps)) if timing_reps else None,
        rest=None if ex else _capture(*rest),
        partials=_capture(partial(rep._scores_partials, bufs)) if ex else None,
        finalize=_capture(partial(rep._finalize, bufs), copy_out) if ex else None,
        full=_capture(run_stats, *rest) if full else None)


def _check_paired(rep: MatrixReporter, msg: str) -> None:
    # a captured statistics phase must not follow one whose scores (own set) have not run
    if rep._fuse_ref() and not rep.own.clean:
        raise RuntimeError(msg)


class ReportGraph:
    """HIP graphs over a MatrixReporter's own buffer set.  1 GPU: ``run()`` replays the whole
    report (segment statistics, scores + straggler masks, the device-to-host copy of the packed
    results) as one graph; the same work is also captured as two halves for callers that record
    timing events between them (``run_stats()`` + ``run_rest()``: bench.py's one-report-at-a-time
    leg, its "phases" figures); one graph instead of two saves a graph launch per report.
    N GPUs: statistics, the shard's partials and the combine are graphs; the all_gather of the
    partials stays an eager collective between them."""

    def __init__(self, rep: MatrixReporter, ns: Optional[torch.Tensor], s_push: int, stats=None):
        self.rep = rep
        if stats is None:  # the statistics phase (record streams: MatrixReporter.graph_records)
            stats = lambda bufs: rep.compute_stats(ns, s_push, bufs=bufs)  # noqa: E731
        self.g = _build_slot(rep, rep.own, stats, rep.h_out, full=not rep.exchange)

    def _check_clean(self) -> None:
        _check_paired(self.rep, "ReportGraph: the statistics graph was captured to follow a scores "
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
        self.g.stats.replay()
        self.rep.own.clean = False

    def run_rest(self) -> BatchResult:
        rep, g = self.rep, self.g
        rep._order_after_inflight()
        if g.rest is None:  # N GPUs: partials graph, eager all_gather, combine graph
            g.partials.replay()
            rep._exchange()
            g.finalize.replay()
        else:
            g.rest.replay()
        return self._finish()

    def run(self) -> BatchResult:
        if self.g.full is None:
            self.run_stats()
            return self.run_rest()
        self._check_clean()
        self.rep._order_after_inflight()
        self.g.full.replay()
        return self._finish()


# NVRX_PIPE_MODE: alt | side | whole for every PipelinedReports that is given no mode= (timing A/B)
_PIPE_MODE = os.environ.get("NVRX_PIPE_MODE", "")
# "auto": alt while a report's statistics phase reads at most this many bytes.  Two reports'
# statistics kernels then overlap at their launch boundaries (one launch's ramp and tail, ~15-35
# us) -- configs[1] (4.3 GB) 0.673-0.687 -> 0.638-0.651 ms per report (with the stagger below,
# profiles/r05/pipe_modes.json); a longer phase gains nothing there and loses to the two kernels
# sharing the GPU for their whole duration: configs[2] (34 GB) 5.57 ms whole, 5.65 side, 5.79 alt
# (same file).  Above it: whole on 1 GPU, side on N GPUs (the exchange sits between a report's
# phases, so it needs two streams).
PIPE_ALT_MAX_BYTES = 8 << 30

TIMED_SPIN_CYCLES = 50_000  # ~20-25 us of device spin ahead of a timed report
STAGGER_FRAC = 0.25  # PipelinedReports: a burst's second report starts this much of a phase later


def _spin(cycles: int) -> None:
    """A one-wave device spin on the current stream (torch's private _sleep kernel)."""
    spin = getattr(torch.cuda, "_sleep", None)
    if spin is not None:
        spin(int(cycles))


class PipelinedReports:
    """Full reports as HIP graphs, `depth` (default two) in flight: the host reads report i while
    report i+1 runs, so the GPU sees back-to-back reports instead of one per host round trip.
    - Slot: report i uses slot k = i % depth: a buffer set (slots[k]; slots[0] is the reporter's
      own), a pinned host buffer for its packed results and the graphs over both (graphs[k]).
      It runs stats[k % len(stats)]: one callable stats(bufs) per input set.
    - mode "alt": a buffer set and a stream per slot, so report i+1's statistics kernel starts
      while report i's drains (depth > 2: at most two statistics phases at once); report i's
      scores wait for report i-1's, so the individual history advances in submission order.
    - mode "side": buffer sets as in alt; all statistics phases on one stream, every rest on another.
    - mode "whole" (1 GPU, depth 2): every slot over the reporter's own set, one whole-report
      graph per report on the caller's stream.
    - mode "auto" (default): alt while a statistics phase reads at most PIPE_ALT_MAX_BYTES
      (stats_bytes), else whole, or side on N GPUs.  N GPUs take the largest shard's bytes: one
      all_reduce in the constructor, so every rank constructs its pipeline at the same point.
    - N GPUs (exchange): statistics, the shard's partials and the combine (+ result copy) are
      graphs; the all_gather of the partials runs eagerly between them, in report order.
    - timing: submit(timed=True) lets the reports in flight finish, then replays the slot's
      timed statistics graph (the phase timing_reps times back to back) between two timing
      events (ROCm's torch refuses events inside a capture) and the rest as another graph: the
      phase alone on an idle device.  collect() returns the mean ms per phase.
    - inputs (per input set, the tensors its statistics phase reads), in every mode: they must
      not change while a report that reads them is in flight; collect() raises if torch
      modified one in place between that report's submit() and collect().
    - Other work on the same reporter (report(), a ReportGraph, compute_stats, reset_history)
      issued before collect() queues behind the reports in flight (_order_after_inflight)."""

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
        if timing_reps < 1:
            raise ValueError("timing_reps >= 1")
        self.rep, self.depth, self.timing, self.timing_reps = rep, depth, timing, timing_reps
        self.bufs = [torch.zeros_like(rep.h_out).pin_memory() for _ in range(depth)]
        self.slots = [rep.own] + [_ReportBuffers.new(rep) if self.alt else rep.own
                                  for _ in range(depth - 1)]
        self.graphs = [_build_slot(rep, self.slots[k], stats[k % len(stats)], self.bufs[k],
                                   timing_reps=timing_reps if timing else 0, full=not self.alt,
                                   scores_write_host=rep._fuse_ref())
                       for k in range(depth)]
        if self.alt:
            self.streams = [torch.cuda.Stream(rep.device) for _ in range(depth)]
            self.hist_done = [torch.cuda.Event() for _ in range(depth)]
            self.stats_done = [torch.cuda.Event() for _ in range(depth)]
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
        _check_paired(self.rep, "PipelinedReports: an unpaired statistics phase (ReportGraph."
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
            # a short spin keeps the device busy while the host queues the graphs, so the first event
            # fires right before the statistics phase rather than a graph-launch latency ahead of it
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
        g = self.graphs[k]
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
            (g.stats_timed if timed else g.stats).replay()
            if timed:
                self.ev[1].record(s)
        self.stats_done[k].record(s)
        if self.mode == "side":
            s = self.streams[1]
            s.wait_event(self.stats_done[k])
        with torch.cuda.stream(s):
            s.wait_event(self.hist_done[(k - 1) % self.depth])  # report i-1's history update first
            if self.rep.exchange:
                g.partials.replay()
                self.hist_done[k].record(s)
                # the eager all_gather of this slot's partials, ordered after them on s (every
                # rank submits its reports, hence its collectives, in the same order)
                self.rep._exchange(self.slots[k])
                g.finalize.replay()
            else:
                g.rest.replay()
                self.hist_done[k].record(s)
        self.done[k].record(s)

    def _submit_whole(self, k: int, timed: bool) -> None:
        g = self.graphs[k]
        if timed:
            self.ev[0].record()
            g.stats_timed.replay()
            self.ev[1].record()
            g.rest.replay()
        else:
            g.full.replay()
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
