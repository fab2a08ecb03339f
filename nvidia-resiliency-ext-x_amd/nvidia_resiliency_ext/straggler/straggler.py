"""Detector facade (drop-in for straggler/straggler.py:34-408).

Same classmethod API: initialize / shutdown / detection_section / wrap_callables /
restore_original_callables / generate_report / generate_report_if_interval_elapsed /
is_interval_elapsed.  Kernel durations go to the device-resident record log of the
nvrx profiler (cupti.py); at report time the section and kernel statistics and all
scores are computed by HIP kernels (nvrx_section_stats, nvrx_profiler_get_stats,
ReportGenerator).
"""
from __future__ import annotations

import collections
import dataclasses
import functools
import inspect
import socket
import time
from collections.abc import Callable
from contextlib import contextmanager
from typing import Any, Deque, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import dist_utils, histograms, ops
from .cupti import CuptiManager
from .interval_tracker import ReportIntervalTracker
from .reporting import ReportGenerator
from .statistics import Statistic


@dataclasses.dataclass(frozen=True)
class CallableId:
    """A callable to wrap in a detection section: ``getattr(obj, name)`` (straggler.py:34-62)."""

    obj: object
    name: str
    arg_filter_fn: Optional[Callable[[inspect.BoundArguments], bool]] = None
    extra_args_fn: Optional[Callable[[inspect.BoundArguments], dict]] = None
    ignored_args: Optional[tuple] = None

    def __str__(self):
        if inspect.ismodule(self.obj):
            obj_name = self.obj.__name__
        elif inspect.isclass(self.obj):
            obj_name = f"{self.obj.__module__}.{self.obj.__name__}"
        elif hasattr(self.obj, "__class__"):
            obj_name = getattr(self.obj.__class__, "__name__", self.obj)
        else:
            obj_name = getattr(self.obj, "__name__", self.obj)
        return f"{obj_name}.{self.name}"


@dataclasses.dataclass
class CustomSection:
    """A user-defined section: CPU elapsed times (ms) of its profiled entries."""

    name: str
    location: str
    total_entry_cnt: int = 0
    max_elapseds_len: int = 8 * 1024
    cpu_elapsed_times: Deque[float] = dataclasses.field(
        default_factory=lambda: collections.deque(maxlen=CustomSection.max_elapseds_len))


@dataclasses.dataclass
class KernelTailAttribution:
    """One kernel behind a tail score (``kernel_tail_score(attribute=)`` and its individual leg)."""

    name: str
    loss_ns: float        # tail_ns - total_ns * base_share: tail time beyond what the base predicts
    tail_ns: int          # the kernel's weighted counts above its threshold bucket (ns, a lower bound)
    total_ns: int         # all its weighted counts
    tail_calls: int       # its calls above the threshold bucket
    threshold_us: float   # upper edge of the threshold bucket, as ``histograms.edges_us``
    base_share: float     # the tail's share of the base's (fleet's / history's) time on this kernel


@dataclasses.dataclass
class TailScore:
    """What ``Detector.kernel_tail_score`` returns for this rank."""

    score: float          # about 1 healthy, lower = more time in the fleet's tail; NaN: no samples
    tail_ns: int          # weighted counts above the fleet's threshold buckets (ns, a lower bound)
    total_ns: int         # all weighted counts
    fleet_share: float    # fleet_tail / fleet_total: the tail's share of the fleet's time
    is_straggler: bool    # score < threshold (NaN never)
    top: List[Tuple[str, int]]  # (kernel name, calls above its threshold bucket), most first
    attribution: Optional[List[KernelTailAttribution]] = None  # with attribute > 0, largest loss first


@dataclasses.dataclass
class IndividualTailScore:
    """What ``Detector.kernel_individual_tail_score`` returns for this rank."""

    score: float          # about 1 = as its own past, lower = more time in its own tail; NaN: no history
    tail_ns: int          # weighted counts above the history's threshold buckets (ns, a lower bound)
    total_ns: int         # all weighted counts of the kernels scored
    history_share: float  # base_tail / base_total: the tail's share of the history's time
    is_straggler: bool    # score < threshold (NaN never)
    top: List[Tuple[str, int]]  # (kernel name, calls above its threshold bucket), most first
    intervals: int        # intervals the history has absorbed, this one included if it was
    attribution: Optional[List[KernelTailAttribution]] = None  # with attribute > 0, largest loss first


class _TailHistory:
    """The Detector's own histogram history: kernel name -> slot of an int32 [1, capacity, 240]
    device tensor that grows by doubling."""

    def __init__(self):
        self.slots: Dict[str, int] = {}
        self.hist: Optional[torch.Tensor] = None
        self.intervals = 0

    def index(self, names: Sequence[str], dev) -> np.ndarray:
        """The slots of the interval's kernels (new names get new slots), the tensor grown to hold them."""
        for n in names:
            self.slots.setdefault(n, len(self.slots))
        cap = 0 if self.hist is None else self.hist.shape[1]
        if len(self.slots) > cap:
            grown = torch.zeros((1, max(2 * cap, len(self.slots), 64), histograms.BINS),
                                dtype=torch.int32, device=dev)
            if cap:
                grown[:, :cap] = self.hist
            self.hist = grown
        return np.fromiter((self.slots[n] for n in names), dtype=np.int32, count=len(names))


class Detector:
    """Straggler detection entry point; class methods only (not instantiable)."""

    initialized: bool = False
    scores_to_compute: Sequence[str]
    gather_on_rank0: bool
    profiling_interval: int
    report_time_interval: float
    custom_sections: Dict[str, CustomSection]
    cupti_manager: CuptiManager
    reporter: ReportGenerator
    report_interval_tracker: ReportIntervalTracker
    original_callables: Optional[Dict[CallableId, Any]]
    _tail_history: _TailHistory

    def __new__(cls):
        raise RuntimeError(f"class {cls.__name__} should not be instantiated")

    @classmethod
    def initialize(cls, scores_to_compute: Union[Sequence[str], str] = "all",
                   gather_on_rank0: bool = True, profiling_interval: int = 1,
                   report_time_interval: float = 60, node_name: Optional[str] = None):
        assert not cls.initialized
        cls.scores_to_compute = (["relative_perf_scores", "individual_perf_scores"]
                                 if str(scores_to_compute) == "all" else scores_to_compute)
        cls.gather_on_rank0 = gather_on_rank0
        cls.profiling_interval = profiling_interval
        cls.custom_sections = {}
        cls.cupti_manager = CuptiManager(statsMaxLenPerKernel=8 * 1024)
        cls.cupti_manager.initialize()
        cls.reporter = ReportGenerator(scores_to_compute=cls.scores_to_compute,
                                       gather_on_rank0=gather_on_rank0,
                                       node_name=(node_name if node_name else socket.gethostname()))
        cls.report_interval_tracker = ReportIntervalTracker(time_interval=report_time_interval,
                                                            profiling_interval=profiling_interval)
        cls.initialized = True
        cls.original_callables = {}
        cls._tail_history = _TailHistory()

    @classmethod
    def shutdown(cls):
        cls._tail_history = _TailHistory()
        cls.cupti_manager.shutdown()
        cls.restore_original_callables()
        cls.cupti_manager = None
        cls.initialized = False

    @classmethod
    def _get_section_summaries(cls):
        """Section timing statistics, on the device (nvrx_section_stats)."""
        names: List[str] = []
        chunks: List[np.ndarray] = []
        for key, section in cls.custom_sections.items():
            assert key == section.name
            if len(section.cpu_elapsed_times) == 0:
                continue
            names.append(key)
            chunks.append(np.fromiter(section.cpu_elapsed_times, dtype=np.float64))
        if not names:
            return {}
        off = np.zeros(len(chunks) + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in chunks])
        dev = cls.reporter._dev()
        # pinned staging both ways and one synchronisation (four blocking round trips before:
        # ~0.2-0.4 ms of a live report, tools/probe_report_breakdown.py)
        pin = dev.type == "cuda"
        vals_h = torch.from_numpy(np.concatenate(chunks))
        off_h = torch.from_numpy(off)
        if pin:
            vals_h, off_h = vals_h.pin_memory(), off_h.pin_memory()
        num_d, out_d = ops.section_stats(vals_h.to(dev, non_blocking=pin), off_h.to(dev, non_blocking=pin),
                                         max(len(c) for c in chunks))
        num_t = torch.empty(num_d.shape, dtype=num_d.dtype, pin_memory=pin)
        out_t = torch.empty(out_d.shape, dtype=out_d.dtype, pin_memory=pin)
        num_t.copy_(num_d, non_blocking=pin)
        out_t.copy_(out_d, non_blocking=pin)
        if pin:
            torch.cuda.current_stream(dev).synchronize()
        num, out = num_t.numpy(), out_t.numpy()
        return {n: {Statistic.MIN: float(out[0, i]), Statistic.MAX: float(out[1, i]),
                    Statistic.MED: float(out[2, i]), Statistic.AVG: float(out[3, i]),
                    Statistic.STD: float(out[4, i]), Statistic.NUM: int(num[i])}
                for i, n in enumerate(names)}

    @classmethod
    def _get_kernel_summaries(cls):
        """Per-kernel statistics from the device record log (name-sorted mapping)."""
        return cls.cupti_manager.get_results_columns()

    @staticmethod
    def _tail_attribution(names, mine, top, kind, **base) -> List[KernelTailAttribution]:
        """The `top` kernels behind this rank's tail score: two launches and one small
        device-to-host copy of the packed [1, top] outputs."""
        buf = torch.empty(ops.TailAttribution.PACKED * top, dtype=torch.uint8, device=mine.device)
        out = ops.TailAttribution.packed(
            buf, 1, top, torch.empty((1, len(names)), dtype=torch.float64, device=mine.device))
        ops.histogram_tail_attribution(mine, top=top, kind=kind, out=out, **base)
        idx, loss, tail, total, calls, thr, share = (v[0] for v in ops.TailAttribution.unpack(
            buf.cpu().numpy(), 1, top))
        edges = histograms.edges_us()
        return [KernelTailAttribution(names[int(k)], float(loss[j]), int(tail[j]), int(total[j]),
                                      int(calls[j]), float(edges[int(thr[j]) + 1]), float(share[j]))
                for j, k in enumerate(idx) if k >= 0]

    @classmethod
    def kernel_quantiles(cls, permille: Sequence[int] = (500, 900, 990)) -> Dict[str, Tuple[float, ...]]:
        """Duration quantiles (us) of every kernel captured in the current report interval:
        composite kernel name -> one value per entry of ``permille`` (up to 8 ints in
        [0, 1000]).  Entry pm is the sample of 0-based rank ``(pm * (n - 1)) // 1000`` among the
        kernel's n retained durations sorted ascending -- a sample, never an interpolation.
        Beyond the reference: the tail a rank that is slow on every n-th call shows, which its
        median hides.  Call it BEFORE ``generate_report``, which resets the profiler results
        (afterwards the interval is empty and this returns {}).  It changes neither the
        report, nor the scores, nor any collective."""
        assert cls.initialized
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        names, _, q = cls.cupti_manager.get_quantiles(permille)
        return {n: tuple(float(x) for x in q[:, i]) for i, n in enumerate(names)}

    @classmethod
    def kernel_histograms(cls) -> Dict[str, np.ndarray]:
        """Duration histograms of every kernel captured in the current report interval:
        composite kernel name -> int64 counts [240] over the fixed log-linear buckets of
        ``straggler.histograms`` (``histograms.edges_us()`` gives the edges in us).  The buckets
        are the same on every rank and in every report, so the counts of a kernel add over ranks
        and over intervals (``histograms.merge``), and ``histograms.quantile_bounds`` brackets any
        quantile of the sum.  Beyond the reference.  Call it BEFORE ``generate_report``, which
        resets the profiler results (afterwards the interval is empty and this returns {}).  It
        changes neither the report, nor the scores, nor any collective."""
        assert cls.initialized
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        names, _, counts = cls.cupti_manager.get_histograms()
        return {n: counts[i].copy() for i, n in enumerate(names)}

    @classmethod
    def kernel_tail_score(cls, permille: int = 990, threshold: Optional[float] = None,
                          top: int = 8, attribute: int = 0) -> TailScore:
        """This rank's tail score over the current report interval: what the median-based scores
        cannot see, a rank that is slow on every n-th call.  The ranks' kernel histograms
        (``kernel_histograms``) are summed to the fleet's, T_k is the bucket of the fleet's
        ``permille`` quantile of kernel k, ``w(b)`` a bucket's lower edge in ns, and

            score = (1 - tail_ns / total_ns) / (1 - fleet_tail / fleet_total)

        with ``tail_ns`` this rank's weighted counts above T_k over its kernels ("ncclDev"
        kernels are left out, as in the report): about 1 for a healthy rank, lower for one that
        spends more of its time in the fleet's tail -- the scale of the GPU scores, and
        ``is_straggler`` is ``score < threshold`` (None: 0.75, ``identify_stragglers``' default).
        ``top`` is the length of ``TailScore.top``, the (kernel name, calls above T_k) pairs with
        the most tail calls.  A count is not a cost: ``attribute=n`` (1..16) adds
        ``TailScore.attribution``, the n kernels with the largest excess tail time ``tail_ns -
        total_ns * fleet_share_k`` in ns as ``KernelTailAttribution``, largest first, computed on
        the device (no further collective).  Exact integer sums on the device (include/nvrx_straggler.h).  A
        slowdown below one bucket (12.5 %) may not cross T_k, and ``permille`` must leave more
        room than the slow rank's own share of the fleet's samples (8 ranks, every 10th call
        slow: use 950, not 990).

        A COLLECTIVE, unlike the other ``kernel_*`` calls: it adds one ``all_gather_object`` (the
        kernel names) and one ``all_reduce`` (SUM of an int64 [kernels, 240] tensor) on the
        reporter's group, so EVERY rank must call it, at the same point.  Call it BEFORE
        ``generate_report``, which resets the interval; the report is unchanged by it.  With a
        world of one, or without a process group, the fleet is the rank itself.  Beyond the
        reference."""
        assert cls.initialized
        pm = ops.tail_permille(permille)
        ntop = ops.attribution_request(attribute, "relative")[0] if attribute else 0
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        group = cls.reporter.group
        names, _, counts = cls.cupti_manager.get_histograms()  # name-sorted, int64 [n, 240] (host)
        union = sorted(set().union(*dist_utils.all_gather_object(list(names), group)))
        col = {n: i for i, n in enumerate(union)}
        index = np.fromiter((col[n] for n in names), dtype=np.int32, count=len(names))
        fleet_h = np.zeros((len(union), histograms.BINS), np.int64)
        fleet_h[index] = counts
        fleet = torch.from_numpy(fleet_h).to(dist_utils.get_device_for_backend(group))
        dist_utils.all_reduce(fleet, op=torch.distributed.ReduceOp.SUM, group=group)
        thr = 0.75 if threshold is None else float(threshold)
        nan = float("nan")
        if not names:  # nothing captured on this rank: no score (the collectives above still ran)
            return TailScore(nan, 0, 0, nan, False, [], [] if ntop else None)
        dev = cls.reporter._dev()
        valid = torch.from_numpy(np.fromiter(("ncclDev" not in n for n in union), dtype=np.uint8,
                                             count=len(union))).to(dev)
        fleet = fleet.to(dev)
        t_k, sums = ops.histogram_tail_threshold(fleet, pm, col_valid=valid)
        mine = torch.from_numpy(counts.astype(np.uint32).view(np.int32)).to(dev)
        mine = mine.view(1, len(names), histograms.BINS)
        index_d = torch.from_numpy(index).to(dev)
        res = ops.histogram_tail_scores(mine, t_k, sums, score_thr=thr, thr_index=index_d,
                                        tail_calls=True)
        attribution = None
        if ntop:
            attribution = cls._tail_attribution(names, mine, ntop, "relative", thr=t_k,
                                                thr_index=index_d,
                                                base=ops.histogram_tail_base(fleet, t_k))
        ftail, ftotal = (int(v) & (2 ** 64 - 1) for v in sums.tolist())
        calls = res.tail_calls.view(-1).cpu().numpy().view(np.uint32)
        order = sorted(range(len(names)), key=lambda k: (-int(calls[k]), names[k]))
        return TailScore(float(res.score.item()), int(res.tail_ns.item()) & (2 ** 64 - 1),
                         int(res.total_ns.item()) & (2 ** 64 - 1),
                         float(ftail) / float(ftotal) if ftotal else nan, bool(res.strag.item()),
                         [(names[k], int(calls[k])) for k in order[:max(int(top), 0)] if calls[k]],
                         attribution)

    @classmethod
    def kernel_individual_tail_score(cls, permille: int = 990, threshold: Optional[float] = None,
                                     top: int = 8, absorb: str = "healthy",
                                     attribute: int = 0) -> IndividualTailScore:
        """This rank's tail score over the current report interval against its OWN history: the
        individual leg of ``kernel_tail_score``, as the individual GPU score is of the relative
        one.  It sees what a comparison with the fleet cannot: a world of one, a degradation that
        hits every rank together, a large share of the ranks slow on every n-th call.  The
        Detector keeps, on the device, the summed histograms of the intervals absorbed so far per
        kernel name; T_k is the bucket of the ``permille`` quantile of kernel k's history, and

            score = (1 - tail_ns / total_ns) / (1 - base_tail / base_total)

        with ``tail_ns`` / ``base_tail`` this interval's / the history's weighted counts above T_k
        over the kernels that have history and ran in this interval ("ncclDev" kernels are left
        out, as in the report; a kernel name seen for the first time gets a history slot and is
        scored from the next interval on).  About 1 for a rank that behaves as it did, lower for
        one that spends more time above its own past's quantile; ``is_straggler`` is ``score <
        threshold`` (None: 0.75).  The first interval has no history: NaN, never flagged.
        ``absorb``: which intervals join the history -- ``"healthy"`` (default) all but flagged
        ones, so a slow interval does not teach the history that slow is normal, ``"always"``,
        or ``"never"``.  ``top`` is the length of ``IndividualTailScore.top``.  ``attribute=n``
        (1..16) adds ``IndividualTailScore.attribution``, the n kernels with the largest excess
        tail time against the history the score saw (``KernelTailAttribution``, largest first).
        Exact integer
        sums on the device (include/nvrx_straggler.h); a slowdown below one bucket (12.5 %) may not
        cross T_k.  The history costs 960 bytes of device memory per kernel name and is cleared by
        ``initialize`` / ``shutdown`` and ``reset_tail_history``.

        NOT a collective: local to the rank.  Call it BEFORE ``generate_report``, which resets the
        interval; it changes neither the report nor any collective.  Beyond the reference."""
        assert cls.initialized
        pm = ops.tail_permille(permille)
        if absorb not in ("healthy", "always", "never"):
            raise ValueError(f"absorb must be 'healthy', 'always' or 'never', got {absorb!r}")
        ntop = ops.attribution_request(attribute, "individual")[0] if attribute else 0
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        names, _, counts = cls.cupti_manager.get_histograms()  # name-sorted, int64 [n, 240] (host)
        th = cls._tail_history
        nan = float("nan")
        if not names:  # nothing captured: no score, nothing to absorb
            return IndividualTailScore(nan, 0, 0, nan, False, [], th.intervals, [] if ntop else None)
        dev = cls.reporter._dev()
        index = torch.from_numpy(th.index(names, dev)).to(dev)
        valid = torch.from_numpy(np.fromiter(("ncclDev" not in n for n in names), dtype=np.uint8,
                                             count=len(names))).to(dev)
        mine = torch.from_numpy(counts.astype(np.uint32).view(np.int32)).to(dev)
        mine = mine.view(1, len(names), histograms.BINS)
        args = dict(permille=pm, hist_index=index, hist_stride=th.hist.shape[1], col_valid=valid)
        res = ops.histogram_history_scores(mine, th.hist, update=absorb == "always" and not ntop,
                                           tail_calls=True,
                                           score_thr=0.75 if threshold is None else float(threshold),
                                           **args)
        attribution = None
        if ntop:  # between the score and the update: against the history the score saw
            attribution = cls._tail_attribution(names, mine, ntop, "individual", hist=th.hist, **args)
        if absorb == "healthy" or (absorb == "always" and ntop):
            ops.histogram_history_scores(mine, th.hist, score=False,
                                         skip_rows=res.strag if absorb == "healthy" else None, **args)
        M = 2 ** 64 - 1
        flagged = bool(res.strag.item())
        if absorb == "always" or (absorb == "healthy" and not flagged):
            th.intervals += 1
        btail, btotal = int(res.base_tail_ns.item()) & M, int(res.base_total_ns.item()) & M
        calls = res.tail_calls.view(-1).cpu().numpy().view(np.uint32)
        order = sorted(range(len(names)), key=lambda k: (-int(calls[k]), names[k]))
        return IndividualTailScore(
            float(res.score.item()), int(res.tail_ns.item()) & M, int(res.total_ns.item()) & M,
            float(btail) / float(btotal) if btotal else nan, flagged,
            [(names[k], int(calls[k])) for k in order[:max(int(top), 0)] if calls[k]], th.intervals,
            attribution)

    @classmethod
    def reset_tail_history(cls) -> None:
        """Forget the history of ``kernel_individual_tail_score``: the next interval scores NaN."""
        cls._tail_history = _TailHistory()

    @classmethod
    def age_tail_history(cls, shift: int = 1) -> None:
        """Let the history of ``kernel_individual_tail_score`` forget: every count of every
        kernel's summed histogram becomes ``count >> shift`` (``shift`` in 1..31; halved for 1), on
        the device (``ops.histogram_history_age``).  A workload that changed for good -- a new
        sequence length, a kernel one bucket slower after a driver update -- then stops being
        scored against a past that no longer exists after a few calls, without the
        ``reset_tail_history`` that forgets everything at once.  ``IndividualTailScore.intervals``
        keeps counting the intervals absorbed.  Nothing happens before the first interval.  NOT a
        collective: local to the rank.  Beyond the reference."""
        s = ops.age_shift(shift)
        hist = cls._tail_history.hist
        if hist is not None and hist.numel():
            ops.histogram_history_age(hist, s)

    @classmethod
    def kernel_attribution(cls, top: int = 8, kind: str = "relative"):
        """The kernels behind this rank's GPU score in the LAST report: a list of at most `top`
        (1..16) ``KernelAttribution(name, score, loss_us, share)``, largest loss first, where
        ``loss_us = NUM*AVG * (1 - score)`` and the shares of all scored kernels sum to
        ``1 - (GPU score)``.  kind: "relative" (against the best rank) or "individual" (against
        this rank's own best).  Call it AFTER ``generate_report``; RuntimeError before the first
        one.  Beyond the reference: local to the rank, no collective, the report is unchanged."""
        assert cls.initialized
        return cls.reporter.kernel_attribution(top=top, kind=kind)

    @classmethod
    def _reset_sections_elapseds(cls):
        for section in cls.custom_sections.values():
            section.cpu_elapsed_times.clear()

    @classmethod
    def generate_report(cls):
        """ReportGenerator.generate_report over the current summaries, then reset them
        (straggler.py:227-245)."""
        assert cls.initialized
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        section_summaries = cls._get_section_summaries()
        kernel_summaries = cls._get_kernel_summaries()
        report = cls.reporter.generate_report(section_summaries, kernel_summaries)
        cls._reset_sections_elapseds()
        cls.cupti_manager.reset_results()
        return report

    @classmethod
    def generate_report_if_interval_elapsed(cls):
        assert cls.initialized
        cls.report_interval_tracker.iter_increase()
        if cls.report_interval_tracker.is_interval_elapsed():
            return cls.generate_report()
        return None

    @classmethod
    def is_interval_elapsed(cls) -> bool:
        return cls.report_interval_tracker.is_interval_elapsed()

    @staticmethod
    def _get_this_context_block_location() -> str:
        frame = inspect.currentframe().f_back.f_back.f_back  # type: ignore
        return f"{frame.f_code.co_filename}:{frame.f_lineno}"  # type: ignore

    @classmethod
    def _ensure_section_name_is_valid(cls, name, location):
        if name in cls.custom_sections and location != cls.custom_sections[name].location:
            raise ValueError(f"Section name '{name}' is already used at: "
                             f"{cls.custom_sections[name].location}")

    @classmethod
    @contextmanager
    def detection_section(cls, name: Optional[str] = None, profile_cuda: bool = True):
        """Monitor a block of user code: CPU time always, GPU kernels when profile_cuda.
        Only every `profiling_interval`-th entry of a section is profiled."""
        if not cls.initialized:
            raise RuntimeError("Detector is not initialized.")
        location = Detector._get_this_context_block_location()
        if name is None:
            name = location
        section = cls.custom_sections.get(name)
        if section is None:
            section = CustomSection(name=name, location=location)
            cls.custom_sections[name] = section
        profile_this_entry = (section.total_entry_cnt % cls.profiling_interval) == 0
        section.total_entry_cnt += 1
        if profile_this_entry:
            if profile_cuda:
                cls.cupti_manager.start_profiling()
            t0 = time.perf_counter_ns()
            try:
                yield
            except BaseException:
                if profile_cuda:
                    cls.cupti_manager.stop_profiling()
                raise
            section.cpu_elapsed_times.append((time.perf_counter_ns() - t0) * 1e-6)
            if profile_cuda:
                cls.cupti_manager.stop_profiling()
        else:
            yield

    @classmethod
    def _build_wrapper(cls, fn, callable_id, profile_cuda: bool = True):
        @functools.wraps(fn)
        def wrapper(*args, **kwargs):
            with cls.detection_section(name=str(callable_id), profile_cuda=profile_cuda):
                return fn(*args, **kwargs)

        return wrapper

    @classmethod
    def wrap_callables(cls, callable_ids: List[CallableId], profile_cuda: bool = True):
        cls.original_callables = {}
        for cid in callable_ids:
            original = getattr(cid.obj, cid.name)
            cls.original_callables[cid] = original
            setattr(cid.obj, cid.name, cls._build_wrapper(original, cid, profile_cuda=profile_cuda))

    @classmethod
    def restore_original_callables(cls):
        if cls.original_callables:
            for cid, original in cls.original_callables.items():
                setattr(cid.obj, cid.name, original)
