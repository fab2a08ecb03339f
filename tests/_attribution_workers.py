"""Fresh-process workers for the score-attribution tests: a 2-rank ReportGenerator world and the
Detector (one profiler may exist per process)."""
import dataclasses

import numpy as np

from _quantile_workers import NAMES, pushed_durations
from _report_workers import get_summary

SLOWED = "mid_k"  # the kernel whose durations double in the Detector's second interval


def rel_attribution(rank, ws):
    from nvidia_resiliency_ext import straggler

    rg = straggler.reporting.ReportGenerator(['relative_perf_scores'], gather_on_rank0=False,
                                             node_name=f'testnode{rank}')
    ks = {'kernel0': get_summary((rank + 1) * np.array([1.0, 1.0, 2.0])),
          'kernel1': get_summary((rank + 1) * np.array([2.0, 2.0, 3.0]))}
    rep = rg.generate_report({}, kernel_summaries=ks)
    att = rg.kernel_attribution(top=2, kind="relative")
    return dict(score=rep.gpu_relative_perf_scores[rank], att=[dataclasses.astuple(a) for a in att])


def detector_attribution(rank, ws):
    from nvidia_resiliency_ext import straggler

    D = straggler.Detector
    D.initialize(scores_to_compute="all", gather_on_rank0=False, node_name="n0")
    try:
        out = []
        for scale in (1, 2):  # the second interval: SLOWED takes twice as long
            with D.detection_section("step"):
                for name, d in pushed_durations().items():
                    D.cupti_manager.push(name, d * np.uint32(scale if name == SLOWED else 1))
            rep = D.generate_report()
            out.append(dict(
                names=list(rep.local_kernel_summaries),
                rel_score=rep.gpu_relative_perf_scores[0], ind_score=rep.gpu_individual_perf_scores[0],
                rel=[dataclasses.astuple(a) for a in D.kernel_attribution(kind="relative")],
                ind=[dataclasses.astuple(a) for a in D.kernel_attribution(top=2, kind="individual")],
                again=[dataclasses.astuple(a) for a in D.kernel_attribution(top=2, kind="individual")]))
        assert len(NAMES) == 3
        return out
    finally:
        D.shutdown()
