"""Fresh-process workers for the histogram tests of the profiler handle and the Detector (one
profiler may exist per process)."""
import numpy as np

NAMES = ["zeta_kernel_blk_64_1_1_grid_8_1_1", "alpha_blk_256_1_1_grid_1_1_1", "mid_k"]
COUNTS = [21, 7, 1]
RING = 7


def pushed_durations():
    rng = np.random.default_rng(240)
    d = {n: rng.integers(1000, 900_000, size=c, dtype=np.uint32) for n, c in zip(NAMES, COUNTS)}
    d[NAMES[0]][-3:] = (5, 70_000_000, 70_000_001)  # far apart, and two in one bucket
    return d


def _stats_tuple(stats):
    return {k: (s.num_calls, s.min, s.max, s.median, s.avg, s.stddev) for k, s in stats.items()}


def profiler_histograms(rank, ws):
    from nvidia_resiliency_ext.straggler import cupti

    p = cupti.KernelProfiler(statsMaxLenPerKernel=RING, capture=False)
    try:
        p.initialize()
        p.start()
        for name, d in pushed_durations().items():  # not in sorted order
            p.push(name, d)
        before = _stats_tuple(p.get_stats())
        names, num, counts = p.get_histograms()
        again = p.get_histograms()
        after = _stats_tuple(p.get_stats())
        nrec = len(p.get_records()[0])
        p.reset()
        empty = p.get_histograms()
        return dict(names=names, num=num.tolist(), counts=counts, again_names=again[0],
                    again_counts=again[2], before=before, after=after, nrec=nrec,
                    empty=(empty[0], empty[1].tolist(), tuple(empty[2].shape)))
    finally:
        p.close()


def detector_histograms(rank, ws):
    from nvidia_resiliency_ext import straggler

    D = straggler.Detector
    D.initialize(scores_to_compute="all", gather_on_rank0=False, node_name="n0")
    try:
        with D.detection_section("step"):
            for name, d in pushed_durations().items():
                D.cupti_manager.push(name, d)
        h = D.kernel_histograms()
        rep = D.generate_report()
        S = straggler.Statistic
        kern = {k: (v[S.NUM], v[S.MIN], v[S.MAX], v[S.MED]) for k, v in rep.local_kernel_summaries.items()}
        return dict(h=h, kern=kern, rel=dict(rep.gpu_relative_perf_scores), after=D.kernel_histograms())
    finally:
        D.shutdown()
