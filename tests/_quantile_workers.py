"""Fresh-process workers for the quantile tests of the profiler handle and the Detector (one
profiler may exist per process)."""
import numpy as np

NAMES = ["zeta_kernel_blk_64_1_1_grid_8_1_1", "alpha_blk_256_1_1_grid_1_1_1", "mid_k"]
COUNTS = [10, 256, 1000]


def pushed_durations():
    rng = np.random.default_rng(21)
    return {n: rng.integers(1000, 900_000, size=c, dtype=np.uint32) for n, c in zip(NAMES, COUNTS)}


def _stats_tuple(stats):
    return {k: (s.num_calls, s.min, s.max, s.median, s.avg, s.stddev) for k, s in stats.items()}


def profiler_quantiles(rank, ws, permille):
    from nvidia_resiliency_ext.straggler import cupti

    p = cupti.KernelProfiler(statsMaxLenPerKernel=256, capture=False)
    try:
        p.initialize()
        p.start()
        for name, d in pushed_durations().items():  # not in sorted order
            p.push(name, d)
        before = _stats_tuple(p.get_stats())
        names, num, q = p.get_quantiles(permille)
        again = p.get_quantiles(permille)
        after = _stats_tuple(p.get_stats())
        nrec = len(p.get_records()[0])
        p.reset()
        empty = p.get_quantiles(permille)
        return dict(names=names, num=num.tolist(), q=q, again_q=again[2], again_names=again[0],
                    before=before, after=after, nrec=nrec,
                    empty=(empty[0], empty[1].tolist(), tuple(empty[2].shape)))
    finally:
        p.close()


def detector_quantiles(rank, ws, permille):
    from nvidia_resiliency_ext import straggler

    D = straggler.Detector
    D.initialize(scores_to_compute="all", gather_on_rank0=False, node_name="n0")
    try:
        with D.detection_section("step"):
            for name, d in pushed_durations().items():
                D.cupti_manager.push(name, d)
        q = D.kernel_quantiles(permille)
        q_default = D.kernel_quantiles()
        rep = D.generate_report()
        S = straggler.Statistic
        kern = {k: (v[S.NUM], v[S.MIN], v[S.MAX], v[S.MED]) for k, v in rep.local_kernel_summaries.items()}
        return dict(q=q, q_default=q_default, kern=kern, rel=dict(rep.gpu_relative_perf_scores),
                    after=D.kernel_quantiles(permille))
    finally:
        D.shutdown()
