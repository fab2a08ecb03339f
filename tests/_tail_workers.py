"""Rank workers of the Detector.kernel_tail_score tests: every rank pushes its own, seeded records
(overlapping but different kernel-name sets, one rank with a tail) and calls the collective."""
import queue
import sys
import traceback

import numpy as np
import torch.multiprocessing as mp

from _mp import PATHS

NAMES = [f"k{j}_blk_256_1_1_grid_{j + 1}_1_1" for j in range(6)]
CALLS = 400
SLOW_RANK = 1
EVERY, FACTOR = 10, 3
PM, THRESHOLD = 900, 0.9


def rank_names(rank, ws):
    """All but one kernel per rank (rank r misses NAMES[r]); with ws == 1 all of them."""
    return [n for j, n in enumerate(NAMES) if ws == 1 or j != rank]


def pushed(rank, ws):
    """name -> u32 ns of this rank's pushes: ~2 % jitter about a per-kernel base; the slow rank
    is FACTOR x slower on every EVERY-th call."""
    rng = np.random.default_rng(500 + rank)
    out = {}
    for n in rank_names(rank, ws):
        base = 20_000 * (NAMES.index(n) + 1)
        d = (base * (1.0 + 0.02 * rng.random(CALLS))).astype(np.uint64)
        if rank == SLOW_RANK or ws == 1:
            d[::EVERY] *= FACTOR
        out[n] = d.astype(np.uint32)
    return out


def tail_score_rank(rank, ws, tail=True):
    from nvidia_resiliency_ext import straggler

    D = straggler.Detector
    D.initialize(scores_to_compute="all", gather_on_rank0=False, node_name=f"node{rank}")
    try:
        with D.detection_section("step"):
            for name, d in pushed(rank, ws).items():
                D.cupti_manager.push(name, d)
        ts = D.kernel_tail_score(permille=PM, threshold=THRESHOLD, top=3) if tail else None
        rep = D.generate_report()
        S = straggler.Statistic
        kern = {k: tuple(v[s] for s in (S.NUM, S.MIN, S.MAX, S.MED, S.AVG, S.STD))
                for k, v in rep.local_kernel_summaries.items()}
        return dict(ts=None if ts is None else vars(ts), kern=kern,
                    rel=dict(rep.gpu_relative_perf_scores), ind=dict(rep.gpu_individual_perf_scores),
                    after=D.kernel_histograms())
    finally:
        D.shutdown()


def _solo_entry(q):
    for p in PATHS:
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        import torch

        assert not torch.distributed.is_initialized()
        q.put(("ok", tail_score_rank(0, 1)))
    except BaseException:
        q.put(("error", traceback.format_exc()))
        raise


def run_solo(timeout=120):
    """tail_score_rank in a fresh process WITHOUT a process group, under its own time limit."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_solo_entry, args=(q,))
    p.start()
    try:
        status, res = q.get(timeout=timeout)
    except queue.Empty:
        raise AssertionError(f"the worker did not finish within {timeout} s") from None
    finally:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()
    assert status == "ok", res
    return res
