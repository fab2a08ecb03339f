"""Worker of the Detector.kernel_individual_tail_score test: one rank without a process group
pushes seeded records over several report intervals and calls the method before every report."""
import numpy as np

import _tail_workers as TW

NAMES = TW.NAMES
NCCL = "ncclDevKernel_AllReduce_blk_64_1_1_grid_8_1_1"
NEW = "late_blk_128_1_1_grid_4_1_1"
SLOW = NAMES[5]
CALLS, EXTRA, FACTOR = 400, 100, 3
PM, THRESHOLD, TOP = 990, 0.9, 3


def pushed(interval):
    """name -> u32 ns of one interval's pushes.  Intervals 0 and 1 are identical; interval 2 adds
    EXTRA records FACTOR x slower on SLOW and a kernel name not seen before."""
    rng = np.random.default_rng(900)
    out = {}
    for j, n in enumerate(NAMES + [NCCL]):
        out[n] = (20_000 * (j + 1) * (1.0 + 0.02 * rng.random(CALLS))).astype(np.uint32)
    if interval == 2:
        out[SLOW] = np.concatenate([out[SLOW], out[SLOW][:EXTRA] * FACTOR])
        out[NEW] = np.full(50, 33_000, np.uint32)
    return out


def _interval(D, i):
    with D.detection_section("step"):
        for name, d in pushed(i).items():
            D.cupti_manager.push(name, d)
    hists = {n: c.tolist() for n, c in D.kernel_histograms().items()}
    ts = D.kernel_individual_tail_score(permille=PM, threshold=THRESHOLD, top=TOP)
    slots = dict(D._tail_history.slots)
    D.generate_report()
    return dict(ts=vars(ts), hists=hists, slots=slots, after=D.kernel_histograms())


def individual_rank(rank, ws):
    from nvidia_resiliency_ext import straggler

    D = straggler.Detector
    out = []
    D.initialize(scores_to_compute="all", gather_on_rank0=False, node_name="node0")
    try:
        out = [_interval(D, i) for i in range(3)]
    finally:
        D.shutdown()
    D.initialize(scores_to_compute="all", gather_on_rank0=False, node_name="node0")
    try:
        out.append(_interval(D, 0))  # a fresh Detector starts from no history
        D.reset_tail_history()
        out.append(_interval(D, 1))  # and so does a reset one
    finally:
        D.shutdown()
    return out


def _solo_entry(q):
    import sys
    import traceback

    from _mp import PATHS

    for p in PATHS:
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        q.put(("ok", individual_rank(0, 1)))
    except BaseException:
        q.put(("error", traceback.format_exc()))
        raise


def run_solo(timeout=120):
    """individual_rank in a fresh process without a process group, under its own time limit."""
    import queue

    import torch.multiprocessing as mp

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
