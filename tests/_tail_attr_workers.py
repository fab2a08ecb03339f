"""Worker of the Detector tail attribution test: one rank without a process group pushes the
seeded records of ``_history_tail_workers`` over three report intervals and, before every report,
asks both tail scores for their attribution."""
import _history_tail_workers as HW

PM, THRESHOLD, TOP, ATTRIBUTE = HW.PM, HW.THRESHOLD, HW.TOP, 3


def _plain(ts):
    d = dict(vars(ts))
    d["attribution"] = None if ts.attribution is None else [vars(a) for a in ts.attribution]
    return d


def solo_rank(rank, ws):
    from nvidia_resiliency_ext import straggler

    D = straggler.Detector
    out = []
    D.initialize(scores_to_compute="all", gather_on_rank0=False, node_name="node0")
    try:
        for i in range(3):
            with D.detection_section("step"):
                for name, d in HW.pushed(i).items():
                    D.cupti_manager.push(name, d)
            hists = {n: c.tolist() for n, c in D.kernel_histograms().items()}
            rel = D.kernel_tail_score(permille=PM, threshold=THRESHOLD, top=TOP, attribute=ATTRIBUTE)
            plain = D.kernel_tail_score(permille=PM, threshold=THRESHOLD, top=TOP)
            ind = D.kernel_individual_tail_score(permille=PM, threshold=THRESHOLD, top=TOP,
                                                 attribute=ATTRIBUTE)
            D.generate_report()
            out.append(dict(hists=hists, rel=_plain(rel), rel_plain=_plain(plain), ind=_plain(ind)))
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
        q.put(("ok", solo_rank(0, 1)))
    except BaseException:
        q.put(("error", traceback.format_exc()))
        raise


def run_solo(timeout=120):
    """solo_rank in a fresh process without a process group, under its own time limit."""
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
