"""The individual tail-score definition (include/nvrx_straggler.h, nvrx_histogram_history_scores)
in plain Python integers and CPython floats: the reference of the history tail-score tests.  No
numpy arithmetic, no native library, nothing from ``histograms.py``."""
import math
from operator import mul

from _tail_ref import BINS, M64, W, bits  # noqa: F401

SCORE, UPDATE = 1, 2
U32 = 0xFFFFFFFF


def threshold_of(h, pm):
    """The bucket of the sample of 0-based rank (pm (N - 1)) // 1000 of histogram h (N > 0)."""
    rank, c = (pm * (sum(h) - 1)) // 1000, 0
    for b in range(BINS):
        c += h[b]
        if c > rank:
            return b
    raise AssertionError("empty histogram")


def history_scores(counts, hist, pm, mode=SCORE | UPDATE, hist_index=None, col_valid=None,
                   skip_rows=None, score_thr=0.75):
    """counts [R][K][240], hist [R][S][240] lists of ints (hist is not modified).  Returns
    (rows, new_hist): rows is None without SCORE, else per row a dict of tail_ns, total_ns,
    base_tail_ns, base_total_ns (mod 2^64), score (CPython float), strag, calls[K], T[K];
    new_hist is hist itself without UPDATE."""
    assert mode in (SCORE, UPDATE, SCORE | UPDATE)
    K = len(counts[0]) if counts else 0
    slot = list(range(K)) if hist_index is None else list(hist_index)
    taken = [k for k in range(K) if slot[k] >= 0 and (col_valid is None or col_valid[k])]
    assert len({slot[k] for k in taken}) == len(taken)
    rows = None
    if mode & SCORE:
        rows = []
        for r, row in enumerate(counts):
            tail = total = btail = btotal = 0
            calls, T = [0] * K, [-1] * K
            for k in taken:
                c, h = row[k], hist[r][slot[k]]
                if sum(h) == 0 or sum(c) == 0:
                    continue
                t = T[k] = threshold_of(h, pm)
                total += sum(map(mul, c, W))
                tail += sum(map(mul, c[t + 1:], W[t + 1:]))
                btotal += sum(map(mul, h, W))
                btail += sum(map(mul, h[t + 1:], W[t + 1:]))
                calls[k] = sum(c[t + 1:]) & U32
            tail, total, btail, btotal = tail & M64, total & M64, btail & M64, btotal & M64
            score = math.nan
            if total != 0 and btotal != 0:
                den = 1.0 - float(btail) / float(btotal)
                if den != 0.0:
                    score = (1.0 - float(tail) / float(total)) / den
            rows.append(dict(tail_ns=tail, total_ns=total, base_tail_ns=btail, base_total_ns=btotal,
                             score=score, strag=score < score_thr, calls=calls, T=T))
    new = hist
    if mode & UPDATE:
        new = [[list(h) for h in hr] for hr in hist]
        for r, row in enumerate(counts):
            if skip_rows is not None and skip_rows[r]:
                continue
            for k in taken:
                new[r][slot[k]] = [min(a + b, U32) for a, b in zip(hist[r][slot[k]], row[k])]
    return rows, new
