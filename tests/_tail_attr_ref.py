"""A plain reference of the tail score attribution (include/nvrx_straggler.h), independent of
``straggler.histograms``: loops over Python ints, f64 by ``float``, ``sorted`` with the key
``(-loss, k)``.  Inputs are nested lists (or anything ``int()`` takes); u32 counts as unsigned."""
import math
import struct

BINS = 240
M64 = (1 << 64) - 1


def edge(b: int) -> int:
    return b if b < 8 else (8 + b % 8) << (b // 8 - 1)


W = [edge(min(b, BINS - 2)) for b in range(BINS)]


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def rank_bucket(h, pm):
    """The bucket of the sample of 0-based rank (pm (n - 1)) // 1000; None without samples."""
    n = sum(h)
    if n == 0:
        return None
    rank, acc = (pm * (n - 1)) // 1000, 0
    for b in range(BINS):
        acc += h[b]
        if acc > rank:
            return b


def sums(h, t):
    total = tail = calls = 0
    for b in range(BINS):
        total += h[b] * W[b]
        if b > t:
            tail += h[b] * W[b]
            calls += h[b]
    return tail & M64, total & M64, calls & 0xFFFFFFFF


def excess(tail, total, btail, btotal):
    if btotal == 0:
        share = math.nan if btail == 0 else math.inf
    else:
        share = float(btail) / float(btotal)
    prod = float(total) * share
    return share, float(tail) - prod


def rank_rows(R, K, top, element):
    """Per row the `top` taken elements by (-loss, k); every output as nested lists."""
    out = dict(idx=[], loss=[], tail_ns=[], total_ns=[], tail_calls=[], thr_bucket=[], base_share=[],
               loss_all=[])
    for r in range(R):
        taken, dense = [], [math.nan] * K
        for k in range(K):
            e = element(r, k)
            if e is None or math.isnan(e["loss"]):
                continue
            dense[k] = e["loss"]
            taken.append((k, e))
        taken = sorted(taken, key=lambda ke: (-ke[1]["loss"], ke[0]))[:top]
        pad = top - len(taken)
        out["idx"].append([k for k, _ in taken] + [-1] * pad)
        out["loss"].append([e["loss"] for _, e in taken] + [math.nan] * pad)
        out["tail_ns"].append([e["tail"] for _, e in taken] + [0] * pad)
        out["total_ns"].append([e["total"] for _, e in taken] + [0] * pad)
        out["tail_calls"].append([e["calls"] for _, e in taken] + [0] * pad)
        out["thr_bucket"].append([e["T"] for _, e in taken] + [-1] * pad)
        out["base_share"].append([e["share"] for _, e in taken] + [math.nan] * pad)
        out["loss_all"].append(dense)
    return out


def relative(counts, pm, top, col_valid=None, fleet=None, thr_index=None):
    R, K = len(counts), len(counts[0]) if len(counts) else 0
    if fleet is None:
        fleet = [[sum(counts[r][k][b] for r in range(R)) for b in range(BINS)] for k in range(K)]
    T = []
    for u, f in enumerate(fleet):
        t = rank_bucket(f, pm)
        T.append(-1 if t is None or (col_valid is not None and not col_valid[u]) else t)

    def element(r, k):
        u = k if thr_index is None else thr_index[k]
        if u < 0 or T[u] < 0 or sum(counts[r][k]) == 0:
            return None
        tail, total, calls = sums(counts[r][k], T[u])
        btail, btotal, _ = sums(fleet[u], T[u])
        share, loss = excess(tail, total, btail, btotal)
        return dict(loss=loss, tail=tail, total=total, calls=calls, T=T[u], share=share)

    return rank_rows(R, K, top, element)


def individual(counts, hist, pm, top, hist_index=None, col_valid=None):
    R, K = len(counts), len(counts[0]) if len(counts) else 0

    def element(r, k):
        s = k if hist_index is None else hist_index[k]
        if s < 0 or (col_valid is not None and not col_valid[k]):
            return None
        t = rank_bucket(hist[r][s], pm)
        if t is None or sum(counts[r][k]) == 0:
            return None
        tail, total, calls = sums(counts[r][k], t)
        btail, btotal, _ = sums(hist[r][s], t)
        share, loss = excess(tail, total, btail, btotal)
        return dict(loss=loss, tail=tail, total=total, calls=calls, T=t, share=share)

    return rank_rows(R, K, top, element)
