"""The tail-score definition (include/nvrx_straggler.h) in plain Python integers and CPython
floats: the reference of the tail-score tests.  No numpy arithmetic, no native library."""
import math
import struct
from operator import mul

BINS = 240
M64 = (1 << 64) - 1


def edge(b: int) -> int:
    return b if b < 8 else (8 + b % 8) << (b // 8 - 1)


W = [edge(min(b, 238)) for b in range(BINS)]


def bucket(x: int) -> int:
    if x < 8:
        return x
    e = x.bit_length() - 1
    return 8 * (e - 2) + ((x >> (e - 3)) & 7)


def fleet_of(counts):
    """counts: [R][K][240] lists of ints -> F[K][240]."""
    K = len(counts[0]) if counts else 0
    return [list(map(sum, zip(*[row[k] for row in counts]))) for k in range(K)]


def threshold(fleet, pm, col_valid=None):
    """T[K] and (fleet_tail, fleet_total) mod 2^64."""
    T, tail, total = [], 0, 0
    for k, f in enumerate(fleet):
        n = sum(f)
        if n == 0 or (col_valid is not None and not col_valid[k]):
            T.append(-1)
            continue
        rank, c, t = (pm * (n - 1)) // 1000, 0, -1
        for b in range(BINS):
            c += f[b]
            if c > rank:
                t = b
                break
        T.append(t)
        total += sum(map(mul, f, W))
        tail += sum(map(mul, f[t + 1:], W[t + 1:]))
    return T, (tail & M64, total & M64)


def scores(counts, T, sums, score_thr, thr_index=None):
    """Per row: tail_ns, total_ns (mod 2^64), score (CPython float), strag, tail_calls[K]."""
    ftail, ftotal = sums
    out = []
    for row in counts:
        tail = total = 0
        calls = []
        for k, h in enumerate(row):
            ti = k if thr_index is None else thr_index[k]
            t = T[ti] if ti >= 0 else -1
            if t < 0:
                calls.append(0)
                continue
            total += sum(map(mul, h, W))
            tail += sum(map(mul, h[t + 1:], W[t + 1:]))
            calls.append(sum(h[t + 1:]) & 0xFFFFFFFF)
        tail &= M64
        total &= M64
        score = math.nan
        if total != 0 and ftotal != 0:
            share = float(tail) / float(total)
            fs = float(ftail) / float(ftotal)
            den = 1.0 - fs
            if den != 0.0:
                score = (1.0 - share) / den
        out.append(dict(tail_ns=tail, total_ns=total, score=score, strag=score < score_thr,
                        calls=calls))
    return out


def full(counts, pm, score_thr=0.75, col_valid=None):
    """The three steps over one [R][K][240] list; returns (F, T, sums, rows)."""
    F = fleet_of(counts)
    T, sums = threshold(F, pm, col_valid)
    return F, T, sums, scores(counts, T, sums, score_thr)


def bits(x: float):
    """f64 bit pattern, every NaN equal."""
    return "nan" if x != x else struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def hist_of(keys):
    h = [0] * BINS
    for x in keys:
        h[bucket(int(x))] += 1
    return h
