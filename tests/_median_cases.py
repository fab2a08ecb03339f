"""Segments built to order for the branches of the median select (`lean_core`, `hist_locate1`,
csrc/segment_wave.h), one aim each (numpy, no GPU).

`build_cases(PL, n, full, kb, m0)` returns the cases of one lean_core instantiation at one retained
length: keys in push order, the `Want` their trace (tests/_median_trace.py) must show, and a short
list of wrong answers -- what a sloppy version of the aimed-at branch would return -- each of which
must differ from the right MED as float32 microseconds (`wrong_answers`).
tests/test_median_trace_cpu.py checks all of that on the CPU; tests/test_gpu_median_branches.py runs
the same segments through the four kernel families against the oracle.

Layout.  d = key - MN.  A histogram level takes LOG bits, so a value is a tuple of digits, one per
level (`Tree`), and a bucket at level k is a prefix of k + 1 digits.  Every segment is
    lower filler | structure M | upper filler
with the counts of the fillers chosen so that rank t0 lands on M[mid].  The fillers hold MIN (d = 0)
and MAX (d = R, which fixes `bits` and B) and live in buckets of level len(prefix) that M does not
use.  The structure is
    compaction cases   a below-siblings | the n0 candidates of bucket prefix + (u,) | b above-siblings
                       (siblings, two digits away under the same prefix, lift every ancestor bucket
                       past 64 samples so the walk descends to level len(prefix))
    two_buckets        a samples ending at hi(b0) - 1 | b samples starting at lo(b1)
    one_value          65 copies of a value between its two neighbours
The padding value is the pivot median3(p[0], p[n / 2], p[n - 1]): p[0] = P, and the other two probes
are a sample <= P and one >= P (MIN and MAX unless a case pins the last slot).
Structure values stay below 2^24 (or are multiples of 512 below 2^28), so neighbouring order
statistics differ as float32 microseconds and a wrong sample cannot hide; keys stay below 0xE0000000.
"""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

import _median_trace as T

MN = 1000
R23 = (1 << 23) - 1          # range 2^23 - 1: bits 23, B = 0x4B000000
R24 = 1 << 23                # range 2^23: bits 24, B = 0
R32 = 0xD0000000             # range >= 2^31: bits 32; MN + R32 < 0xE0000000
KEY_WIDE = 0xE0000000

Case = namedtuple("Case", "name keys want wrong")
# exits: the exit of every visit, in order ("compact" matches any compaction; None: the visits
# after the ones listed are free); at: index of the visit the other fields speak about; pad_at /
# n0: of that visit (pad_at only when the segment has padding); locs: per hist_locate1 call of that
# visit the (row, lane, j, ba) it must find; hasB; lane63_top: lane 63's packed key is 0xFFFFFFFF
# and it is taken as s[t1]
Want = namedtuple("Want", "exits at pad_at n0 locs hasB tie lane63_top",
                  defaults=(None, None, None, None, None, False))


# ------------------------------------------------------------------ the digit tree
class Tree:
    def __init__(self, LOG, R):
        self.LOG, self.R, self.bits = LOG, R, int(R).bit_length()
        s = self.bits - LOG if self.bits > LOG else 0
        self.S = [s]
        while s > 0:
            s = s - LOG if s > LOG else 0
            self.S.append(s)

    def value(self, digits, low=0):
        prev, d = self.bits, 0
        for dig, s in zip(digits, self.S):
            assert 0 <= dig < 1 << min(prev - s, self.LOG), (digits, self.S)
            d |= dig << s
            prev = s
        assert 0 <= low < 1 << prev
        return d | low

    def floor(self, v, k):
        return v >> self.S[k] << self.S[k]

    def where(self, b, BPL):
        """(row, lane, j, ba) of bin b."""
        return b // BPL // 16, b // BPL, b % BPL, b


Ctx = namedtuple("Ctx", "PL n full kb m0 NB LOG BPL pad t0 t1 even")


def _ctx(PL, n, full, kb, m0):
    NB, LOG, BPL = T.bins(PL)
    return Ctx(PL, n, full, kb, m0, NB, LOG, BPL, 0 if full else 64 * PL - n,
               n // 2 if n & 1 else n // 2 - 1, n // 2, n % 2 == 0)


def _segment(cx, name, tree, M, mid, P, fl, last=None, pins=None):
    """The keys in push order, None when the structure does not fit this n."""
    M = [int(v) for v in M]
    assert M == sorted(M) and 0 <= mid < len(M) and 0 <= M[0] and M[-1] <= tree.R
    rng = np.random.default_rng(zlib.crc32(name.encode()) + cx.n)
    L = cx.t0 - mid
    U = cx.n - len(M) - L
    if L < (0 if M[0] == 0 else 1) or U < (0 if M[-1] == tree.R else 1):
        return None
    lo_end = tree.floor(M[0], fl) or M[0]
    up = tree.floor(M[-1], fl) + (1 << tree.S[fl])
    up_start = up if up <= tree.R else M[-1] + 1
    forced_lo = [0] if L and M[0] != 0 else []
    forced_up = [tree.R] if U and M[-1] != tree.R else []
    if P not in M:
        if P < lo_end:
            assert 0 < P
            forced_lo.append(P)
        else:
            assert up_start <= P < tree.R, (name, P, up_start)
            forced_up.append(P)
    if len(forced_lo) > L or len(forced_up) > U:
        return None
    assert L == len(forced_lo) or lo_end > 0, name
    lower = forced_lo + [int(v) for v in rng.integers(0, max(lo_end, 1), size=L - len(forced_lo))]
    upper = forced_up + [int(v) for v in rng.integers(up_start, tree.R + 1, size=U - len(forced_up))]
    d = lower + M + upper
    assert len(d) == cx.n and min(d) == 0 and max(d) == tree.R, (name, len(d), min(d), max(d))
    srt = sorted(d)
    assert srt[cx.t0] == M[mid]
    # push order: p[0] = P, the other two probes on either side of it
    pins = dict(pins or {})
    if last is None:
        last = tree.R
    pins[cx.n - 1] = last
    pins[cx.n // 2] = 0 if last >= P else tree.R
    pins[0] = P
    assert len(pins) == len(set(pins)) and sorted((P, pins[cx.n // 2], last))[1] == P
    pool = list(d)
    for v in pins.values():
        pool.remove(v)
    pool = [int(v) for v in rng.permutation(np.array(pool, np.int64))]
    out = np.empty(cx.n, np.int64)
    free = iter(pool)
    for i in range(cx.n):
        out[i] = pins[i] if i in pins else next(free)
    assert sorted(out.tolist()) == srt
    keys = (MN + out).astype(np.uint32)
    assert int(keys.max()) < KEY_WIDE
    return keys


def _spread(lo, width, count, center):
    """`count` ascending values in [lo, lo + width): distinct when the bucket is wide enough, else
    distinct around index `center` and saturating at the bucket's ends."""
    if width >= 2 * count:
        return [lo + 1 + i * (width // count) for i in range(count)]
    step = 4 if width >= 16 else 1   # 4 ns apart: the halves of an even n still differ as f32 us
    return [lo + min(max((i - center) * step + width // 2, 0), width - 1) for i in range(count)]


def _last_slot(cx):
    """The push position the compactions reach last."""
    o = T.slot_order(cx.PL, cx.n, cx.m0)
    return int(o[o >= 0][-1])


def _compact_name(cx, k, in_bucket):
    if not cx.full and cx.pad and in_bucket:
        return "compact_masked"
    return "compact_keepbin" if cx.kb and k == 0 else "compact_plain"


def _target(cx, name, prefix, u, n0, r0, pmode, R=R23, tie=False, sib=40, step512=False, top=False):
    """Rank t0 on candidate r0 of the n0 samples of bucket prefix + (u,), reached by len(prefix)
    descents.  pmode, the padding value: out (below the window / in a lower level-0 bucket), above,
    sib (in the window, another bucket), in (the median's bucket), med (= s[t0]), med1 (= s[t1])."""
    tree = Tree(cx.LOG, R)
    k = len(prefix)
    if k >= len(tree.S):
        return None
    e = 1 if cx.even else 0
    if r0 + e >= n0:
        return None
    W = 1 << tree.S[k]
    lo0 = tree.value(list(prefix) + [u])
    if step512:
        cands = [lo0 + 512 * i for i in range(n0)]
        assert cands[-1] < lo0 + W
        if top:
            cands[-1] = lo0 + W - 1
    elif W == 1:
        cands = [lo0] * n0
    else:
        cands = _spread(lo0, W, n0, r0)
    if tie:
        assert n0 >= 8 and 2 <= r0 and r0 + 3 < n0 and W > 1
        for i in range(r0 - 2, r0 + 4):
            cands[i] = cands[r0]
        cands.sort()
    a = b = 0
    if k >= 1:
        a = min(sib, cx.t0 - 1 - r0)
        b = min(sib, cx.n - cx.t0 - 1 - (n0 - r0))
        if a < 1 or b < 1 or a + b + n0 < 65:
            return None
    sa = [tree.value(list(prefix) + [u - 2]) + i % W for i in range(a)]
    sb = [tree.value(list(prefix) + [u + 2]) + i % W for i in range(b)]
    M = sorted(sa) + cands + sorted(sb)
    mid = a + r0
    top0 = prefix[0] if k else u
    P = {"out": (top0 << tree.S[0]) - 5, "above": ((top0 + 1) << tree.S[0]) + 5,
         "sib": sa[0] if sa else None, "in": cands[0] if r0 > 0 else cands[-1],
         "med": cands[r0], "med1": cands[r0 + e]}[pmode]
    if P is None or (pmode == "in" and P in (cands[r0], cands[r0 + e])):
        return None
    last, pins = None, {}
    if n0 == 65 or top:
        # the candidate the compaction reaches last: the smallest of 65 (dropping it moves both
        # ranks up by one), or the one with the top packed key
        val = cands[-1] if top else cands[0]
        at = _last_slot(cx)
        if at == cx.n - 1:
            last = val
        elif at in (0, cx.n // 2):
            return None
        else:
            pins[at] = val
        if P == val:
            return None
    keys = _segment(cx, name, tree, M, mid, P, k, last, pins)
    if keys is None:
        return None
    in_bucket = pmode in ("in", "med", "med1")
    if W == 1:
        final = "one_value"
    elif n0 <= T.CAND:
        final = _compact_name(cx, k, in_bucket)
    else:
        final = "descend"
    pad_at = {"out": "below" if k else "window", "above": "above" if k else "window", "sib": "window"}.get(
        pmode, "bucket")
    want = Want(exits=("descend",) * k + (final,) + ((None,) if final == "descend" else ()), at=k,
                pad_at=pad_at, n0=n0, locs=(tree.where(u, cx.BPL),), hasB=R < 1 << 23, tie=tie or None,
                lane63_top=top)
    s0, s1 = cands[r0], cands[r0 + e]
    wrong = ["distinct_below", "distinct_above"]
    if not tie and W > 1:
        wrong += ["rank_minus", "rank_plus"]
    if e and s0 != s1:
        wrong += ["d1_as_d0", "d0_as_d1"]
    if cx.pad and not tie and W > 1 and (P < s0 or (P == s0 and e and s0 != s1)):
        wrong.append("pad_left_in")
    if n0 == 65:
        wrong.append("n65_as_64")
    return Case(name, keys, want, tuple(wrong))


def _two(cx, name, prefix, b0, b1, pmode, R=R23):
    """s[t0] = hi(b0) - 1 and s[t1] = lo(b1) in different buckets of level len(prefix) (even n).
    pmode, the padding value: lt (a sample below b0), ge (one above b1), t0 (= s[t0]), t1 (= s[t1])."""
    if not cx.even:
        return None
    tree = Tree(cx.LOG, R)
    k = len(prefix)
    W = 1 << tree.S[k]
    a = b = 2
    if k >= 1:
        a, b = min(33, cx.t0), min(33, cx.n - cx.t1 - 1)
        if a + b < 65:
            return None
    x0 = tree.value(list(prefix) + [b0]) + W - 1
    x1 = tree.value(list(prefix) + [b1])
    M = sorted(x0 - min(i, W - 1) for i in range(a)) + [x1 + min(i, W - 1) for i in range(b)]
    top0 = prefix[0] if k else b0
    top1 = prefix[0] if k else b1
    P = {"lt": (top0 << tree.S[0]) - 5, "ge": ((top1 + 1) << tree.S[0]) + 5, "t0": x0, "t1": x1}[pmode]
    keys = _segment(cx, name, tree, M, a - 1, P, k)
    if keys is None:
        return None
    want = Want(exits=("descend",) * k + ("two_buckets",), at=k,
                pad_at="lt_hi0" if pmode in ("lt", "t0") else "ge_lo1",
                locs=(tree.where(b0, cx.BPL), tree.where(b1, cx.BPL)), hasB=R < 1 << 23)
    wrong = ["d1_as_d0", "d0_as_d1", "distinct_below", "distinct_above"]
    if W > 1:
        wrong += ["rank_minus", "rank_plus"]
    if cx.pad and W > 1 and pmode in ("lt", "t0"):
        wrong.append("pad_left_in")
    return Case(name, keys, want, tuple(wrong))


def _one_narrow(cx, name, R):
    """bits <= LOG: shift is 0 at level 0 and every bin is one value."""
    tree = Tree(cx.LOG, R)
    assert tree.S == [0]
    v = R // 2
    M = [v - 1] * 3 + [v] * 4 + [v + 1] * 3
    keys = _segment(cx, name, tree, M, 4, v - 1, 0)
    if keys is None:
        return None
    want = Want(exits=("one_value",), at=0, pad_at="window", n0=4, locs=(tree.where(v, cx.BPL),), hasB=True)
    return Case(name, keys, want, ("distinct_below", "distinct_above") +
                (("pad_left_in",) if cx.pad >= 4 else ()))


def _one_equal(cx, name):
    keys = np.full(cx.n, MN + 123_456, np.uint32)
    want = Want(exits=("one_value",), at=0, pad_at="bucket", n0=cx.n, locs=((0, 0, 0, 0),), hasB=True)
    return Case(name, keys, want, ("b_left_in",))


def _one_deep(cx, name, R):
    """More than 64 copies of the median value between its two neighbours: a descent at every
    level until shift is 0.  The padding is the lower neighbour: inside every window, and in the
    bin next to the median's at the last level."""
    tree = Tree(cx.LOG, R)
    depth = len(tree.S)
    first = 0 if R >= 1 << 24 else 9   # a small magnitude: v - 1, v, v + 1 differ as f32 us
    v = tree.value([first] + [3] * (depth - 2) + [1])
    M = [v - 1] + [v] * 65 + [v + 1]
    keys = _segment(cx, name, tree, M, 33, v - 1, 1)
    if keys is None:
        return None
    want = Want(exits=("descend",) * (depth - 1) + ("one_value",), at=depth - 1, pad_at="window", n0=65,
                locs=(tree.where(1, cx.BPL),), hasB=R < 1 << 23)
    return Case(name, keys, want, ("distinct_below", "distinct_above") +
                (("pad_left_in",) if cx.pad >= 34 else ()))


@lru_cache(maxsize=None)
def build_cases(PL, n, full, kb, m0=0):
    """Every case that fits n samples (all of them from n = 32 PL + 2 up; the 66-sample segments
    of PL 4 have no room for the siblings of a descent)."""
    cx = _ctx(PL, n, full, kb, m0)
    NB, BPL = cx.NB, cx.BPL
    t, u = NB // 2 + 3, NB // 4 + 1
    t24 = NB // 4 + 3            # range 2^23 over 24 bits: only the lower half of the bins is reached
    tl = 9                       # the descents start low: a narrow deep bucket holds values 1 ns apart,
    #                              which differ as f32 microseconds only at a small magnitude
    e = 1 if cx.even else 0
    out = []

    def add(c):
        if c is not None:
            out.append(c)

    # (a) two_buckets: level 0 and 1; adjacent, far apart, one lane, neighbouring lanes, the three
    # row boundaries; the padding below hi0, at or above lo1, equal to s[t0], equal to s[t1]
    add(_two(cx, "a_l0_adjacent_pad_t0", (), t, t + 1, "t0"))
    add(_two(cx, "a_l0_far_pad_t1", (), t, t + 17 * BPL + 1, "t1"))
    if BPL >= 2:
        add(_two(cx, "a_l0_one_lane_pad_lt", (), 6 * BPL, 6 * BPL + 1, "lt"))
    add(_two(cx, "a_l0_next_lane_pad_ge", (), 7 * BPL - 1, 7 * BPL, "ge"))
    for r, pm in ((1, "lt"), (2, "ge"), (3, "t0")):
        add(_two(cx, f"a_l0_row{r}_boundary_pad_{pm}", (), 16 * r * BPL - 1, 16 * r * BPL, pm))
    for pm in ("lt", "ge", "t0", "t1"):
        add(_two(cx, f"a_l1_adjacent_pad_{pm}", (tl,), u, u + 1, pm))
    add(_two(cx, "a_l1_far_pad_t0", (tl,), u, u + 20, "t0"))
    add(_two(cx, "a_l0_top_bucket_pad_lt", (), t, NB - 1, "lt"))

    # (b) one_value: bits <= LOG (bits = LOG, bits = 3, bits = 0) and after every descent
    add(_one_narrow(cx, "b_l0_bits_log", (1 << cx.LOG) - 1))
    add(_one_narrow(cx, "b_l0_bits_3", 7))
    add(_one_equal(cx, "b_l0_all_equal"))
    add(_one_deep(cx, "b_deep_bits32", R32))
    add(_one_deep(cx, "b_deep_bits23", R23))

    # (c) (d) (e) compaction counts and variants, at level 0 and below it, by where the padding is
    r_of = {1: 0, 61: 0, 62: 30, 63: 62 - e, 64: 31, 65: 32}
    for n0 in (1, 61, 62, 63, 64, 65):
        for pm in ("out", "in"):
            add(_target(cx, f"c_l0_n{n0}_pad_{pm}", (), t, n0, r_of[n0], pm))
    add(_target(cx, "c_l0_n64_pad_med", (), t, 64, 31, "med"))
    add(_target(cx, "c_l0_n64_pad_med1", (), t, 64, 31, "med1"))
    add(_target(cx, "c_l0_n64_tie_pad_out", (), t, 64, 31, "out", tie=True))
    add(_target(cx, "c_l0_n64_tie_pad_in", (), t, 64, 31, "in", tie=True))
    for n0 in (1, 63, 64, 65):
        for pm in ("out", "above", "sib", "in"):
            add(_target(cx, f"c_l1_n{n0}_pad_{pm}", (tl,), u, n0, r_of[n0], pm))
    add(_target(cx, "c_l1_n64_pad_med", (tl,), u, 64, 31, "med"))
    add(_target(cx, "c_l1_n62_tie_pad_in", (tl,), u, 62, 30, "in", tie=True))
    # (e) the padding in the median's bucket at level 1 with more than 64 samples: another descent
    add(_target(cx, "e_l2_n64_pad_in", (tl, u), 5, 64, 31, "in"))
    add(_target(cx, "e_l2_n64_pad_med", (tl, u), 5, 64, 31, "med"))
    add(_target(cx, "e_l2_n20_pad_sib", (tl, u), 5, 20, 9, "sib"))

    # (f) the packed rank key at its top: PL 4, shift 26, 64 candidates, the largest at bucket
    # offset 2^26 - 1 compacted last (lane 63): its key is the idle lanes' 0xFFFFFFFF
    if PL == 4:
        add(_target(cx, "f_top_key_lane63", (), 1, 64, 63 - e, "out", R=R32, step512=True, top=True))

    # (g) the median's bucket: every row, first / last bin of a lane, bucket 0, bucket NB - 1
    for r in (0, 1, 2, 3):
        first = (16 * r + 2) * BPL
        add(_target(cx, f"g_row{r}_first_bin", (), first, 64, 31, "out"))
        add(_target(cx, f"g_row{r}_last_bin", (), first + 3 * BPL + BPL - 1, 64, 31, "in"))
    add(_target(cx, "g_row_start_lane16", (), 16 * BPL, 33, 16, "out"))
    add(_target(cx, "g_bucket0_then_l1", (0,), u, 64, 31, "above"))
    add(_target(cx, "g_top_bucket_then_l1", (NB - 1,), u, 64, 31, "out"))

    # (h) range 2^23 (B = 0, bits 24) beside the default 2^23 - 1 (B = 0x4B000000, wlo starts at B)
    for n0, pm in ((64, "in"), (65, "in"), (64, "out"), (63, "sib")):
        add(_target(cx, f"h_r24_l1_n{n0}_pad_{pm}", (tl,), u, n0, r_of[n0], pm, R=R24))
    add(_two(cx, "h_r24_l1_two_pad_t0", (tl,), u, u + 1, "t0", R=R24))
    add(_target(cx, "h_r24_l0_n64_pad_med", (), t24, 64, 31, "med", R=R24))

    names = [c.name for c in out]
    assert len(names) == len(set(names))
    return tuple(out)


# ------------------------------------------------------------------ what a trace must show
def unmet(tr, want):
    """What the trace does not show of a Want (empty: met)."""
    bad = []
    exits = [v.exit for v in tr.visits]
    w = list(want.exits)
    if w and w[-1] is None:
        w.pop()
        exits = exits[:len(w)]
        if len(tr.visits) <= len(w):
            bad.append("no visit after the descents")
    if len(exits) != len(w) or any(not g.startswith(x) for g, x in zip(exits, w)):
        bad.append(("exits", exits, want.exits))
        return bad
    v = tr.visits[want.at]
    if want.n0 is not None and v.n0 != want.n0:
        bad.append(("n0", v.n0, want.n0))
    if (want.pad_at if tr.pad else "none") != v.pad_at:
        bad.append(("pad_at", v.pad_at, want.pad_at))
    if want.locs is not None:
        got = tuple((l.row, l.lane, l.j, l.ba) for l in v.locs)
        if got != tuple(want.locs):
            bad.append(("locs", got, want.locs))
    if want.hasB is not None and tr.hasB != want.hasB:
        bad.append(("B", tr.hasB))
    if want.tie and not (v.tie0 and v.tie1 and tr.d0 == tr.d1):
        bad.append("tie")
    if want.lane63_top:
        lo0 = v.wlo + (v.locs[0].ba << v.shift)
        if not (v.L1 == 63 and (((v.cands[63] - lo0) << 6) | 63) == T.M32 and v.shift == 26):
            bad.append(("lane63", v.L1))
    return bad


# ------------------------------------------------------------------ sensitivity
def med_us(k0, k1, n):
    """MED as the kernels and the oracle form it: f32(ns) / 1000, the two middle samples averaged
    in f32 for even n."""
    f = (np.array([k0, k1], np.uint32).astype(np.float32) / np.float32(1000)).astype(np.float32)
    return f[0] if n & 1 else np.float32((f[0] + f[1]) / np.float32(2))


def wrong_answers(keys, tr):
    """name -> MED (f32 us) a sloppy version of the select would return; absent where the sloppy
    version has nothing to return for this segment."""
    k = np.asarray(keys, np.uint32).astype(np.int64)
    n = k.size
    s = np.sort(k)
    t0, t1 = (n // 2 if n & 1 else n // 2 - 1), n // 2
    out = {}
    if t0 >= 1:
        out["rank_minus"] = med_us(s[t0 - 1], s[t1 - 1], n)      # `<=` for `<` in a rank or a prefix
    if t1 + 1 < n:
        out["rank_plus"] = med_us(s[t0 + 1], s[t1 + 1], n)
    lo, hi = s[s < s[t0]], s[s > s[t1]]
    if lo.size:                                                   # a whole run of ties skipped
        out["distinct_below"] = med_us(lo[-1], lo[-1] if s[t1] == s[t0] else s[t0], n)
    if hi.size:
        out["distinct_above"] = med_us(hi[0] if s[t1] == s[t0] else s[t1], hi[0], n)
    if n % 2 == 0:
        out["d1_as_d0"] = med_us(s[t0], s[t0], n)                 # the second locate / readlane dropped
        out["d0_as_d1"] = med_us(s[t1], s[t1], n)
    if tr.pad:                                                    # the padding's copies never taken out
        sp = np.sort(np.concatenate([k, np.full(tr.pad, tr.pad_key, np.int64)]))
        out["pad_left_in"] = med_us(sp[t0], sp[t1], n)
    out["b_left_in"] = med_us((s[t0] + T.B23) & T.M32, (s[t1] + T.B23) & T.M32, n)   # d0 - B forgotten
    for v in tr.visits:                                           # 65 candidates treated as 64
        if v.exit == "descend" and v.n0 == 65:
            lanes = np.array(v.cands[:64], np.int64)              # what fits the wave, in LDS order
            below_bucket = int((s - tr.mn < min(v.cands)).sum())
            r0, r1 = t0 - below_bucket, t1 - below_bucket
            if 0 <= r0 and r1 < 64:
                c = np.sort(lanes) + tr.mn
                out["n65_as_64"] = med_us(c[r0], c[r1], n)
    return out


def insensitive(case, tr):
    """The wrong answers of the case that coincide with the right MED (must be empty)."""
    right = med_us(tr.mn + tr.d0, tr.mn + tr.d1, tr.n)
    got = wrong_answers(case.keys, tr)
    return [w for w in case.wrong if w not in got or got[w].view(np.uint32) == right.view(np.uint32)]


# ------------------------------------------------------------------ lengths
def lengths(PL, masked):
    """The retained lengths of a class: both parities, a large and a small padding; PL 4 also the
    66-sample segment whose 190 padding copies outnumber it (strided only: a ragged segment of
    up to 128 samples runs a lane class)."""
    return (32 * PL + 2, 64 * PL - 4, 64 * PL - 1) if masked else (64 * PL,)


SHORT_PL4 = 66
