"""Segments built to order for the branches of csrc/segment_quantiles.hip (numpy, no GPU).

wave_case(name, n, m0), gt26(n, m0) and stream_case(name, n, m0) return six segments of n keys for a wave class (m0: the segment's offset in
its first 16-byte vector, which with n fixes the class and so the histogram's fan-out), the
permille list of the launch, and per segment the visits its trace (tests/_quantile_trace.py) must
show.  tests/test_quantile_trace_cpu.py checks those on the CPU; tests/test_gpu_quantile_branches.py
runs the same segments on the GPU against np.sort.

Layout of the register-path cases.  Every segment spans d = key - MN in [0, 2^23): 23 bits, so
every key is below 2^24 and distinct keys convert to distinct float32 microseconds.  A histogram
level takes LOG bits, so a value is a tuple of digits, one per level (level_shifts), and a bin at
level i is a prefix of i digits:
    A     `na` copies of one value (digits t, 5, [3,] 1): a window of more than 64 at every level
    A-1, A+1  one sample each: they share A's window down to the last level
    B     66 copies of A's value with another last digit: leaves A's window at the last level only
    C     20 values under the prefix (t, 9): leaves at the second level, into a compaction
    E     64 or 65 values under the prefix (t, 12)
    U     30 values under the prefix (u): leaves at the first level, into a compaction
    X, Y  64 and 65 values under the prefixes (x) and (x + 1), or (x, 7) and (x, 8)
    0 and 2^23 - 1, and filler in first-level bins no block uses
"""
from collections import namedtuple

import numpy as np

import _quantile_trace as T

BITS = 23
MN = 1000
PM = (0, 1, 250, 500, 900, 990, 999, 1000)        # tests/test_gpu_quantiles.py PM
DESC_REPEATS = (1000, 990, 990, 500, 500, 0, 250)  # its REQUESTS["repeats_descending"]
SPREAD = (0, 140, 285, 430, 570, 715, 860, 1000)

# the table of the issue: per class a length just above its lower edge and its upper edge
CLASS_LENGTHS = {4: (200, 256), 8: (260, 512), 16: (520, 1024), 32: (1030, 2048), 64: (2060, 4096),
                 128: (4100, 8192)}
TABLE_LENGTHS = [n for pair in CLASS_LENGTHS.values() for n in pair]
BEGINS = (0, 3)
WAVE_CASES = ("j_deep", "k_pad_deep", "k_pad_ends", "l_boundary", "n_equal", "n_bins", "n_repeats")
GT26_LENGTHS = (2, 33, 64, 65, 200)
STREAM_LENGTHS = (8193, 9001)
STREAM_CASES = ("o_last_byte", "o_top_bytes", "o_merge_split", "o_equal")

Case = namedtuple("Case", "segs pm wants")
# a visit the trace must show.  exit: a name or a prefix ("compact"); level: the least level;
# count / nranks: exact when given; first: it is the first visit; needs_pad: only a segment with
# padding (pad > 0) can show it
Want = namedtuple("Want", "exit level padin count nranks first needs_pad",
                  defaults=(1, None, None, None, False, False))
# the streaming kernel: per pass the set of rank groups sharing a histogram
Shares = namedtuple("Shares", "per_pass")


def matches(v, w):
    return (v.exit.startswith(w.exit) and v.level >= w.level and (w.padin is None or v.padin == w.padin)
            and (w.count is None or v.count == w.count) and (w.nranks is None or len(v.ranks) == w.nranks))


def unmet(trace, wants):
    """The wants the trace does not show (a segment without padding is excused from needs_pad)."""
    out = []
    for w in wants:
        if isinstance(w, Shares):
            got = [frozenset(p.share) for p in trace.passes]
            if got != [frozenset(s) for s in w.per_pass]:
                out.append((w, got))
        elif w.needs_pad and trace.pad == 0:
            continue
        elif not any(matches(v, w) for v in (trace.visits[:1] if w.first else trace.visits)):
            out.append(w)
    return out


# ------------------------------------------------------------------ the digit tree
def level_shifts(LOG):
    """s2 of every histogram level of a 23-bit range: [17, 11, 5, 0] for LOG 6."""
    s, out = BITS, []
    while s > 0:
        s = s - LOG if s > LOG else 0
        out.append(s)
    return out


class Tree:
    def __init__(self, LOG):
        self.S = level_shifts(LOG)
        self.NB = 1 << LOG
        assert len(self.S) >= 3 and BITS - self.S[0] == LOG

    def value(self, digits, low=0):
        """The value with these leading digits and `low` in the bits below them."""
        prev, d = BITS, 0
        for dig, s in zip(digits, self.S):
            assert 0 <= dig < 1 << (prev - s)
            d |= dig << s
            prev = s
        assert 0 <= low < 1 << prev
        return d | low

    def leaf(self, digits):
        """A full-depth value: the given digits, 3s in between, the last digit last."""
        head = list(digits[:-1])[:len(self.S) - 1]
        return self.value(head + [3] * (len(self.S) - 1 - len(head)) + [digits[-1]])

    def cluster(self, digits, count, rng):
        free = self.S[len(digits) - 1]
        return self.value(digits) + rng.integers(0, 1 << free, size=count)

    def filler(self, count, total, reserved, rng):
        """`count` values in first-level bins outside `reserved`: the first of `total` draws, so
        layouts that differ by a sample or two share all but that many."""
        tops = np.array([b for b in range(self.NB) if b not in reserved])
        v = (rng.choice(tops, size=total) << self.S[0]) + rng.integers(0, 1 << self.S[0], size=total)
        return v[:count]


def assemble(tree, blocks, n, reserved, seed):
    rng = np.random.default_rng(seed)
    parts = [np.asarray(b, np.int64) for b in blocks] + [np.array([0, (1 << BITS) - 1])]
    used = sum(p.size for p in parts)
    assert used <= n, (used, n)
    d = np.concatenate(parts + [tree.filler(n - used, n, reserved, rng)])
    assert d.size == n and d.min() == 0 and d.max() == (1 << BITS) - 1
    return d


def arrange(d, x0, order, seed, base=MN):
    """The keys in push order: one sample of value x0 first (None: whatever the order puts there),
    the others shuffled, ascending or descending."""
    rng = np.random.default_rng(seed)
    d = np.sort(d)
    if order == "shuffle":
        d = rng.permutation(d)
    elif order == "desc":
        d = d[::-1].copy()
    if x0 is not None:
        at = int(np.nonzero(d == x0)[0][0])
        d = np.concatenate([[x0], d[:at], d[at + 1:]])
    return (base + d).astype(np.uint32)


def pm_into(n, d, lo, hi):
    """A permille whose rank lands on a sample with lo <= d <= hi, nearest the middle of them."""
    s = np.sort(d)
    a, b = int(np.searchsorted(s, lo, "left")), int(np.searchsorted(s, hi, "right")) - 1
    assert a <= b
    best = min(range(1001), key=lambda p: abs((p * (n - 1)) // 1000 - (a + b) / 2))
    assert a <= (best * (n - 1)) // 1000 <= b, (n, a, b)
    return best


ORDERS = ("shuffle", "shuffle", "asc", "desc", "shuffle", "shuffle")


def _tree_for(n, m0):
    PL = T.wave_class(n, m0)
    NB, LOG = T.bins(PL)
    tr = Tree(LOG)
    t, u, x = NB // 2 + 3, NB // 4 + 1, NB // 8 + 2
    return tr, t, u, x


def _span(tree, digits):
    lo = tree.value(digits)
    return lo, lo + (1 << tree.S[len(digits) - 1]) - 1


def _deep_blocks(tr, t, u, rng, na=70, with_b=True, ne=0):
    a = tr.leaf((t, 5, 1))
    blocks = [np.full(na, a), [a - 1, a + 1], tr.cluster((t, 9), 20, rng), tr.cluster((u,), 30, rng)]
    if with_b:
        blocks.append(np.full(66, tr.leaf((t, 5, 3))))
    if ne:
        blocks.append(tr.cluster((t, 12), ne, rng))
    return a, blocks


def j_deep(n, m0, pm=None):
    """(j) the window of A holds more than 64 samples at every level until sh == 0."""
    tr, t, u, _ = _tree_for(n, m0)
    a, blocks = _deep_blocks(tr, t, u, np.random.default_rng(n))
    d = assemble(tr, blocks, n, {t, u}, seed=n + 1)
    b = tr.leaf((t, 5, 3))
    if pm is None:
        s = np.sort(d)
        at = int(np.searchsorted(s, a))
        # two ranks inside A (the permilles nearest its first and last third)
        pa1 = min(range(1001), key=lambda p: abs((p * (n - 1)) // 1000 - (at + 20)))
        pa2 = min(range(1001), key=lambda p: abs((p * (n - 1)) // 1000 - (at + 50)))
        pm = (pa1, pa2, pm_into(n, d, b, b), pm_into(n, d, *_span(tr, (t, 9))),
              pm_into(n, d, *_span(tr, (u,))), 0, 1000)
        assert all(s[r] == a for r in T.ranks(n, (pa1, pa2)))
    depth = len(tr.S)
    wants = [Want("one_value", depth + 1, nranks=2),         # two ranks in A down to the last level
             Want("histogram", depth, nranks=3),             # A, A and B still together there
             Want("one_value", depth + 1, nranks=1),         # B
             Want("compact", 3, count=20, nranks=1),         # C: left at the second level
             Want("compact", 2, count=30, nranks=1)]         # U: left at the first level
    segs = [arrange(d, None, o, seed=10 * n + i) for i, o in enumerate(ORDERS)]
    return Case(segs, pm, [wants for _ in segs])


def k_pad_deep(n, m0):
    """(k) sample 0 (the padding) deep in the tree: equal to, one below and one above A; equal to
    a requested order statistic of C (a compaction); one of E's 64 / 65 values."""
    tr, t, u, _ = _tree_for(n, m0)
    depth = len(tr.S)
    segs, wants = [], []
    for i in range(6):
        ne = 64 if i == 4 else 65
        a, blocks = _deep_blocks(tr, t, u, np.random.default_rng(n), with_b=False, ne=ne)
        d = assemble(tr, blocks, n, {t, u}, seed=n + 1)
        if i == 0:
            pc = pm_into(n, d, *_span(tr, (t, 9)))
            pm = (pm_into(n, d, a, a), pc, pm_into(n, d, *_span(tr, (u,))),
                  pm_into(n, d, *_span(tr, (t, 12))), 0, 1000, pm_into(n, d, a + 1, (1 << BITS) - 2))
        s = np.sort(d)
        if i < 3:
            x0 = (a, a - 1, a + 1)[i]
            w = [Want("histogram", depth, padin=True, needs_pad=True), Want("one_value", depth + 1)]
        elif i == 3:
            x0 = int(s[(pc * (n - 1)) // 1000])
            w = [Want("compact", 3, padin=True, count=20, needs_pad=True)]
        else:
            x0 = int(s[(pm[3] * (n - 1)) // 1000])
            w = [Want("compact", 3, padin=True, count=64, needs_pad=True) if i == 4 else
                 Want("histogram", 3, padin=True, count=65, needs_pad=True)]
        segs.append(arrange(d, x0, "shuffle", seed=20 * n + i))
        wants.append(w)
    return Case(segs, pm, wants)


def k_pad_ends(n, m0):
    """(k) sample 0 as MIN and as MAX (the padding leaves the windows of the deep ranks at the
    first level), and as a requested order statistic of U (a compaction at the second level)."""
    tr, t, u, _ = _tree_for(n, m0)
    depth = len(tr.S)
    a, blocks = _deep_blocks(tr, t, u, np.random.default_rng(n), with_b=False, ne=65)
    d = assemble(tr, blocks, n, {t, u}, seed=n + 1)
    pu = pm_into(n, d, *_span(tr, (u,)))
    pm = (pm_into(n, d, a, a), pm_into(n, d, *_span(tr, (t, 9))), pu, 0, 1000, 1, 999)
    xu = int(np.sort(d)[(pu * (n - 1)) // 1000])
    deep = Want("histogram", depth, padin=False)
    segs, wants = [], []
    for i, (x0, order) in enumerate(((0, "shuffle"), ((1 << BITS) - 1, "shuffle"), (xu, "shuffle"),
                                     (0, "asc"), ((1 << BITS) - 1, "desc"), (xu, "shuffle"))):
        segs.append(arrange(d, x0, order, seed=30 * n + i))
        wants.append([deep, Want("histogram", 1, padin=True, first=True, needs_pad=True)] +
                     ([Want("compact", 2, padin=True, count=30, needs_pad=True)] if x0 == xu else
                      [Want("compact", 2, padin=True, needs_pad=True)]))
    return Case(segs, pm, wants)


def l_boundary(n, m0):
    """(l) exactly 64 and exactly 65 samples in a window, after the first level (prefixes (x) and
    (x + 1)) and after the second ((x, 7) and (x, 8)); as distinct-ish values and as 64 / 65
    copies of one value; with the padding inside the window of 64."""
    tr, _, _, x = _tree_for(n, m0)
    segs, wants = [], []
    pm = None
    for i in range(6):
        rng = np.random.default_rng(n + 5)
        deep, equal, padded = i in (2, 3, 5), i in (1, 3), i in (4, 5)
        px, py = ((x, 7), (x, 8)) if deep else ((x,), (x + 1,))
        if equal:
            bx, by = np.full(64, tr.leaf(px + (2, 1))), np.full(65, tr.leaf(py + (2, 1)))
        else:
            bx, by = tr.cluster(px, 64, rng), tr.cluster(py, 65, rng)
        d = assemble(tr, [bx, by], n, {x, x + 1}, seed=n + 1)
        if pm is None:
            s = np.sort(d)
            at = int(np.searchsorted(s, tr.value((x,))))
            near = lambda r: min(range(1001), key=lambda p: abs((p * (n - 1)) // 1000 - r))  # noqa: E731
            pm = (near(at + 10), near(at + 50), near(at + 64 + 10), near(at + 64 + 50), 0, 1000)
            assert [(p * (n - 1)) // 1000 - at < 64 for p in pm[:4]] == [True, True, False, False]
            assert all(at <= (p * (n - 1)) // 1000 < at + 129 for p in pm[:4])
        lev = 3 if deep else 2
        w = [Want("compact_le26", lev, count=64, nranks=2, padin=padded or None, needs_pad=padded),
             Want("histogram", lev, count=65, nranks=2)]
        if equal:
            w.append(Want("one_value", lev + 1, count=65, nranks=2))
        segs.append(arrange(d, int(bx[3]) if padded else None, ORDERS[i], seed=40 * n + i))
        wants.append(w)
    return Case(segs, pm, wants)


def n_equal(n, m0):
    """(n) all eight permilles equal, on the deep data: one group in every visit."""
    c = j_deep(n, m0)
    pm = (c.pm[0],) * 8
    depth = len(level_shifts(T.bins(T.wave_class(n, m0))[1]))
    return Case(c.segs, pm, [[Want("histogram", 1, nranks=8, first=True),
                              Want("one_value", depth + 1, nranks=8)] for _ in c.segs])


def n_bins(n, m0):
    """(n) eight ranks in eight different first-level bins: a ramp over the 23 bits."""
    d = (np.arange(n, dtype=np.int64) * ((1 << BITS) - 1)) // (n - 1)
    segs = [arrange(d, None, o, seed=50 * n + i) for i, o in enumerate(ORDERS)]
    return Case(segs, SPREAD, [[Want("histogram", 1, nranks=8, first=True)] for _ in segs])


def n_repeats(n, m0):
    """(n) the descending request with repeats, on the deep data."""
    c = j_deep(n, m0, pm=DESC_REPEATS)
    return Case(c.segs, DESC_REPEATS, [[Want("histogram", 1, nranks=7, first=True),
                                        Want("", 2, nranks=2)] for _ in c.segs])


def wave_case(name, n, m0):
    return {"j_deep": j_deep, "k_pad_deep": k_pad_deep, "k_pad_ends": k_pad_ends,
            "l_boundary": l_boundary, "n_equal": n_equal, "n_bins": n_bins, "n_repeats": n_repeats}[name](n, m0)


# ------------------------------------------------------------------ (m) key ranges above 2^26
def gt26(n, m0):
    """(m) n keys over a range above 2^26, ties included: multiples of 512 (4096 for the range
    above 2^31), so distinct keys stay distinct as float32 microseconds.  n <= 64: the one visit is
    a compaction with sh > 26; longer segments take a histogram level first."""
    segs = []
    for i in range(6):
        rng = np.random.default_rng(1000 * n + i)
        if i == 4:    # bits = 32: the window mask is all ones
            v = rng.integers(0, 0xD0000000 >> 12, size=n) << 12
            lo, hi = 4096, 0xD0000000
        elif i == 5:  # two clusters 2^26 apart and more: (d << 6) would wrap and reorder them
            v = np.where(rng.random(n) < 0.5, 0, 1 << 26) + (rng.integers(0, 64, size=n) << 9)
            lo, hi = 0, (1 << 27) + 512
        else:
            pool = rng.integers(0, 1 << 21, size=5 if i == 1 else n) << 9
            v = rng.choice(pool, size=n)
            lo, hi = 512, 1 << 30
        p, q = (0, 1) if i == 2 or n == 2 else (1, 0) if i == 3 else (n // 2, n - 1)
        v[p], v[q] = lo, hi       # sample 0 is MIN (i == 2) or MAX (i == 3)
        assert hi - lo > 1 << 26
        segs.append((MN + v).astype(np.uint32))
    first = (Want("compact_gt26", 1, padin=True, count=n, nranks=8, first=True) if n <= T.QCAND else
             Want("histogram", 1, padin=True, count=n, nranks=8, first=True))
    return Case(segs, PM, [[first] for _ in segs])


# ------------------------------------------------------------------ (o) the streaming kernel
def stream_case(name, n, m0):
    q = n // 4
    if name == "o_last_byte":    # one prefix for three passes, eight different last bytes
        d = 0xABCD00 + (np.arange(n, dtype=np.int64) * 256) // n
        pm, shares = SPREAD, [[tuple(range(8))]] * 4
    elif name == "o_top_bytes":  # eight different top bytes, the keys multiples of 4096 below them
        tops = np.array([0x00, 0x01, 0x10, 0x3F, 0x40, 0x7F, 0x80, 0xDF], np.int64)
        rng = np.random.default_rng(n)
        d = (tops[(np.arange(n) * 8) // n] << 24) | (rng.integers(0, 1 << 12, size=n) << 12)
        pm = (62, 187, 312, 437, 562, 687, 812, 937)
        shares = [[tuple(range(8))]] + [[(r,) for r in range(8)]] * 3
    elif name == "o_merge_split":
        # ranks 0, 2, 4, 6 in the lower half (byte 2 = 0x10), 1, 3, 5, 7 in the upper (0x20); the
        # lower half splits again on byte 1 (ranks 0, 2 | 4, 6); the last byte tells all apart
        i = np.arange(n, dtype=np.int64)
        b2 = np.where(i < 2 * q, 0x10, 0x20)
        b1 = np.where(i < q, 1, np.where(i < 2 * q, 2, 7))
        d = (b2 << 16) | (b1 << 8) | ((i * 256) // n)
        pm = (100, 600, 200, 700, 300, 800, 400, 900)
        shares = [[tuple(range(8))], [tuple(range(8))], [(0, 2, 4, 6), (1, 3, 5, 7)],
                  [(0, 2), (4, 6), (1, 3, 5, 7)]]
    else:                        # o_equal
        d = np.full(n, 0x345678, np.int64)
        pm, shares = PM, [[tuple(range(8))]] * 4
    segs = [arrange(d, None, o, seed=60 * n + i, base=0) for i, o in enumerate(ORDERS)]
    return Case(segs, pm, [[Shares(shares)] for _ in segs])


def strided(segs, begin):
    """The six segments at [begin, begin + n) of a stride that is a multiple of 4, so every one
    starts begin slots into a 16-byte vector; the slots between them hold a key no segment has."""
    n = len(segs[0])
    stride = (begin + n + 3) // 4 * 4 + 4
    host = np.full(len(segs) * stride, 0xDEAD0000, np.uint32)
    for s, keys in enumerate(segs):
        host[s * stride + begin: s * stride + begin + n] = keys
    return host, stride
