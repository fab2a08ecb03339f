"""Dispatch model of the ragged statistics (csrc/segment_ragged*.hip, segment_addr.h): plain Python,
no torch, no GPU.

Two sides decide what happens to a ragged segment.  The classifier sorts it into one of 13
length classes from its own retained length (`seg_class`).  The host launches class kernels from
the caller's `max_len` hint and `cap` alone (`launched`, `exact_variant`).  A segment whose class
is not launched sits in a list no kernel reads: its output row is never written and nothing
reports it.  tests/test_ragged_model_cpu.py proves on this model that the two sides agree
(closure), tests/test_gpu_ragged_classes.py ties `seg_class` to the product function through
tests/native/ragged_class.hip and runs the device at every edge `gate_keeps` finds.

These restate the product by hand; a threshold that changes there is changed here by hand, and
`gate_keeps` (a scan, not a list) then moves the test cases with it."""
from collections import namedtuple
from functools import lru_cache

CLASSES = ("T8", "T16", "T32", "T64", "T128",         # lane classes: one lane per segment
           "W4", "W8", "W16", "W32", "W64", "W128",   # wave classes (PL): one wave per segment
           "X",                                       # workgroup class: the EXACT kernels
           "F")                                       # FULL: FAST, aligned, exactly 64 * PL samples
LANE = CLASSES[:5]
WAVE = CLASSES[5:11]
LANE_N = {"T8": 8, "T16": 16, "T32": 32, "T64": 64, "T128": 128}
WAVE_PL = {"W4": 4, "W8": 8, "W16": 16, "W32": 32, "W64": 64, "W128": 128}
FULL_LENS = (1024, 2048, 4096, 8192)    # 64 * PL, PL 16..128
LDS_SEGMENT = 32768                     # NVRX_LDS_SEGMENT (nvrx_internal.h)
MAX_SEGMENT = 1 << 30                   # NVRX_MAX_SEGMENT (nvrx_straggler.h)
XG_CHUNK = 8192                         # segment_sorted.h
CLS_THREADS = 1024                      # segment_ragged.hip: the classifier's block
CLS_MAX_BLOCKS = 1024
SCAN_KEEPS = 70000                      # gate_keeps scans keep = 1..SCAN_KEEPS


def keep_of(length, cap):
    """Retained length of a ring of `length` pushes (segment_addr.h seg_keep; cap <= 0: all)."""
    return cap if cap > 0 and length > cap else length


def full_len(keep, aligned16, exact):
    """The FULL length of a launch whose longest retained run is `keep` (0: none)."""
    return keep if not exact and aligned16 and keep in FULL_LENS else 0


def _clog2(n):
    """ceil(log2 n) as 32 - clz(n - 1) computes it (0 for n = 1)."""
    return (n - 1).bit_length()


def seg_class(n, aligned16, exact, full_n):
    """Class of a segment of n >= 1 retained samples (segment_ragged_kernels.h seg_class)."""
    if n <= 128:
        return CLASSES[max(_clog2(n), 3) - 3]
    if exact:
        return "X"
    if n == full_n:
        return "F"
    need = n if aligned16 else n + 3
    lg = _clog2(need)
    return CLASSES[lg - 3] if lg <= 13 else "X"


def launched(max_len, cap, aligned16, exact):
    """The classes ragged_launch_classes launches for the hint (segment_ragged.hip)."""
    keep = keep_of(max_len, cap)
    need = keep if aligned16 else keep + 3
    out = set()
    if not exact and full_len(keep, aligned16, exact):
        out.add("F")
    if (keep > 128) if exact else (need > 64 * 128):
        out.add("X")
    if not exact:
        if keep > 128:
            out.add("W4")
        for c in WAVE[1:]:
            if need > 64 * (WAVE_PL[c] // 2):
                out.add(c)
    for c in LANE:
        if c == "T8" or keep > LANE_N[c] // 2:
            out.add(c)
    return frozenset(out)


def exact_global_np2(max_len):
    """Scratch elements per block of the long-ring EXACT kernel (segment_sorted.h)."""
    np2 = XG_CHUNK
    while np2 < max_len:
        np2 <<= 1
    return np2


Variant = namedtuple("Variant", "kernel np2")


def exact_variant(keep):
    """The EXACT kernel ragged_launch_exact picks for a launch of longest retained run `keep`
    (segment_ragged_big.hip); np2 only for the global-memory kernel."""
    if keep <= 1024:
        return Variant("lds1024", None)
    if keep <= 8192:
        return Variant("lds8192", None)
    if keep <= LDS_SEGMENT:
        return Variant("lds32768", None)
    assert keep <= MAX_SEGMENT
    return Variant("global", exact_global_np2(keep))


def gate_keeps(aligned16, exact):
    """{class: [(closed_keep, open_keep), ...]} -- see `_gate_scan` (scanned once per process)."""
    return {c: list(pairs) for c, pairs in _gate_scan(bool(aligned16), bool(exact))}


@lru_cache(maxsize=None)
def _gate_scan(aligned16, exact):
    """{class: [(closed_keep, open_keep), ...]}: for every launch gate, each pair of neighbouring
    keeps between which the gate changes -- the larger of a closed run and the smaller of the
    open run next to it, in either order of appearance.  Found by scanning `launched` over
    keep = 1..SCAN_KEEPS (cap 0), never typed in.  T8 has no gate (always launched)."""
    gates = {}
    prev = launched(1, 0, aligned16, exact)
    for keep in range(2, SCAN_KEEPS + 1):
        cur = launched(keep, 0, aligned16, exact)
        for c in prev ^ cur:
            gates.setdefault(c, []).append((keep - 1, keep) if c in cur else (keep, keep - 1))
        prev = cur
    return tuple((c, tuple(pairs)) for c, pairs in gates.items())


def all_gate_keeps(aligned16, exact):
    """Every keep next to a gate change, ascending."""
    return sorted({k for pairs in gate_keeps(aligned16, exact).values() for p in pairs for k in p})


@lru_cache(maxsize=None)
def reachable(aligned16, exact):
    """The classes some launch of this (aligned16, mode) can populate."""
    out = set()
    for keep in range(1, SCAN_KEEPS + 1):
        fn = full_len(keep, aligned16, exact)
        out.add(seg_class(keep, aligned16, exact, fn))
    return frozenset(out)


@lru_cache(maxsize=None)
def class_edges(aligned16, exact, upto=SCAN_KEEPS):
    """Every retained length n <= upto at which seg_class changes between n - 1 and n (with and
    without n as the FULL length), both sides: the class-boundary lengths."""
    edges = {1}
    for fn in (0,) + FULL_LENS:
        prev = seg_class(1, aligned16, exact, fn)
        for n in range(2, upto + 1):
            cur = seg_class(n, aligned16, exact, fn)
            if cur != prev:
                edges.update((n - 1, n))
            prev = cur
    return tuple(sorted(edges))


def expect_exact_bits(keep_s, aligned16, exact):
    """Whether AVG / STD of a segment of keep_s retained samples must carry the reference's bits:
    the lane classes (the reference's sequential f32 sums), EXACT mode, and anything the FAST
    classifier sends to the workgroup class.  NUM / MIN / MAX / MED are bit-exact everywhere."""
    return exact or keep_s <= 128 or seg_class(keep_s, aligned16, False, 0) == "X"


def classifier_blocks(nseg):
    """(nblocks, chunk) of the classifier launches: block b classifies segments
    [b * chunk, min(nseg, (b + 1) * chunk))."""
    nblocks = min(CLS_MAX_BLOCKS, (nseg + CLS_THREADS - 1) // CLS_THREADS)
    return nblocks, (nseg + nblocks - 1) // nblocks
