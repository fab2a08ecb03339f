"""The launches of tests/test_gpu_ragged_classes.py as data (numpy, no torch, no GPU): segment
lengths, cap, hint, alignment promise and mode of every case, built from the dispatch model
(tests/_ragged_model.py), and `coverage()`, which proves on the model that the cases reach every
class, both sides of every launch gate and every EXACT kernel.  tests/test_ragged_model_cpu.py
runs `coverage()` without a GPU: a case list that has gone incomplete fails there first.

A length of 0 is an empty segment (the classifier writes num 0 and NaN), a length of -1 a skipped
one (outputs untouched); the offsets form (`form == "off"`, seg_len NULL) cannot express a skip."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import _ragged_model as M

Case = namedtuple("Case", "name group lens cap max_len aligned16 exact form dup colref")
PARAMS = [(a, e) for a in (False, True) for e in (False, True)]  # (aligned16, exact)
CAPS = (8, 128, 129, 1024, 8192)
CAP_HINT = 50000
EXACT_EDGES = (129, 1024, 1025, 8192, 8193, 32768, 32769, 65536, 65537)
FAST_X_EDGES = (8189, 8190, 8192)   # FAST, not aligned: need = n + 3 crosses 8192 slots
NSEGS = (1, 1023, 1024, 1025, 8 * 1024 + 1, 65 * 1024 + 3)
COPIES_UPTO = 1100                  # three copies (three 4-byte phases) of every length up to here


def tag(aligned16, exact):
    return f"{'aligned' if aligned16 else 'unaligned'}-{'EXACT' if exact else 'FAST'}"


def _case(name, group, lens, cap, max_len, aligned16, exact, form="len", dup=(), colref=0):
    lens = np.asarray(lens, np.int64)
    if form == "off":
        lens = np.maximum(lens, 0)
    assert lens.size and int(lens.max()) <= max_len  # the contract: the hint bounds every length
    return Case(name, group, lens, cap, max_len, aligned16, exact, form, tuple(dup), colref)


def kept(case):
    """Retained length per segment (0 empty, < 0 skipped)."""
    return np.where((case.cap > 0) & (case.lens > case.cap), case.cap, case.lens)


def populated(case):
    """The classes the classifier puts a segment of this case into."""
    keep = M.keep_of(case.max_len, case.cap)
    fn = M.full_len(keep, case.aligned16, case.exact)
    k = kept(case)
    return frozenset(M.seg_class(int(n), case.aligned16, case.exact, fn) for n in np.unique(k[k > 0]))


def case_launched(case):
    return M.launched(case.max_len, case.cap, case.aligned16, case.exact)


def _edges(aligned16, exact):
    return M.class_edges(aligned16, exact)


def _interleave(lens):
    """A few empty and skipped segments between the others."""
    out = []
    for i, n in enumerate(lens):
        out.append(n)
        if i % 10 == 3:
            out.append(0)
        if i % 15 == 7:
            out.append(-1)
    return out


def _boundary_lens(upto, aligned16, exact, extra=()):
    lens = sorted({n for n in _edges(aligned16, exact) if n <= upto} | {n for n in extra if n >= 1})
    return [n for n in lens for _ in range(3 if n <= COPIES_UPTO else 1)]


# ------------------------------------------------------------------ (a) every gate, both sides
def gate_case(keep, aligned16, exact, form="len"):
    """max_len = keep exactly, cap 0: every class-boundary length <= keep, keep - 1 and keep."""
    lens = _boundary_lens(keep, aligned16, exact, extra=(keep - 1, keep))
    if form == "off" and aligned16:
        # offsets form: segment s + 1 starts where s ends, so 16-byte aligned starts need lengths
        # that are multiples of 4 (empty segments included, skipped ones impossible)
        lens = [n for n in lens if n % 4 == 0]
    return _case(f"gate-{tag(aligned16, exact)}-keep{keep}-{form}", "a", _interleave(lens), 0, keep,
                 aligned16, exact, form, dup=(1,))


def gate_cases(aligned16, exact):
    out = []
    for keep in M.all_gate_keeps(aligned16, exact):
        out.append(gate_case(keep, aligned16, exact))
        if not aligned16 or keep % 4 == 0:
            out.append(gate_case(keep, aligned16, exact, "off"))
    return out


def cap_cases(aligned16, exact):
    """The same keeps reached through cap under a large hint, overflowed segments present."""
    out = []
    for cap in CAPS:
        lens = _boundary_lens(cap, aligned16, exact, extra=(cap - 1, cap))
        lens += [cap + 1, cap + 7, 3 * cap + 2, CAP_HINT]
        out.append(_case(f"cap-{tag(aligned16, exact)}-cap{cap}", "a", _interleave(lens), cap, CAP_HINT,
                         aligned16, exact, dup=(2, len(lens))))
    return out


LOOSE_LENS = (1, 2, 3, 4, 5, 5, 0, -1, 4, 3, 5, 1, 0, 2, -1, 5)


def loose_cases(aligned16, exact):
    """(tight, loose): the same segments under max_len = true longest and under max_len = 20000."""
    t = tag(aligned16, exact)
    return (_case(f"tight-{t}", "a", LOOSE_LENS, 0, 5, aligned16, exact),
            _case(f"loose-{t}", "a", LOOSE_LENS, 0, 20000, aligned16, exact))


# ------------------------------------------------------------------ (b) EXACT kernels at their edges
def exact_edge_case(keep, aligned16):
    lens = [57, keep, 0, min(keep - 1, 131), keep, -1, 3]
    return _case(f"exact-edge-{tag(aligned16, True)}-keep{keep}", "b", lens, 0, keep, aligned16, True,
                 dup=(4,))


def fast_x_case(keep):
    lens = [keep, 300, min(keep, 8189), 0, keep, 8188, -1, 5]
    return _case(f"fast-x-keep{keep}", "b", lens, 0, keep, False, False, dup=(4,))


def edge_cases():
    return ([exact_edge_case(k, a) for k in EXACT_EDGES for a in (False, True)] +
            [fast_x_case(k) for k in FAST_X_EDGES])


# ------------------------------------------------------------------ (c) the classifier's partition
# config -> (aligned16, exact, cap, max_len, {where: [(class, lo, hi, count)]}); where: "first" =
# block 0 only, "last" = the last block only, "high" = one block of index >= 64 only (the middle
# block when there are no 64)
PARTITION = {
    "fast-aligned-cap1024": (True, False, 1024, 3000, {
        "first": [("W4", 129, 256, 40), ("F", 1024, 1600, 9)],
        "last": [("W8", 257, 512, 40)],
        "high": [("W16", 513, 1023, 12), ("F", 1024, 1024, 3)]}),
    "fast-unaligned": (False, False, 0, 8200, {
        "first": [("W4", 126, 253, 40), ("W32", 1022, 2045, 4), ("X", 8190, 8200, 3)],
        "last": [("W8", 254, 509, 40), ("W64", 2046, 4093, 3), ("W128", 4094, 8189, 3)],
        "high": [("W16", 510, 1021, 12), ("X", 8190, 8200, 2)]}),
    "exact-aligned": (True, True, 0, 400, {
        "first": [("X", 129, 400, 40)],
        "last": [],
        "high": [("X", 129, 400, 40)]}),
}


def partition_blocks(nseg):
    """{where: block index} of the deliberate placements."""
    nblocks, _ = M.classifier_blocks(nseg)
    return {"first": 0, "last": nblocks - 1, "high": 64 if nblocks > 65 else nblocks // 2}


def partition_case(nseg, config, skipped=True, colref=0):
    """The bulk: lane-class, empty and skipped segments, lane classes other than T8 absent from
    whole blocks; a few hundred wave / FULL / X segments in chosen blocks only."""
    aligned16, exact, cap, max_len, special = PARTITION[config]
    rng = np.random.default_rng(nseg)
    nblocks, chunk = M.classifier_blocks(nseg)
    block = np.arange(nseg) // chunk
    u = rng.random(nseg)
    # (without skipped segments -- the fused column reference reads every row -- few empty ones, so
    # that some columns have none)
    lens = np.where(u < (0.15 if skipped else 0.02), 0,
                    np.where(skipped & (u < 0.30), -1, rng.integers(1, 9, nseg)))
    for lo, hi, ulo, uhi, inblock in ((9, 16, 0.90, 1.00, block % 2 == 1),          # T16: odd blocks
                                      (17, 32, 0.80, 0.90, block % 3 == 0),         # T32: every third
                                      (33, 64, 0.75, 0.80, block >= nblocks // 2),  # T64: the upper half
                                      (65, 128, 0.72, 0.75, (block == 0) | (block == nblocks - 1))):
        at = inblock & (u >= ulo) & (u < uhi)
        lens[at] = rng.integers(lo, hi + 1, int(at.sum()))
    if nseg == 1:
        lens[:] = 5
    where = partition_blocks(nseg)
    taken = np.zeros(nseg, bool)
    for w, groups in special.items() if nseg > 1000 else ():
        b = where[w]
        members = np.flatnonzero((block == b) & ~taken)
        for cls, lo, hi, count in groups:
            at = rng.choice(members, count, replace=False)
            members = np.setdiff1d(members, at)
            taken[at] = True
            lens[at] = rng.integers(lo, hi + 1, count)
            lens[at[0]], lens[at[-1]] = lo, hi
    dup = tuple(int(s) for s in np.flatnonzero(lens > 0)[::97][:40])
    return _case(f"partition-{config}-nseg{nseg}", "c", lens, cap, max_len, aligned16, exact, dup=dup,
                 colref=colref)


COLREF_NSEG, COLREF_NCOLS = 1024, 32


def partition_cases():
    out = []
    for nseg in NSEGS:
        for config in PARTITION:
            colref = nseg == COLREF_NSEG and config == "fast-unaligned"
            out.append(partition_case(nseg, config, skipped=not colref, colref=COLREF_NCOLS if colref else 0))
    return out


def one_class_cases():
    """A whole launch in one class: every other class has count 0 and their starts coincide."""
    rng = np.random.default_rng(3)
    return [
        _case("one-class-T8", "c", rng.integers(1, 9, 1500), 0, 8, False, False, dup=(0, 700)),
        _case("one-class-W4", "c", 4 * rng.integers(33, 65, 300), 0, 256, True, False, dup=(0, 150)),
        _case("one-class-X", "c", rng.integers(129, 401, 150), 0, 400, False, True, dup=(0, 70)),
    ]


@lru_cache(maxsize=None)
def all_cases():
    out = []
    for a, e in PARAMS:
        out += gate_cases(a, e) + cap_cases(a, e) + list(loose_cases(a, e))
    return tuple(out + edge_cases() + partition_cases() + one_class_cases())


# ------------------------------------------------------------------ (d) coverage
def coverage(cases=None):
    """What covers what, from the model alone: {(aligned16, exact): {"class": {class: case name},
    "closed": {gate: case name}, "open": {gate: case name}}, "variants": {...}, "np2": {...}}.
    AssertionError when a reachable class, one side of a gate, an EXACT kernel or an np2 value of
    (b) has no case: the case list is incomplete."""
    cases = all_cases() if cases is None else cases
    report = {"variants": {}, "np2": {}}
    closed_keep = {}
    for a, e in PARAMS:
        report[(a, e)] = {"class": {}, "closed": {}, "open": {}}
    for c in cases:
        pop, run = populated(c), case_launched(c)
        r = report[(c.aligned16, c.exact)]
        for cls in pop:
            r["class"].setdefault(cls, c.name)
        for gate in M.gate_keeps(c.aligned16, c.exact):
            if gate not in run and pop - {gate}:     # closed while another class is populated:
                best = closed_keep.get((c.aligned16, c.exact, gate), 0)  # the longest such launch
                if M.keep_of(c.max_len, c.cap) > best:
                    closed_keep[(c.aligned16, c.exact, gate)] = M.keep_of(c.max_len, c.cap)
                    r["closed"][gate] = c.name
            if gate in run and gate in pop:          # open and populated
                r["open"].setdefault(gate, c.name)
        if "X" in pop and "X" in run:
            v = M.exact_variant(M.keep_of(c.max_len, c.cap))
            report["variants"].setdefault(v.kernel, c.name)
            if c.group == "b" and v.np2:
                report["np2"].setdefault(v.np2, c.name)
    for a, e in PARAMS:
        r = report[(a, e)]
        missing = M.reachable(a, e) - set(r["class"])
        assert not missing, (tag(a, e), "classes without a case", sorted(missing))
        for side in ("closed", "open"):
            missing = set(M.gate_keeps(a, e)) - set(r[side])
            assert not missing, (tag(a, e), f"gates never {side}", sorted(missing))
    assert set(report["variants"]) == {"lds1024", "lds8192", "lds32768", "global"}, report["variants"]
    assert set(report["np2"]) == {65536, 131072}, report["np2"]
    return report


def format_coverage(report):
    lines = []
    for a, e in PARAMS:
        r = report[(a, e)]
        lines.append(f"[{tag(a, e)}]")
        for cls in M.CLASSES:
            if cls in r["class"]:
                lines.append(f"  class {cls:5s} populated: {r['class'][cls]}")
        for gate in M.CLASSES:
            if gate in r["open"]:
                lines.append(f"  gate  {gate:5s} closed: {r['closed'][gate]}; open: {r['open'][gate]}")
    for k, v in report["variants"].items():
        lines.append(f"EXACT kernel {k}: {v}")
    for k, v in sorted(report["np2"].items()):
        lines.append(f"np2 {k}: {v}")
    return "\n".join(lines)
