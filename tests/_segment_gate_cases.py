"""The launches of tests/test_gpu_quantile_gates.py and tests/test_gpu_histogram_gates.py as data
(numpy, no torch, no GPU), built from the gate model (tests/_segment_gate_model.py), and the
constructed segments of the histogram's counting (tests/_histogram_count_trace.py).

Every gate case says what it is aimed at: its family, the form of the launch (strided aligned or
not, ragged with or without the caller's aligned16), how the keep is reached (plain, or through
cap from a longer segment), and `aims`: the (kernel, edge, side) of every launch gate its keep
lies next to.  tests/test_segment_gate_model_cpu.py proves each claim on the model from the
layout alone, and `coverage()` lists the reachable combinations no case is aimed at.

A ragged length of 0 is an empty segment, -1 a skipped one (the offsets-only form has none)."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import _histogram_count_trace as HT
import _segment_gate_model as M
from nvidia_resiliency_ext.straggler import _native, histograms

Aim = namedtuple("Aim", "kernel edge side")
Strided = namedtuple("Strided", "family name form via keep nseg stride begin length cap base_off aims")
Ragged = namedtuple("Ragged", "family name form via keep lens off cap max_len aligned16 seg_form aims")
Count = namedtuple("Count", "name kernel keys m0 wants")

LOOSE_HINT = 70000
NSEGS = (1, 3, 4, 5, 6, 3, 4, 5)   # the wave kernels take four segments per workgroup
KEY_LO, KEY_HI = 1000, 3_000_000


def _aims(family, form, keep):
    return tuple(Aim(g.kernel, g.edge, side) for g, side in M.gates_at(family, form, keep))


def gate_keeps(family):
    return M.all_gate_keeps(family)


# ---------------------------------------------------------------------------- strided launches
def _stride(keep, begin, extra, mod4):
    """The smallest stride >= begin + length + extra with stride % 4 == mod4."""
    s = keep + begin + extra
    return s + (mod4 - s) % 4


def _strided(family, tag, keep, nseg, stride, begin, length, cap, base_off):
    aligned = stride % 4 == 0 and (base_off + begin + length - keep) % 4 == 0  # what the builder intends
    form = "strided-aligned" if aligned else "strided-unaligned"
    via = "cap" if cap else "plain"
    name = f"{family}-{tag}-keep{keep}-n{nseg}-st{stride}-b{begin}-len{length}-off{base_off}"
    return Strided(family, name, form, via, keep, nseg, stride, begin, length, cap, base_off,
                   _aims(family, form, keep))


@lru_cache(maxsize=None)
def strided_cases(family, keep):
    out = []
    # begin 0..3, a stride with stride % 4 == 0 (every segment in the same phase) and one with
    # stride % 4 == 1 (the phase moves from segment to segment)
    i = 0
    for mod4 in (0, 1):
        for begin in range(4):
            out.append(_strided(family, "plain", keep, NSEGS[i % len(NSEGS)],
                                _stride(keep, begin, 2, mod4), begin, keep, 0, 0))
            i += 1
    # through cap from len = keep + d: the cut moves the phase.  begin + d = 0 (mod 4) with
    # stride % 4 == 0 is an aligned launch reached through cap
    for d in range(1, 5):
        for mod4, begin in sorted({(0, 0), (0, (4 - d) % 4), (1, d % 4)}):
            out.append(_strided(family, "cap", keep, 3 + d % 4, _stride(keep + d, begin, 1, mod4), begin,
                                keep + d, keep, 0))
    # a base 1..3 elements off the 16-byte grid, stride % 4 == 0: every segment has the same
    # non-zero phase and the host's pointer test decides; with begin = 4 - off the pointer test
    # must find the launch aligned again
    for off in range(1, 4):
        out.append(_strided(family, "base", keep, 3 + off, _stride(keep, 0, 4, 0), 0, keep, 0, off))
        out.append(_strided(family, "base", keep, 4, _stride(keep, 4 - off, 4, 0), 4 - off, keep, 0, off))
        out.append(_strided(family, "basecap", keep, 3, _stride(keep + 2, 0, 4, 0), 0, keep + 2, keep, off))
    return tuple(out)


def strided_segments(c):
    """[(n, phase)] of every segment, from the layout alone."""
    return [(c.keep, M.strided_first(c.base_off, c.stride, c.begin, c.length, c.cap, s) % 4)
            for s in range(c.nseg)]


def strided_range(c, slack=M.PRODUCT):
    return M.seg_range_strided(c.base_off, c.stride, c.begin, c.length, c.cap, slack)


def strided_numel(c):
    return c.base_off + (c.nseg - 1) * c.stride + c.begin + c.length


def strided_retained(c, host, s):
    """host: the whole allocation (the tensor handed over starts at host[base_off])."""
    end = c.base_off + s * c.stride + c.begin + c.length
    return host[end - c.keep: end]


# ---------------------------------------------------------------------------- ragged launches
def lower_lens(family, keep, upto=None):
    """Lengths below `keep` on both sides of every class edge (phase 0), and 1."""
    out = {1}
    prev = M.seg_class(family, 1, 0)
    for n in range(2, keep):
        cur = M.seg_class(family, n, 0)
        if cur != prev:
            out.update((n - 1, n))
        prev = cur
    if family == "histogram":
        out.update(n for n in (300, 5000) if n < keep)
    return sorted(out)


def _layout_len(lens, phases, aligned16):
    """seg_len form: runs with gaps, segment i in phase phases[i] (0 under aligned16)."""
    off, pos = [], 4
    for i, n in enumerate(lens):
        ph = 0 if aligned16 else phases[i]
        pos += (ph - pos) % 4
        off.append(pos)
        pos += max(n, 0) + (i % 3)
    return np.array(off, np.int64)


def _ragged(family, tag, keep, lens, phases, cap, max_len, aligned16, seg_form):
    form = "ragged-aligned" if aligned16 else "ragged-unaligned"
    if seg_form == "len":
        lens = np.asarray(lens, np.int64)
        off = _layout_len(lens, phases, aligned16)
    else:
        # offsets only: back to back, so the phase of a run is set by what lies before it -- a
        # filler segment of 1..3 samples (a real segment, checked like every other) moves it
        seq, pos = [], 0
        for n, ph in zip(lens, phases):
            assert n >= 0
            f = 0 if aligned16 else (ph - pos) % 4
            if f:
                seq.append(f)
                pos += f
            assert not aligned16 or pos % 4 == 0, "a run off the grid breaks the promise"
            seq.append(n)
            pos += n
        lens = np.asarray(seq, np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert int(lens.max()) <= max_len   # the contract: the hint bounds every length
    name = f"{family}-{tag}-keep{keep}-{form}-{seg_form}"
    return Ragged(family, name, form, "cap" if cap else "plain", keep, lens, off, cap, max_len,
                  bool(aligned16), seg_form, _aims(family, form, keep))


def _interleave(lens):
    out = []
    for i, n in enumerate(lens):
        out.append(n)
        if i % 4 == 1:
            out.append(0)
        if i % 5 == 2:
            out.append(-1)
    return out


@lru_cache(maxsize=None)
def ragged_gate_cases(family, keep):
    """max_len = keep: segments at the keep in phases 0..3 (phase 0 under aligned16), shorter ones
    of every lower class, empty and skipped ones between them; both segment forms."""
    out = []
    low = lower_lens(family, keep)
    for aligned16 in (False, True):
        lens = _interleave([keep, low[0], keep] + low[1:] + [keep - 1, keep, keep])
        phases = [(i * 3 + 1) % 4 for i in range(len(lens))]
        at = [i for i, n in enumerate(lens) if n == keep]
        for j, i in enumerate(at):
            phases[i] = j % 4
        out.append(_ragged(family, "gate", keep, lens, phases, 0, keep, aligned16, "len"))
        if aligned16:
            # starts on the grid need lengths that are multiples of 4: only the last run is free
            lens = sorted({(n + 3) // 4 * 4 for n in low if (n + 3) // 4 * 4 < keep} | {0}) + [keep]
            phases = [0] * len(lens)
        else:
            lens = [n for n in lens if n >= 0]
            phases = [(i * 3 + 1) % 4 for i in range(len(lens))]
            for j, i in enumerate(i for i, n in enumerate(lens) if n == keep):
                phases[i] = j % 4
        out.append(_ragged(family, "gate", keep, lens, phases, 0, keep, aligned16, "off"))
    return tuple(out)


@lru_cache(maxsize=None)
def ragged_cap_cases(family, keep):
    """The keep reached through cap under a large hint."""
    out = []
    low = [n for n in lower_lens(family, keep) if n < 600 or n > keep - 600][:6]
    # aligned16 = False: every cut phase (start phase + len - cap), rings that overflowed far
    lens = [keep + 1, keep + 2, keep + 3, keep + 4, keep + 1, keep + 2, 2 * keep + 3, keep, 0, -1] + low
    phases = [0, 0, 0, 0, 1, 3, 2, 3] + [i % 4 for i in range(2 + len(low))]
    for seg_form in ("len", "off"):
        ll, pp = (lens, phases) if seg_form == "len" else \
            ([n for n in lens if n >= 0], [p for n, p in zip(lens, phases) if n >= 0])
        out.append(_ragged(family, "cap", keep, ll, pp, keep, LOOSE_HINT, False, seg_form))
    # aligned16 = True: len - cap a multiple of 4.  A cut off the 16-byte grid would break the
    # promise of aligned16, which is about every retained run (segment_addr.h: "aligned = every
    # retained run starts on a 16-byte boundary"), not about where the segment begins
    lens = [keep + 4, keep + 8, keep + 4 * ((keep + 3) // 4), 0, -1] + low + [keep]
    out.append(_ragged(family, "cap", keep, lens, [0] * len(lens), keep, LOOSE_HINT, True, "len"))
    lens = [n for n in lens if n >= 0 and n % 4 == 0] + [keep + 4]
    out.append(_ragged(family, "cap", keep, lens, [0] * len(lens), keep, LOOSE_HINT, True, "off"))
    return tuple(out)


ALL_CLASSES = {"quantiles": [1, 0, 200, 300, 254, 600, 1100, -1, 2100, 4200, 8100, 8190, 8192, 9000, 0, 7],
               "histogram": [0, 5, 1000, -1, 16381, 16384, 16390, 20000, 3]}


def all_class_cases(family, aligned16=False):
    """(tight, loose): one launch holding a segment of every class under max_len = max(lens), and
    the same data under a loose hint; the results are required equal bit for bit."""
    lens = ALL_CLASSES[family]
    phases = [(3 * i + 3) % 4 for i in range(len(lens))]
    tight = _ragged(family, "tight", max(lens), lens, phases, 0, max(lens), aligned16, "len")
    return tight, tight._replace(name=tight.name.replace("tight", "loose"), max_len=LOOSE_HINT)


def ragged_lens(c):
    """Length per segment as the device sees it."""
    return c.lens if c.seg_form == "len" else np.diff(c.off)


def ragged_segments(c):
    """[(n, phase)] of every segment from the layout alone: the retained length (< 0: skipped) and
    the phase of the first retained sample."""
    out = []
    for s, n in enumerate(ragged_lens(c)):
        n = int(n)
        keep = M.seg_keep(n, c.cap)
        out.append((keep, int(c.off[s] + max(n, 0) - max(keep, 0)) % 4))
    return out


def ragged_range(c, slack=M.PRODUCT):
    return M.seg_range_ragged(c.max_len, c.cap, c.aligned16, slack)


def ragged_numel(c):
    lens = ragged_lens(c)
    return int((c.off[:len(lens)] + np.maximum(lens, 0)).max())


def ragged_retained(c, host, s):
    n = int(ragged_lens(c)[s])
    keep = M.seg_keep(n, c.cap)
    return host[int(c.off[s]) + n - keep: int(c.off[s]) + n]


def case_segments(c):
    return strided_segments(c) if isinstance(c, Strided) else ragged_segments(c)


def case_range(c, slack=M.PRODUCT):
    return strided_range(c, slack) if isinstance(c, Strided) else ragged_range(c, slack)


def gate_cases(family):
    """Every gate case of a family."""
    out = []
    for keep in gate_keeps(family):
        out += strided_cases(family, keep) + ragged_gate_cases(family, keep) + ragged_cap_cases(family, keep)
    return out


# ---------------------------------------------------------------------------- keys
def full_span(n, rng):
    """Every u32 up to NVRX_KEY_MAX: wide keys, the top bit set."""
    v = rng.integers(0, _native.KEY_MAX + 1, size=n, dtype=np.uint64).astype(np.uint32)
    if n >= 2:
        v[0], v[-1] = _native.KEY_MAX, 0
    return v


def host_keys(c, seed):
    """The whole allocation of a case: uniform keys in [1000, 3 10^6), the retained run of one
    segment per launch spanning every u32 key."""
    rng = np.random.default_rng(seed)
    numel = strided_numel(c) if isinstance(c, Strided) else ragged_numel(c)
    host = rng.integers(KEY_LO, KEY_HI, size=numel + 8, dtype=np.uint32)
    segs = case_segments(c)
    live = [s for s, (n, _) in enumerate(segs) if n > 0]
    if live:
        s = live[len(live) // 2]
        run = strided_retained(c, host, s) if isinstance(c, Strided) else ragged_retained(c, host, s)
        run[:] = full_span(run.size, rng)
    return host


# ---------------------------------------------------------------------------- coverage
def _taken(c):
    """The kernels that take a segment of the case at its keep."""
    return {M.seg_class(c.family, n, ph) for n, ph in case_segments(c) if n == c.keep}


def coverage(family):
    """The (form, kernel, edge, side, via) combinations the model finds reachable that no case is
    aimed at, and the open sides at which no case has the kernel take a segment at the keep."""
    aimed, taken = set(), set()
    for c in gate_cases(family):
        for a in c.aims:
            aimed.add((c.form, a.kernel, a.edge, a.side, c.via))
            if a.side == "open" and a.kernel in _taken(c):
                taken.add((c.form, a.kernel, a.edge, c.via))
    missing = []
    for form in M.FORMS:
        for g in M.gate_keeps(family, form):
            for via in ("plain", "cap"):
                for side in ("closed", "open"):
                    if (form, g.kernel, g.edge, side, via) not in aimed:
                        missing.append((form, g.kernel, g.edge, side, via))
                if (form, g.kernel, g.edge, via) not in taken:
                    missing.append((form, g.kernel, g.edge, "open: not taken", via))
    return missing


# ---------------------------------------------------------------------------- histogram counting
_EDGE = None


def key_of(b):
    """A key of bucket b (its lower edge)."""
    global _EDGE
    if _EDGE is None:
        _EDGE = np.asarray(histograms.edges_keys(), np.uint64)[:HT.BINS].astype(np.uint32)
    return _EDGE[b]


def _from_regs(n, m0, bm, kernel="wave", wave=0):
    """Keys of a segment whose registers (rows of bm, 64 buckets each, in the order count_reg sees
    them) hold the given buckets; masked lanes are skipped."""
    slots, _ = HT.wave_slots(n, m0) if kernel == "wave" else HT.block_slots(n, m0, wave)
    bm = np.asarray(bm)
    assert bm.shape == slots.shape, (bm.shape, slots.shape)
    live = (slots >= 0) & (slots < n)
    keys = np.zeros(n, np.uint32)
    keys[slots[live]] = key_of(bm[live])
    return keys


def _reg(*parts):
    """A register from (count, bucket) runs, lanes ascending."""
    row = np.concatenate([np.full(c, b) for c, b in parts])
    assert row.size == 64
    return row


A, B, C, D, E = 100, 110, 120, 130, 140


def count_cases():
    out = []
    # 15 against 16 misses, replacements of an empty and of a non-empty kept bucket, p0 == p1, a
    # bucket (B) evicted and adopted again
    regs = [_reg((64, A)), _reg((64, A)),
            _reg((15, D), (49, A)),             # 15 misses: nothing replaced
            _reg((16, B), (48, A)),             # 16: b1 (never used, empty) takes B
            _reg((16, C), (40, A), (8, B)),     # b1 = B holds 8: flushed, takes C
            _reg((16, B), (24, A), (24, C)),    # p0 == p1 = 24: b0 = A is flushed, B comes back
            _reg((15, E), (49, B))] + [_reg((64, A))] * 9
    out.append(Count("misses-15-16-flushes", "wave", _from_regs(1024, 0, regs), 0,
                     {"miss15_no_replacement", "miss16_replacement", "flush_empty", "flush_nonempty",
                      "p_equal", "readopt", "spare_evicted"}))
    # replacements alternating between b0 and b1: each register brings 16 of a new bucket and 48
    # of the one adopted last
    ring = [A, B, C, D, E]
    regs = [_reg((64, A))] + [_reg((16, ring[(r + 1) % 5]), (48, ring[r % 5])) for r in range(31)]
    out.append(Count("alternate", "wave", _from_regs(2048, 0, regs), 0,
                     {"alternate", "readopt", "flush_nonempty"}))
    # 64 distinct buckets in one register
    regs = [60 + (np.arange(64) + 5 * r) % 64 for r in range(16)]
    out.append(Count("distinct64", "wave", _from_regs(1024, 0, regs), 0, {"distinct64", "flush_nonempty"}))
    # a head with m0 = 1..3 (lane 0 of the first m0 registers lies before the run: the spare bin,
    # which b0 still holds, is hit), then spread keys evict the spare bin with that count, and a
    # last trip whose masked lanes (19 in one register, then whole registers) miss, adopt the spare
    # bin again and have it flushed at the end
    for m0 in (1, 2, 3):
        n = 1460
        rng = np.random.default_rng(m0)
        keys = key_of(60 + rng.integers(0, 64, size=n))
        out.append(Count(f"spare-m0-{m0}", "wave", keys, m0,
                         {"spare_evicted_nonempty", "readopt_spare", "spare_adopted_in_last_trip",
                          "spare_flushed_at_end"}))
    # the workgroup kernel: nvec an exact multiple of 4096 at phase 0 (the last trip unmasked,
    # nothing clamped), one more than a multiple (one live vector, 4095 clamped re-reads), both
    # with clustered and spread keys so that replacements happen in every wave
    for name, n, m0 in (("block-exact", 32768, 0), ("block-plus1", 16385, 0), ("block-plus1", 49153, 0),
                        ("block-plus1-head", 49150, 3)):
        rng = np.random.default_rng(n)
        keys = rng.integers(KEY_LO, KEY_HI, size=n, dtype=np.uint32)
        keys[n // 3: 2 * n // 3] = full_span(2 * n // 3 - n // 3, rng)
        out.append(Count(f"{name}-{n}", "block", keys, m0, {name.split("-head")[0]}))
    # waves of one workgroup fed different bucket sets: wave w meets buckets 20 + 12 w .. + 2 only
    n, m0 = 20001, 1
    slot = np.arange(n)
    w = (((slot + m0) >> 2) % M.HS_THREADS) >> 6
    out.append(Count("block-waves-differ", "block", key_of(20 + 12 * w + slot % 3), m0, {"waves_differ"}))
    return out


def block_facts(c):
    """What the layout of a workgroup-kernel counting case shows: for every trip the live vectors."""
    n, m0 = int(c.keys.size), c.m0
    nvec = (n + m0 + 3) >> 2
    tv = M.HS_THREADS * M.WV
    trips = (nvec + tv - 1) // tv
    last_live = nvec - (trips - 1) * tv
    facts = set()
    if m0 == 0 and nvec % tv == 0 and n == 4 * nvec:
        facts.add("block-exact")
    if last_live == 1 and trips >= 2:
        facts.add("block-plus1")
    return facts


ACCUMULATE_LENS = [1000, 20000, 0, 16384, 16385, -1, 7]   # both kernels in one launch
