"""Gate model of the segment quantiles and duration histograms (csrc/segment_quantiles.hip,
segment_histogram.hip, segment_addr.h): plain Python, no torch, no GPU.

Two sides decide which kernel takes a segment.  On the device a kernel takes the segments whose
own need (`seg_need`: retained length + offset in the first 16-byte vector) lies in its class
(`quant_class`, `hist_class`).  On the host `seg_range` turns what the caller said into
[need_lo, need_hi] and a class kernel is launched only if that interval meets its class
(`launched`).  A segment whose class is not launched is taken by no kernel: its output row keeps
what it held and nothing reports it.  tests/test_segment_gate_model_cpu.py proves on this model
that the two sides agree (closure) and that the closure can fail; tests/_segment_gate_cases.py
builds the launches next to every gate `gate_keeps` finds.

These restate the product by hand and nothing about the arithmetic inside a kernel.  The numeric
constants are compared with the source text (`source_constants`); the gate expressions cannot be
read that way, what ties them to the product is the sentinel row of every GPU case.

`slack` (a mutation of the model, 0 in the product): `strided_plus` is the 3 `seg_range` adds to
need_hi of an unaligned strided launch, `quant_slack` widens the lower gate of the quantile
classes to `need_hi <= 32 PL + quant_slack`, `hist_slack` raises the workgroup gate to
`need_hi > HIST_WAVE_MAX + hist_slack`."""
import os
import re
from collections import namedtuple
from functools import lru_cache

from _quantile_trace import CLASSES as QUANT_PL, QUANT_WAVE_MAX, wave_class

HIST_WAVE_MAX = 16384   # segment_histogram.hip
HIST_REPLACE = 16
WV = 4
HS_THREADS = 1024
STREAM = "S"            # the quantiles' streaming kernel
WAVE, BLOCK = "wave", "block"   # the histogram's two kernels
FAMILIES = ("quantiles", "histogram")
KERNELS = {"quantiles": tuple(QUANT_PL) + (STREAM,), "histogram": (WAVE, BLOCK)}
FORMS = ("strided-unaligned", "strided-aligned", "ragged-unaligned", "ragged-aligned")
SCAN_KEEPS = 20000      # gate_keeps scans keep = 0..SCAN_KEEPS

Range = namedtuple("Range", "keep need_lo need_hi aligned")
Slack = namedtuple("Slack", "strided_plus quant_slack hist_slack")
PRODUCT = Slack(3, 0, 0)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "nvidia-resiliency-ext-x_amd", "csrc")


# ---------------------------------------------------------------------------- segment_addr.h
def seg_keep(length, cap):
    """Retained length of `length` pushes (cap <= 0: all)."""
    return cap if cap > 0 and length > cap else length


def seg_need(n, phase):
    """What a wave has to hold: n retained samples starting `phase` slots into a 16-byte vector."""
    assert 0 <= phase < 4
    return n + phase


def strided_first(base_phase, stride, begin, length, cap, s=0):
    """Element index, counted from the 16-byte grid, of segment s's first retained sample;
    base_phase: elements the base pointer lies off the grid."""
    return base_phase + s * stride + begin + (length - seg_keep(length, cap))


def seg_range_strided(base_phase, stride, begin, length, cap, slack=PRODUCT):
    """seg_range(StridedSegs): aligned needs stride % 4 == 0 and an aligned first retained sample
    (segment 0's: with such a stride every segment's)."""
    keep = seg_keep(length, cap)
    aligned = stride % 4 == 0 and strided_first(base_phase, stride, begin, length, cap) % 4 == 0
    return Range(keep, keep, keep if aligned else keep + slack.strided_plus, aligned)


def seg_range_ragged(max_len, cap, aligned16, slack=PRODUCT):
    """seg_range(RaggedSegs, max_len, aligned16): the caller's word, need_lo = 0."""
    keep = seg_keep(max_len, cap)
    return Range(keep, 0, keep if aligned16 else keep + 3, bool(aligned16))


# ---------------------------------------------------------------------------- the two families
def quant_class(need):
    """The quantile kernel that takes a need: its PL, STREAM above QUANT_WAVE_MAX."""
    pl = wave_class(need, 0)
    return STREAM if pl is None else pl


def quant_launched(need_lo, need_hi, slack=PRODUCT):
    out = {pl for pl in QUANT_PL
           if not (need_lo > 64 * pl or (pl > 4 and need_hi <= 32 * pl + slack.quant_slack))}
    if need_hi > QUANT_WAVE_MAX:
        out.add(STREAM)
    return frozenset(out)


def hist_class(need):
    return WAVE if need <= HIST_WAVE_MAX else BLOCK


def hist_launched(need_lo, need_hi, slack=PRODUCT):
    out = set()
    if need_lo <= HIST_WAVE_MAX:
        out.add(WAVE)
    if need_hi > HIST_WAVE_MAX + slack.hist_slack:
        out.add(BLOCK)
    return frozenset(out)


def seg_class(family, n, phase):
    """The kernel that takes a segment of n >= 0 retained samples (an empty one is written by the
    kernel of need = phase: PL 4, the wave kernel); a skipped one (n < 0) is no kernel's."""
    assert n >= 0
    return quant_class(seg_need(n, phase)) if family == "quantiles" else hist_class(seg_need(n, phase))


def launched(family, rng, slack=PRODUCT):
    f = quant_launched if family == "quantiles" else hist_launched
    return f(rng.need_lo, rng.need_hi, slack)


def form_range(form, keep, slack=PRODUCT):
    """The range of a launch of this form whose longest retained run is `keep` (however reached:
    seg_range sees keep alone)."""
    if form == "strided-aligned":
        return seg_range_strided(0, 4, 0, keep, 0, slack)
    if form == "strided-unaligned":
        return seg_range_strided(0, 5, 0, keep, 0, slack)
    assert form in FORMS
    return seg_range_ragged(keep, 0, form == "ragged-aligned", slack)


def form_phases(form):
    """The phases a segment of such a launch may have."""
    return (0,) if form.endswith("-aligned") else (0, 1, 2, 3)


# ---------------------------------------------------------------------------- gates, by scanning
Gate = namedtuple("Gate", "kernel edge closed open")   # edge: "lo" (opens as keep grows) / "hi"


@lru_cache(maxsize=None)
def gate_keeps(family, form):
    """Every pair of neighbouring keeps between which `launched` changes for a kernel: the closed
    keep and the open keep next to it.  Found by scanning keep = 0..SCAN_KEEPS, never typed in."""
    gates = []
    prev = launched(family, form_range(form, 0))
    for keep in range(1, SCAN_KEEPS + 1):
        cur = launched(family, form_range(form, keep))
        for k in KERNELS[family]:
            if (k in prev) != (k in cur):
                gates.append(Gate(k, "lo", keep - 1, keep) if k in cur else Gate(k, "hi", keep, keep - 1))
        prev = cur
    return tuple(gates)


def all_gate_keeps(family):
    """Every keep next to a gate change of any form, ascending."""
    return sorted({k for form in FORMS for g in gate_keeps(family, form) for k in (g.closed, g.open)})


def gates_at(family, form, keep):
    """[(gate, side)]: the gates of this form that `keep` lies next to, and on which side."""
    return [(g, side) for g in gate_keeps(family, form)
            for side, k in (("closed", g.closed), ("open", g.open)) if k == keep]


# ---------------------------------------------------------------------------- the source text
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def source_constants():
    """The numeric constants as the source spells them (evaluated products such as 64 * 128)."""
    def const(text, name):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*([0-9* ]+);" % name, text)
        assert m, name
        v = 1
        for f in m.group(1).split("*"):
            v *= int(f)
        return v
    q, h = _src("segment_quantiles.hip"), _src("segment_histogram.hip")
    ladder = tuple(int(x) for x in re.findall(r"^\s*launch_wave_class<(\d+)>\(", q, re.M))
    return {"QUANT_WAVE_MAX": const(q, "QUANT_WAVE_MAX"), "QUANT_PL": ladder,
            "HIST_WAVE_MAX": const(h, "HIST_WAVE_MAX"), "HIST_REPLACE": const(h, "HIST_REPLACE"),
            "WV": const(h, "WV"), "HS_THREADS": const(h, "HS_THREADS")}
