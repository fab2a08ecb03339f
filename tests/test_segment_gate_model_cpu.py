"""The gate model of the segment quantiles and histograms (tests/_segment_gate_model.py): closure of
the device's classes under the host's launch gates, three mutations of the model that break it, the
claims of every GPU case of tests/_segment_gate_cases.py proved from its layout, and the
kept-bucket trace (tests/_histogram_count_trace.py) against np.bincount with the proof that every
counting case reaches its event.  No GPU."""
import numpy as np
import pytest

import _histogram_count_trace as HT
import _quantile_trace as T
import _segment_gate_cases as C
import _segment_gate_model as M
from nvidia_resiliency_ext.straggler import histograms

CLOSURE_KEEPS = {
    "quantiles": list(range(0, M.QUANT_WAVE_MAX + 9)),
    "histogram": [0, 1, 20000] + list(range(M.HIST_WAVE_MAX - 8, M.HIST_WAVE_MAX + 9)),
}
LOOSE = (1, 2, 3, 4, 5, 250, 255, 256, 257, 5000, 70000, 1 << 30)   # added to the keep: looser hints
CAP_OVER = (1, 2, 3, 4, 9, 50000)                                   # len = keep + d, cap = keep


def test_constants_mirror_the_source():
    src = M.source_constants()
    assert src == {"QUANT_WAVE_MAX": M.QUANT_WAVE_MAX, "QUANT_PL": tuple(M.QUANT_PL),
                   "HIST_WAVE_MAX": M.HIST_WAVE_MAX, "HIST_REPLACE": M.HIST_REPLACE, "WV": M.WV,
                   "HS_THREADS": M.HS_THREADS}
    assert M.QUANT_WAVE_MAX == T.QUANT_WAVE_MAX == 64 * max(M.QUANT_PL)
    # the class of a need is the trace model's: one restatement, not two
    for need in (0, 1, 256, 257, 512, 513, 8192, 8193):
        pl = T.wave_class(need, 0)
        assert M.quant_class(need) == (M.STREAM if pl is None else pl)
    assert M.seg_keep(10, 0) == 10 and M.seg_keep(10, 4) == 4 and M.seg_keep(4, 4) == 4 and M.seg_keep(3, 4) == 3
    assert M.seg_need(254, 3) == 257


def _closure_holes(family, slack=M.PRODUCT, keeps=None):
    """Every (how, keep, phase) whose segment no launched kernel takes."""
    holes = []
    for keep in keeps if keeps is not None else CLOSURE_KEEPS[family]:
        # strided: stride % 4 zero and non-zero, the base on and off the grid, plain and through cap
        for base in range(4):
            for stride_mod in (0, 1):
                stride = 4 * (keep + 40) + stride_mod
                for length, cap in [(keep, 0)] + [(keep + d, keep) for d in CAP_OVER if keep]:
                    r = M.seg_range_strided(base, stride, 0, length, cap, slack)
                    assert r.keep == keep
                    on = M.launched(family, r, slack)
                    for s in range(4 if stride_mod else 1):
                        ph = M.strided_first(base, stride, 0, length, cap, s) % 4
                        assert ph == 0 or not r.aligned
                        if M.seg_class(family, keep, ph) not in on:
                            holes.append(("strided", keep, ph, base, stride_mod, cap))
        # ragged: the hint tight or loose, the keep plain or through cap; every shorter segment is
        # some smaller keep's under a looser hint
        for aligned16 in (False, True):
            hints = [(keep + e, 0) for e in (0,) + LOOSE] + [(keep + d, keep) for d in CAP_OVER if keep]
            for max_len, cap in hints:
                r = M.seg_range_ragged(max_len, cap, aligned16, slack)
                on = M.launched(family, r, slack)
                for ph in ((0,) if aligned16 else range(4)):
                    if M.seg_class(family, keep, ph) not in on:
                        holes.append(("ragged", keep, ph, aligned16, max_len, cap))
    return holes


@pytest.mark.parametrize("family", M.FAMILIES)
def test_closure(family):
    assert _closure_holes(family) == []


def test_the_closure_can_fail():
    # strided need_hi = keep on an unaligned launch: 254 at phase 3 needs PL 8, which is not launched
    for family in M.FAMILIES:
        holes = _closure_holes(family, M.Slack(0, 0, 0))
        assert holes and all(h[0] == "strided" and h[2] > 0 for h in holes), holes[:3]
    assert ("strided", 254, 3, 3, 0, 0) in _closure_holes("quantiles", M.Slack(0, 0, 0), keeps=[254])
    # the quantile gate need_hi <= 32 PL + 3: an aligned 257 is PL 8's and PL 8 is not launched
    holes = _closure_holes("quantiles", M.Slack(3, 3, 0))
    assert holes and {h[1] for h in holes} >= {257, 258, 259, 4097, 4099}
    assert not any(h[1] > M.QUANT_WAVE_MAX for h in holes)      # the streaming gate is another
    assert _closure_holes("histogram", M.Slack(3, 3, 0)) == []
    # the histogram gate need_hi > HIST_WAVE_MAX + 3
    holes = _closure_holes("histogram", M.Slack(3, 0, 3))
    assert holes and {h[1] for h in holes} >= {M.HIST_WAVE_MAX + 1, M.HIST_WAVE_MAX - 2}
    assert _closure_holes("quantiles", M.Slack(3, 0, 3)) == []


def test_gate_keeps_are_scanned():
    q = M.all_gate_keeps("quantiles")
    for pl in M.QUANT_PL[1:]:
        # aligned forms change at 32 PL | 32 PL + 1, unaligned ones three below: the + 3 of seg_range
        assert {32 * pl - 3, 32 * pl - 2, 32 * pl, 32 * pl + 1} <= set(q)
    for pl in M.QUANT_PL:   # strided launches also close a class from above
        assert {64 * pl, 64 * pl + 1} <= set(q)
    h = M.all_gate_keeps("histogram")
    assert h == [M.HIST_WAVE_MAX - 3, M.HIST_WAVE_MAX - 2, M.HIST_WAVE_MAX, M.HIST_WAVE_MAX + 1]
    for family in M.FAMILIES:
        for form in M.FORMS:
            gates = M.gate_keeps(family, form)
            assert gates and all(abs(g.closed - g.open) == 1 for g in gates)
            if form.startswith("ragged"):   # need_lo = 0: no ragged launch closes a class from above
                assert all(g.edge == "lo" for g in gates)
        assert max(M.all_gate_keeps(family)) + 8 < M.SCAN_KEEPS


def _prove(c):
    """The claims of one gate case, from its layout and the model."""
    segs = C.case_segments(c)
    rng = C.case_range(c)
    on = M.launched(c.family, rng)
    # the form, as seg_range sees the layout
    strided = isinstance(c, C.Strided)
    form = ("strided-" if strided else "ragged-") + ("aligned" if rng.aligned else "unaligned")
    assert form == c.form, (c.name, form)
    assert rng.keep == c.keep or c.name.startswith(("quantiles-loose", "histogram-loose")), c.name
    if rng.aligned:   # the promise holds: every retained run starts on the grid
        assert all(ph == 0 for n, ph in segs if n > 0), c.name
    elif not strided and c.seg_form == "len" and "gate" in c.name or (strided and c.stride % 4):
        assert {ph for n, ph in segs if n == c.keep} == ({0, 1, 2, 3} if len(segs) >= 4 else
                                                         {ph for _, ph in segs}), c.name
    # how the keep is reached
    lens = [c.length] * c.nseg if strided else [int(n) for n in C.ragged_lens(c)]
    if c.via == "cap":
        assert c.cap == c.keep and any(n > c.cap for n in lens) and any(n == c.keep for n, _ in segs)
    else:
        assert c.cap == 0 and max(lens) == c.keep or "loose" in c.name
    assert max(n for n, _ in segs) <= c.keep and (strided or max(lens) <= c.max_len)
    # every aim: the kernel is launched on the open side only, and the neighbouring keep differs
    assert tuple(c.aims) == tuple(C.Aim(g.kernel, g.edge, side) for g, side in M.gates_at(c.family, form, c.keep))
    for a in c.aims:
        assert (a.kernel in on) == (a.side == "open"), (c.name, a)
        other = c.keep + (1 if (a.edge == "lo") == (a.side == "closed") else -1)
        assert (a.kernel in M.launched(c.family, M.form_range(form, other))) != (a.kernel in on), (c.name, a)
    # closure on the case itself: every segment has a launched kernel
    for n, ph in segs:
        if n >= 0:
            assert M.seg_class(c.family, n, ph) in on, (c.name, n, ph)
    return len(c.aims)


@pytest.mark.parametrize("family", M.FAMILIES)
def test_case_claims(family):
    cases = C.gate_cases(family) + [c for a in (False, True) for c in C.all_class_cases(family, a)]
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert sum(_prove(c) for c in cases) > 0
    for c in cases:   # sizes: a handful of segments of at most about 50k samples
        assert len(C.case_segments(c)) <= 60 and max(n for n, _ in C.case_segments(c)) <= 50000


@pytest.mark.parametrize("family", M.FAMILIES)
def test_case_shapes(family):
    """What the strided and ragged launches have to contain at every gate keep."""
    for keep in C.gate_keeps(family):
        st = C.strided_cases(family, keep)
        plain = [c for c in st if c.via == "plain" and c.base_off == 0]
        assert {(c.begin, c.stride % 4 == 0) for c in plain} == {(b, z) for b in range(4) for z in (False, True)}
        assert {c.nseg for c in plain} >= {1, 3, 4, 5} and all(1 <= c.nseg <= 6 for c in st)
        assert {c.length - c.keep for c in st if c.via == "cap" and c.base_off == 0} == {1, 2, 3, 4}
        assert {c.base_off for c in st if c.stride % 4 == 0} == {0, 1, 2, 3}
        for c in st:   # off the grid with stride % 4 == 0: one phase for all, non-zero unless begin restores it
            if c.base_off and c.via == "plain":
                assert {ph for _, ph in C.strided_segments(c)} == {(c.base_off + c.begin) % 4}
        rg = C.ragged_gate_cases(family, keep)
        assert {(c.aligned16, c.seg_form) for c in rg} == {(a, f) for a in (False, True) for f in ("len", "off")}
        for c in rg:
            segs = C.ragged_segments(c)
            assert c.max_len == keep and c.cap == 0
            phases = {ph for n, ph in segs if n == keep}
            assert phases == ({0} if c.aligned16 else {0, 1, 2, 3}), c.name
            lower = {M.seg_class(family, n, 0) for n in range(1, keep)}
            assert lower <= {M.seg_class(family, n, ph) for n, ph in segs if 0 < n < keep}, c.name
            assert any(n == 0 for n, _ in segs)
            assert c.seg_form == "off" or any(n < 0 for n, _ in segs)
        for c in C.ragged_cap_cases(family, keep):
            segs = C.ragged_segments(c)
            cut = {ph for (n, ph), ln in zip(segs, C.ragged_lens(c)) if ln > c.cap}
            assert cut == ({0} if c.aligned16 else {0, 1, 2, 3}), (c.name, cut)
    tight, loose = C.all_class_cases(family)
    assert {M.seg_class(family, n, ph) for n, ph in C.ragged_segments(tight) if n >= 0} == set(M.KERNELS[family])
    assert tight.max_len == max(tight.lens) and loose.max_len == C.LOOSE_HINT and loose.lens is tight.lens
    # under the loose hint every class kernel runs, under the tight one only those the data needs
    assert M.launched(family, C.ragged_range(loose)) == frozenset(M.KERNELS[family])


@pytest.mark.parametrize("family", M.FAMILIES)
def test_coverage_has_no_hole(family):
    assert C.coverage(family) == []
    # and the table can show one: without the launches reached through cap, their half is missing
    full = C.gate_cases
    try:
        C.gate_cases = lambda f: [c for c in full(f) if c.via == "plain"]
        assert {m[-1] for m in C.coverage(family)} == {"cap"}
    finally:
        C.gate_cases = full


def test_the_plus_three_is_pinned():
    """keep = 254 at phase 3 needs 257: PL 8's, launched only because need_hi = 257 > 256."""
    hit = []
    for c in C.ragged_gate_cases("quantiles", 254):
        if not c.aligned16:
            assert M.launched("quantiles", C.ragged_range(c)) == frozenset({4, 8})
            assert M.launched("quantiles", C.ragged_range(c)._replace(need_hi=254)) == frozenset({4})
            hit += [M.seg_class("quantiles", n, ph) for n, ph in C.ragged_segments(c) if (n, ph) == (254, 3)]
    assert hit and set(hit) == {8}
    for c in C.ragged_gate_cases("histogram", M.HIST_WAVE_MAX - 2):
        if not c.aligned16:
            assert M.BLOCK in {M.seg_class("histogram", n, ph) for n, ph in C.ragged_segments(c) if n > 0}


# ---------------------------------------------------------------------------- the kept-bucket trace
def _bincount(keys):
    return np.bincount(histograms.bucket_of(np.asarray(keys, np.uint32)), minlength=HT.BINS).astype(np.int64)


@pytest.mark.parametrize("n,m0", [(1, 0), (3, 3), (255, 1), (1024, 0), (1025, 0), (2047, 2), (2048, 3), (5000, 1)])
def test_trace_counts_like_bincount(n, m0):
    rng = np.random.default_rng(n + m0)
    for keys in (rng.integers(1000, 3_000_000, size=n, dtype=np.uint32), C.full_span(n, rng),
                 rng.choice(np.array([100_000, 113_000, 126_000], np.uint32), size=n)):
        tr = HT.trace(keys, m0)
        assert np.array_equal(tr.counts, _bincount(keys))
        nreg = len(tr.regs)
        assert tr.counts.sum() == n and tr.spare == 64 * nreg - n   # every slot counted once
        HT.events(tr)
    # one wave of the workgroup kernel counts its own slots; the sixteen together count the segment
    keys = C.full_span(16385 + n, rng)
    total = sum(HT.trace(keys, m0, "block", w).counts for w in range(M.HS_THREADS // 64))
    assert np.array_equal(total, _bincount(keys))


def test_register_order():
    s, per_trip = HT.wave_slots(2048, 3)
    assert per_trip == 16 and s.shape == (48, 64)       # 2051 slots: a third trip for the last 3
    assert s[0, 0] == -3 and s[1, 0] == -2 and s[0, 1] == 1 and s[4, 0] == 253 and s[16, 0] == 1021
    assert np.array_equal(np.sort(s.reshape(-1)), np.arange(-3, 48 * 64 - 3))
    b, _ = HT.block_slots(16385, 0, 5)
    assert b.shape == (32, 64) and b[0, 0] == 4 * 320 and b[4, 0] == 4 * (1024 + 320) and b[16, 0] == 4 * (4096 + 320)
    every = np.concatenate([HT.block_slots(16385, 0, w)[0].reshape(-1) for w in range(16)])
    assert np.array_equal(np.sort(every), np.arange(2 * 16384))


@pytest.mark.parametrize("case", C.count_cases(), ids=lambda c: c.name)
def test_counting_cases_reach_their_event(case):
    n = int(case.keys.size)
    assert case.keys.dtype == np.uint32
    if case.kernel == "wave":
        assert n + case.m0 <= 2048 + 3 and M.hist_class(n + case.m0) == M.WAVE
        tr = HT.trace(case.keys, case.m0)
        assert np.array_equal(tr.counts, _bincount(case.keys))
        ev = HT.events(tr)
        assert case.wants <= ev, (case.name, case.wants - ev, [r for r in tr.regs if r.side][:12])
        return
    assert M.HIST_WAVE_MAX < n + case.m0 <= 49153 + 3 and M.hist_class(n + case.m0) == M.BLOCK
    traces = [HT.trace(case.keys, case.m0, "block", w) for w in range(M.HS_THREADS // 64)]
    assert np.array_equal(sum(t.counts for t in traces), _bincount(case.keys))
    if case.wants == {"waves_differ"}:
        rows = {tuple(t.counts) for t in traces}
        assert len(rows) == len(traces)                       # sixteen different private histograms
        assert all(not (set(np.nonzero(a.counts)[0]) & set(np.nonzero(b.counts)[0]))
                   for i, a in enumerate(traces) for b in traces[:i])
    else:
        assert case.wants <= C.block_facts(case), (case.name, C.block_facts(case))
        last = traces[0].regs[-1].trip
        live = sum(64 * len([r for r in t.regs if r.trip == last]) for t in traces) - \
            (sum(t.spare for t in traces) - case.m0)
        if "block-plus1" in case.wants:    # the last trip: at most one vector's slots are live
            assert 1 <= live <= 4 and last >= 1
        else:                               # nothing masked anywhere
            assert sum(t.spare for t in traces) == 0
        assert any(r.side and r.flushed for t in traces for r in t.regs)


def test_counting_cases_cover_the_events():
    wants = set().union(*(c.wants for c in C.count_cases()))
    assert wants >= {"miss15_no_replacement", "miss16_replacement", "flush_empty", "flush_nonempty", "p_equal",
                     "alternate", "readopt", "distinct64", "spare_evicted", "spare_evicted_nonempty",
                     "readopt_spare", "spare_adopted_in_last_trip", "spare_flushed_at_end", "block-exact",
                     "block-plus1", "waves_differ"}
    assert {c.m0 for c in C.count_cases() if c.name.startswith("spare")} == {1, 2, 3}
