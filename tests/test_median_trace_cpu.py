"""The control-flow model of the median select (tests/_median_trace.py) against np.sort, the proof,
from the keys alone, that every constructed segment of tests/_median_cases.py reaches the branch it
was built for and is sensitive to a sloppy version of it, and the coverage table of the four
kernel families' instantiations, computed from the traces.  tests/test_gpu_median_branches.py runs
the same segments on the GPU.  No GPU."""
import numpy as np
import pytest

import _median_cases as C
import _median_trace as T
from _moments_cases import edge_segments


def _mid_keys(keys):
    s = np.sort(np.asarray(keys, np.uint32).astype(np.int64))
    n = s.size
    return int(s[n // 2 if n & 1 else n // 2 - 1]), int(s[n // 2])


def _check_trace(keys, PL, full, kb, m0=0):
    tr = T.lean_trace(keys, PL, full, kb, m0)   # asserts its d0 / d1 against np.sort itself
    assert (tr.mn + tr.d0, tr.mn + tr.d1) == _mid_keys(keys)
    assert tr.visits[-1].exit != "descend" and all(v.exit == "descend" for v in tr.visits[:-1])
    assert len(tr.visits) < T.levels(tr.LOG)    # the LEVELS bound is never what ends the loop
    return tr


def test_geometry_mirrors_the_header():
    assert [T.bins(PL) for PL in T.CLASSES] == [(64, 6, 1), (128, 7, 2), (256, 8, 4), (256, 8, 4), (512, 9, 8),
                                                (512, 9, 8)]
    assert [T.levels(L) for L in (6, 7, 8, 9)] == [7, 6, 5, 5]
    assert C.Tree(6, C.R32).S == [26, 20, 14, 8, 2, 0] and C.Tree(9, C.R23).S == [14, 5, 0]
    assert T.median3(3, 1, 2) == T.median3(1, 2, 3) == T.median3(2, 3, 1) == 2 and T.median3(5, 5, 1) == 5
    o = T.slot_order(4, 250, 3)
    assert o[0] == -1 and o[1] == 1 and o[64] == -1 and o[128] == -1 and o[192] == 0 and (o >= 0).sum() == 250


def test_instantiation_map():
    assert len(T.instantiations()) == 22
    assert T.instantiation("strided_masked", 255, 0) == (4, False, True)
    assert T.instantiation("strided_masked", 255, 1) == (8, False, True)     # need = n + 3
    assert T.instantiation("strided_masked", 256, 0) is None and T.instantiation("strided_full", 256, 0) == (4, True, True)
    assert T.instantiation("strided_full", 2048, 0) == (32, True, False)
    assert T.instantiation("strided_masked", 8191, 2) is None                # the EXACT kernel
    assert T.instantiation("strided_masked", 66, 3) == (4, False, True)
    assert T.instantiation("ragged_list", 66, 0, True) is None               # a lane class
    assert T.instantiation("ragged_list", 1024, 0, True, 0) == (16, False, False)   # PL 16 without KEEPBIN
    assert T.instantiation("ragged_list", 1024, 0, True, 1024) is None
    assert T.instantiation("ragged_full", 1024, 0, True, 1024) == (16, True, True)
    assert T.instantiation("ragged_list", 1023, 1, False) == (32, False, False)
    assert T.instantiation("ragged_list", 256, 0, True, 0) == (4, False, True)
    assert T.instantiation("ragged_full", 256, 0, True, 0) is None
    for fam, PL, full, kb in T.instantiations():
        n = 64 * PL if full else 64 * PL - 4
        assert T.instantiation(fam, n, 0, True, n if full else 0) == (PL, full, kb)


@pytest.mark.parametrize("PL", T.CLASSES)
def test_model_matches_sort_on_seeded_segments(PL):
    """Uniform keys (the draws of tests/test_gpu_segment_stats.py), narrow ranges with ties and full
    32-bit ranges: both `full` values, both `kb` values, every phase."""
    rng = np.random.default_rng(PL)
    seen = set()
    for rep in range(6):
        for full in (False, True):
            n = 64 * PL if full else int(rng.integers(1, 64 * PL - 2))
            draws = (rng.integers(1000, 3_000_000, size=n), rng.integers(5000, 5000 + 2 * PL, size=n),
                     rng.integers(0, 1 << 32, size=n), 777_000 + rng.integers(0, 3, size=n),
                     rng.integers(0, 1 << 27, size=n) * (rng.random(n) < 0.4))
            for keys in draws:
                for kb in (False, True):
                    m0 = 0 if full else int(rng.integers(0, 4))
                    tr = _check_trace(keys.astype(np.uint32), PL, full, kb, m0)
                    seen.update(v.exit for v in tr.visits)
    assert {"descend", "one_value", "two_buckets"} <= seen


@pytest.mark.parametrize("n", [1, 2, 5, 64, 100, 1024, 3000, 8192])
def test_model_matches_sort_on_the_edge_segments(n):
    need = max(n, 1)
    PL = next(p for p in T.CLASSES if need <= 64 * p)
    for keys in edge_segments(n):
        for kb in (False, True):
            _check_trace(keys, PL, False, kb)
            if n == 64 * PL:
                _check_trace(keys, PL, True, kb)


# ------------------------------------------------------------------ the constructed cases
def _configs():
    """(family, PL, n, full, kb, m0) of every launch tests/test_gpu_median_branches.py makes."""
    out = set()
    for fam, PL0, _, _ in T.instantiations():
        if fam == "strided_masked":
            for n in C.lengths(PL0, True) + ((C.SHORT_PL4,) if PL0 == 4 else ()):
                for ph in range(4):
                    inst = T.instantiation(fam, n, ph)
                    if inst:
                        out.add((fam,) + (inst[0], n, inst[1], inst[2], ph))
        elif fam == "strided_full":
            out.add((fam, PL0, 64 * PL0, True, PL0 <= 16, 0))
        elif fam == "ragged_list":
            for n in C.lengths(PL0, True) + (64 * PL0,):
                for aligned, ph in ((True, 0), (False, 1), (False, 3)):
                    inst = T.instantiation(fam, n, ph, aligned, 0)
                    if inst:
                        out.add((fam,) + (inst[0], n, inst[1], inst[2], ph))
        else:
            out.add((fam, PL0, 64 * PL0, True, PL0 <= 16, 0))
    return sorted(out)


FAMILY_CONFIGS = _configs()
CONFIGS = sorted({c[1:] for c in FAMILY_CONFIGS})


@pytest.mark.parametrize("PL", T.CLASSES)
def test_constructed_cases_reach_their_branch_and_are_sensitive(PL):
    for cfg in (c for c in CONFIGS if c[0] == PL):
        _, n, full, kb, m0 = cfg
        cases = C.build_cases(*cfg)
        if n >= 32 * PL + 2:      # only the 66-sample and the crossed-over segments may lack cases
            want_names = {c.name for c in C.build_cases(PL, n, full, kb, 0)}
            assert {c.name for c in cases} >= want_names - {"f_top_key_lane63"}
        assert len(cases) >= (50 if n % 2 == 0 and n > 32 * PL else 15), (cfg, len(cases))
        for c in cases:
            assert c.keys.size == n and c.keys.dtype == np.uint32 and int(c.keys.max()) < C.KEY_WIDE
            tr = _check_trace(c.keys, PL, full, kb, m0)
            assert not C.unmet(tr, c.want), (cfg, c.name, C.unmet(tr, c.want),
                                             [(v.level, v.shift, v.exit, v.n0, v.pad_at) for v in tr.visits])
            assert len(c.wrong) >= 1 and not C.insensitive(c, tr), (cfg, c.name, C.insensitive(c, tr))


def test_every_case_exists_at_the_main_lengths():
    """From n = 32 PL + 2 up every case is built (the odd lengths lack only two_buckets, n0 = 1 needs
    an odd length); the packed-key case is PL 4's."""
    for PL in T.CLASSES:
        names = set()
        for n in C.lengths(PL, True) + (64 * PL,):
            full = n == 64 * PL
            names |= {c.name for c in C.build_cases(PL, n, full, PL <= 16, 0)}
            even = {c.name for c in C.build_cases(PL, 64 * PL - 4, False, PL <= 16, 0)}
            odd = {c.name for c in C.build_cases(PL, 64 * PL - 1, False, PL <= 16, 0)}
        assert all(x.startswith(("a_", "h_r24_l1_two")) for x in even - odd if "_n1_" not in x), even - odd
        assert all("_n1_" in x for x in odd - even), odd - even
        assert ("f_top_key_lane63" in names) == (PL == 4)
        assert {x[0] for x in names} == set("abcfgh" if PL == 4 else "abcgh") | {"e"}
        if T.bins(PL)[2] >= 2:
            assert "a_l0_one_lane_pad_lt" in names


# ------------------------------------------------------------------ coverage, from the traces
def _coverage():
    cov = {}
    for fam, PL, full, kb in T.instantiations():
        pairs, pads = set(), set()
        for cfg in (c[1:] for c in FAMILY_CONFIGS if c[0] == fam):
            if (cfg[0], cfg[2], cfg[3]) != (PL, full, kb):
                continue
            for c in C.build_cases(*cfg):
                for v in T.lean_trace(c.keys, PL, full, kb, cfg[4]).visits:
                    pairs.add((v.exit, v.level >= 1))
                    pads.add(v.pad_at)
        cov[(fam, PL, full, kb)] = (pairs, pads)
    return cov


def format_coverage(cov):
    lines = []
    for (fam, PL, full, kb), (pairs, pads) in cov.items():
        reach, dead, want_pads = T.reachable(fam, full, kb)
        lines.append(f"{fam} PL{PL} full={int(full)} kb={int(kb)}")
        for e in T.EXITS:
            cells = []
            for deep in (False, True):
                cells.append("reached" if (e, deep) in pairs else "dead: " + dead[(e, deep)] if (e, deep) in dead
                             else "MISSING")
            lines.append(f"    {e:16s} level 0: {cells[0]:70s} level >= 1: {cells[1]}")
        lines.append("    padding: " + ", ".join(sorted(pads)) +
                     ("" if pads >= want_pads else "   MISSING " + ", ".join(sorted(want_pads - pads))))
    return "\n".join(lines)


def test_coverage_table_has_no_missing_reachable_pair():
    cov = _coverage()
    assert len(cov) == 22
    print(format_coverage(cov))
    for key, (pairs, pads) in cov.items():
        reach, dead, want_pads = T.reachable(key[0], key[2], key[3])
        assert not pairs & set(dead), (key, pairs & set(dead))       # the model never enters a dead pair
        assert pairs == reach, (key, "missing", reach - pairs)
        assert pads == want_pads, (key, "missing", want_pads - pads)
    # two_buckets needs t0 != t1: no odd length reaches it
    for cfg in CONFIGS:
        if cfg[1] % 2:
            assert all(v.exit != "two_buckets" for c in C.build_cases(*cfg)
                       for v in T.lean_trace(c.keys, cfg[0], cfg[2], cfg[3], cfg[4]).visits)


def test_exits_of_the_older_uniform_inputs():
    """Not a gate: which exits the uniform draws in [1000, 3e6) of tests/test_gpu_segment_stats.py
    (test_lengths_and_alignment, test_short_segments_parity) reach.  Printed; DESIGN.md section 5
    records it."""
    seen = {}
    for length in (255, 256, 257, 511, 512, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191,
                   8192):
        rng = np.random.default_rng(length)
        for begin in (0, 1, 2, 3):
            stride = length + begin + (int(rng.integers(0, 5)) if begin else 0)
            host = rng.integers(1000, 3_000_000, size=6 * stride, dtype=np.uint32)
            for s in range(6):
                at = s * stride + begin
                aligned = stride % 4 == 0 and begin == 0
                PL = T._smallest_pl(length if aligned else length + 3)
                if PL is None:
                    continue
                full = aligned and length == 64 * PL
                tr = _check_trace(host[at:at + length], PL, full, PL <= 16, 0 if full else at % 4)
                for v in tr.visits:
                    seen[(v.exit, v.level)] = seen.get((v.exit, v.level), 0) + 1
    print(sorted(seen.items()))
