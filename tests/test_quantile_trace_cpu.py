"""The control-flow model of the quantile kernels (tests/_quantile_trace.py) against np.sort, and the
proof, from the keys alone, that every constructed segment of tests/_quantile_cases.py reaches the
branch it was built for (its `wants`).  tests/test_gpu_quantile_branches.py runs those segments on
the GPU; a case whose trace does not show its branch fails here first.  No GPU."""
import numpy as np
import pytest

import _quantile_cases as C
import _quantile_trace as T
import oracle as O

# tests/test_gpu_quantiles.py: LENGTHS, _aligned_case, test_streaming_path's parameters
SEEDED_LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096,
                  4097, 8191, 8192]
SEEDED_STREAMS = [(1, 8193, 0, 0), (3, 8193, 0, 1), (1, 20000, 0, 0), (3, 20000, 0, 3), (2, 40000, 0, 2),
                  (2, 40000, 20000, 0), (3, 20000, 8193, 1), (2, 8190, 0, 3)]


def _sorted_keys(keys, pm):
    s = np.sort(np.asarray(keys, np.uint32))
    return [int(s[r]) for r in T.ranks(len(keys), pm)]


def _us_distinct(keys):
    """Distinct keys convert to distinct float32 microseconds: a wrong sample cannot hide."""
    u = np.unique(np.asarray(keys, np.uint32))
    us = O.key_to_f32(u).astype(np.float32) / np.float32(1000)
    return np.unique(us).size == u.size


def test_geometry_mirrors_the_headers():
    assert [T.bins(PL) for PL in T.CLASSES] == [(64, 6), (128, 7), (256, 8), (256, 8), (512, 9), (512, 9)]
    assert T.wave_class(1, 0) == T.wave_class(256, 0) == T.wave_class(253, 3) == 4
    assert T.wave_class(257, 0) == T.wave_class(254, 3) == 8
    assert T.wave_class(8192, 0) == T.wave_class(8189, 3) == 128
    assert T.wave_class(8193, 0) is None and T.wave_class(8190, 3) is None
    assert T.NQ == 8 and C.level_shifts(6) == [17, 11, 5, 0] and C.level_shifts(9) == [14, 5, 0]


@pytest.mark.parametrize("length", SEEDED_LENGTHS)
def test_model_matches_sort_on_the_seeded_lengths(length):
    seen = set()
    for begin in range(4):
        rng = np.random.default_rng(1000 * length + begin)       # _aligned_case
        stride = length + begin + (int(rng.integers(0, 5)) if begin else 0)
        if begin and stride % 4 == 0:
            stride += 1
        host = rng.integers(1000, 3_000_000, size=6 * stride, dtype=np.uint32)
        for s in range(6):
            at = s * stride + begin
            keys = host[at: at + length]
            tr = T.trace(keys, at % 4, C.PM)   # 8190 and more samples misaligned by 3 stream
            assert tr.keys == _sorted_keys(keys, C.PM), (length, begin, s)
            seen.update(v.exit for v in getattr(tr, "visits", ()))
    # the seeded draws span 22 bits: never the compaction that ranks above 2^26
    assert "compact_gt26" not in seen


@pytest.mark.parametrize("nseg,length,cap,begin", SEEDED_STREAMS)
def test_model_matches_sort_on_the_seeded_streams(nseg, length, cap, begin):
    rng = np.random.default_rng(length + cap + begin)
    stride = length + begin + 1
    host = rng.integers(1000, 3_000_000, size=nseg * stride, dtype=np.uint32)
    keep = min(length, cap) if cap else length
    for s in range(nseg):
        at = s * stride + begin + length - keep
        keys = host[at: at + keep]
        tr = T.trace(keys, at % 4, C.PM)
        assert tr.keys == _sorted_keys(keys, C.PM)
        if length == 8190 and at % 4 != 3:  # 8190 samples stream only when misaligned by 3
            assert isinstance(tr, T.WaveTrace) and tr.PL == 128
            continue
        assert tr.head + 4 * tr.nvec + tr.tail == keep and tr.head == (4 - at % 4) % 4
        # 22-bit keys: every rank shares the top byte's prefix, so pass 1 has one histogram
        assert len(tr.passes[1].prefixes) == 1


def test_table_lengths_and_their_classes():
    """Every class at its lower edge (the padding is large) and its upper edge; misaligned by 3 the
    upper edge crosses into the next class, 8192 into the streaming kernel."""
    for PL, (lo, hi) in C.CLASS_LENGTHS.items():
        assert T.wave_class(lo, 0) == T.wave_class(lo, 3) == T.wave_class(hi, 0) == PL
        assert 64 * PL - lo >= 56 and 64 * PL - hi == 0
        nxt = T.wave_class(hi, 3)
        assert nxt == (None if PL == 128 else 2 * PL)


@pytest.mark.parametrize("n", C.TABLE_LENGTHS)
@pytest.mark.parametrize("name", C.WAVE_CASES)
def test_constructed_wave_cases_reach_their_branch(name, n):
    for begin in C.BEGINS:
        if T.wave_class(n, begin) is None:
            continue  # 8192 + 3: the streaming kernel's, see test_constructed_stream_cases
        case = C.wave_case(name, n, begin)
        assert len(case.segs) == 6 and len(case.wants) == 6
        for i, (keys, wants) in enumerate(zip(case.segs, case.wants)):
            assert keys.size == n and keys.dtype == np.uint32 and _us_distinct(keys)
            tr = T.wave_trace(keys, begin, case.pm)
            assert tr.keys == _sorted_keys(keys, case.pm)
            assert tr.bits == C.BITS and int(keys.min()) == C.MN
            assert not C.unmet(tr, wants), (name, n, begin, i, C.unmet(tr, wants), tr.visits)
            if begin == 3 or n != 64 * tr.PL:
                assert tr.pad > 0
            if name == "n_bins":  # eight first-level bins: after the first visit every rank is alone
                assert len(tr.visits) >= 9 and all(len(v.ranks) == 1 for v in tr.visits[1:])
            if name == "n_equal":
                assert all(len(v.ranks) == 8 for v in tr.visits)
            print(name, n, begin, i, f"PL{tr.PL} pad{tr.pad}",
                  [(v.level, v.sh, v.count, v.ranks, v.exit, v.padin) for v in tr.visits])


@pytest.mark.parametrize("n", C.GT26_LENGTHS)
def test_constructed_gt26_cases(n):
    for begin in C.BEGINS:
        case = C.gt26(n, begin)
        for keys, wants in zip(case.segs, case.wants):
            assert keys.size == n and _us_distinct(keys)
            tr = T.wave_trace(keys, begin, case.pm)
            assert tr.keys == _sorted_keys(keys, case.pm) and tr.bits > 26 and tr.visits[0].sh == tr.bits
            assert not C.unmet(tr, wants), (n, begin, C.unmet(tr, wants), tr.visits)
            exits = [v.exit for v in tr.visits]
            # reachable only with n <= 64: a longer segment's first window is halved LOG times first
            assert ("compact_gt26" in exits) == (n <= T.QCAND)
            assert exits == ["compact_gt26"] if n <= T.QCAND else exits[0] == "histogram"
        assert len({int(k.max()) - int(k.min()) >= 1 << 31 for k in case.segs}) == 2  # bits 32 too
        assert any(np.unique(k).size < n for k in case.segs) or n == 2                # ties


@pytest.mark.parametrize("n", C.STREAM_LENGTHS)
@pytest.mark.parametrize("name", C.STREAM_CASES)
def test_constructed_stream_cases(name, n):
    for begin in range(4):
        case = C.stream_case(name, n, begin)
        for keys, wants in zip(case.segs, case.wants):
            assert keys.size == n and _us_distinct(keys)
            tr = T.stream_trace(keys, begin, case.pm)
            assert tr.keys == _sorted_keys(keys, case.pm)
            assert not C.unmet(tr, wants), (name, n, begin, C.unmet(tr, wants))
            # the scalar head, the vectors and the scalar tail all occur over the four begins
            assert tr.head == (4 - begin) % 4 and tr.nvec > 2000 and tr.tail == (n - tr.head) % 4
            if name != "o_equal":
                assert len(set(tr.keys)) == 8
    heads_tails = {(T.stream_trace(case.segs[0], b, case.pm).head, T.stream_trace(case.segs[0], b, case.pm).tail)
                   for b in range(4)}
    assert {h for h, _ in heads_tails} == {0, 1, 2, 3} and any(t for _, t in heads_tails)


def test_upper_edge_misaligned_streams():
    """8192 samples misaligned by 3 run the streaming kernel: the deep data there, too."""
    case = C.j_deep(8192, 0)
    for keys in case.segs:
        tr = T.trace(keys, 3, case.pm)
        assert isinstance(tr, T.StreamTrace) and tr.keys == _sorted_keys(keys, case.pm)
