"""GPU: segment_quantiles.hip on segments built for one branch each (tests/_quantile_cases.py),
against np.sort, bit for bit (the reference and comparison of tests/test_gpu_quantiles.py).

Which branch a segment takes is proved on the CPU, from its keys, by tests/test_quantile_trace_cpu.py
through the control-flow model tests/_quantile_trace.py; the assertions on the trace repeated here
only tie each GPU run to that proof (class, exits).  Every run is strided, six segments, each
starting `begin` slots into a 16-byte vector."""
import numpy as np
import pytest

import _quantile_cases as C
import _quantile_trace as T
from test_gpu_quantiles import _run_strided

pytestmark = pytest.mark.gpu


def _run(case, begin):
    host, stride = C.strided(case.segs, begin)
    assert stride % 4 == 0
    _run_strided(host, len(case.segs), stride, begin, len(case.segs[0]), pm=case.pm)


@pytest.mark.parametrize("n", C.TABLE_LENGTHS)
@pytest.mark.parametrize("name", C.WAVE_CASES)
def test_constructed_wave_cases(name, n):
    """(j) deep selection, (k) the padding below the first level, (l) 64 / 65 in a window, (n) group
    shapes: per class at its lower edge (large padding) and its upper edge, aligned and misaligned
    by 3 (the upper edge then runs in the next class; 8192 + 3 in the streaming kernel)."""
    PL = next(p for p, pair in C.CLASS_LENGTHS.items() if n in pair)
    for begin in C.BEGINS:
        cls = T.wave_class(n, begin)
        upper = n == 64 * PL
        assert cls == (PL if begin == 0 or not upper else None if PL == 128 else 2 * PL)
        case = C.wave_case(name, n, begin if cls else 0)  # streamed: the data built for PL 128
        if cls:
            for keys, wants in zip(case.segs, case.wants):
                tr = T.wave_trace(keys, begin, case.pm)
                assert tr.PL == cls and not C.unmet(tr, wants)
        _run(case, begin)


@pytest.mark.parametrize("n", C.GT26_LENGTHS)
def test_key_range_above_2_26(n):
    """(m) up to 64 samples over more than 2^26: the compaction that ranks by full compare; 65 and
    200 samples over the same range take a histogram level first."""
    for begin in C.BEGINS:
        case = C.gt26(n, begin)
        for keys in case.segs:
            exits = [v.exit for v in T.wave_trace(keys, begin, case.pm).visits]
            assert exits == ["compact_gt26"] if n <= T.QCAND else exits[0] == "histogram"
        _run(case, begin)


@pytest.mark.parametrize("n", C.STREAM_LENGTHS)
@pytest.mark.parametrize("name", C.STREAM_CASES)
def test_streaming_prefix_sharing(name, n):
    """(o) ranks sharing one prefix to the last byte, eight top bytes, two groups of four that
    split across the passes, one value: scalar head, vectors and scalar tail over the begins."""
    for begin in range(4):
        case = C.stream_case(name, n, begin)
        assert not C.unmet(T.stream_trace(case.segs[0], begin, case.pm), case.wants[0])
        _run(case, begin)
