"""GPU: quantiles through the profiler handle (nvrx_profiler_get_quantiles) and the public
Detector.kernel_quantiles, bit for bit against numpy over the records the rings retain.  Each
test runs its profiler in a fresh process (one profiler per process) and closes it."""
import numpy as np
import pytest

import oracle as O
from _mp import run_world
from _quantile_workers import COUNTS, NAMES, pushed_durations

pytestmark = pytest.mark.gpu
PM = (500, 900, 990)


def _ref(durations, cap, pm):
    kept = np.sort(np.asarray(durations, np.uint32)[-cap:])
    n = len(kept)
    keys = [kept[(int(p) * (n - 1)) // 1000] for p in pm]
    return O.key_to_f32(np.asarray(keys, np.uint32)).astype(np.float32) / np.float32(1000)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def test_profiler_quantiles():
    cap = 256
    r = run_world(1, "_quantile_workers", "profiler_quantiles", permille=PM)[0]
    pushed = pushed_durations()
    assert r["names"] == sorted(NAMES) and r["names"] != NAMES
    assert r["num"] == [min(len(pushed[n]), cap) for n in r["names"]]
    assert sorted(r["num"]) == [10, 256, 256] and max(COUNTS) > cap  # the 1000 pushes: last 256 count
    assert r["q"].dtype == np.float32 and r["q"].shape == (len(PM), len(NAMES))
    for i, n in enumerate(r["names"]):
        assert _bits(r["q"][:, i]) == _bits(_ref(pushed[n], cap, PM)), n
    # a second call gives the same; the log and get_stats are as they were
    assert r["again_names"] == r["names"] and _bits(r["again_q"]) == _bits(r["q"])
    assert r["before"] == r["after"] and list(r["before"]) == sorted(NAMES)
    assert r["nrec"] == sum(COUNTS)
    # the median row agrees with get_stats where n is even only by value of the two middle
    # samples; MIN <= q500 <= q900 <= q990 <= MAX always
    for i, n in enumerate(r["names"]):
        _, mn, mx, _, _, _ = r["before"][n]
        col = r["q"][:, i]
        assert np.float32(mn) <= col[0] <= col[1] <= col[2] <= np.float32(mx)
    assert r["empty"] == ([], [], (len(PM), 0))


def test_detector_kernel_quantiles():
    r = run_world(1, "_quantile_workers", "detector_quantiles", permille=PM)[0]
    pushed = pushed_durations()
    cap = 8 * 1024  # the Detector's rings
    assert list(r["q"]) == sorted(NAMES)
    for n in NAMES:
        assert isinstance(r["q"][n], tuple) and all(isinstance(x, float) for x in r["q"][n])
        assert _bits(r["q"][n]) == _bits(_ref(pushed[n], cap, PM)), n
    assert r["q_default"] == r["q"]  # the default request is (500, 900, 990)
    # the report that follows is what it would have been: every kernel, the reference's statistics
    assert list(r["kern"]) == sorted(NAMES) and r["rel"] == {0: 1.0}
    for n in NAMES:
        st = O.compute_stats(O.ns_to_us(pushed[n]))
        num, mn, mx, med = r["kern"][n]
        assert num == len(pushed[n])
        assert _bits([mn, mx, med]) == _bits([st.min, st.max, st.median]), n
    assert r["after"] == {}  # generate_report reset the interval
