"""GPU: histograms through the profiler handle (nvrx_profiler_get_histograms) and the public
Detector.kernel_histograms, equal to numpy over the records the rings retain.  Each test runs
its profiler in a fresh process (one profiler per process) and closes it."""
import numpy as np
import pytest

import oracle as O
from _histogram_workers import COUNTS, NAMES, RING, pushed_durations
from _mp import run_world
from nvidia_resiliency_ext.straggler import histograms

pytestmark = pytest.mark.gpu


def _ref(durations, cap):
    kept = np.asarray(durations, np.uint32)[-cap:]
    return np.bincount(histograms.bucket_of(kept), minlength=histograms.BINS).astype(np.int64)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def test_profiler_histograms():
    r = run_world(1, "_histogram_workers", "profiler_histograms")[0]
    pushed = pushed_durations()
    assert COUNTS == [21, 7, 1] and RING == 7
    assert r["names"] == sorted(NAMES) and r["names"] != NAMES
    assert r["num"] == [min(len(pushed[n]), RING) for n in r["names"]]
    assert sorted(r["num"]) == [1, 7, 7]  # of the 21 pushes the last 7 count
    assert r["counts"].dtype == np.int64 and r["counts"].shape == (len(NAMES), histograms.BINS)
    for i, n in enumerate(r["names"]):
        assert np.array_equal(r["counts"][i], _ref(pushed[n], RING)), n
    assert r["counts"].sum(1).tolist() == r["num"]
    # a second call gives the same; the log and get_stats are as they were
    assert r["again_names"] == r["names"] and np.array_equal(r["again_counts"], r["counts"])
    assert r["before"] == r["after"] and list(r["before"]) == sorted(NAMES)
    assert r["nrec"] == sum(COUNTS)
    # MIN and MAX of get_stats lie in the lowest / highest occupied bucket
    us = histograms.edges_us()
    for i, n in enumerate(r["names"]):
        _, mn, mx, _, _, _ = r["before"][n]
        occ = np.nonzero(r["counts"][i])[0]
        assert us[occ[0]] <= np.float32(mn) < us[occ[0] + 1]
        assert us[occ[-1]] <= np.float32(mx) < us[occ[-1] + 1]
    assert r["empty"] == ([], [], (0, histograms.BINS))


def test_detector_kernel_histograms():
    r = run_world(1, "_histogram_workers", "detector_histograms")[0]
    pushed = pushed_durations()
    cap = 8 * 1024  # the Detector's rings
    assert list(r["h"]) == sorted(NAMES)
    for n in NAMES:
        assert r["h"][n].dtype == np.int64 and r["h"][n].shape == (histograms.BINS,)
        assert np.array_equal(r["h"][n], _ref(pushed[n], cap)), n
    # the report that follows is what it would have been: every kernel, the reference's statistics
    assert list(r["kern"]) == sorted(NAMES) and r["rel"] == {0: 1.0}
    for n in NAMES:
        st = O.compute_stats(O.ns_to_us(pushed[n]))
        num, mn, mx, med = r["kern"][n]
        assert num == len(pushed[n])
        assert _bits([mn, mx, med]) == _bits([st.min, st.max, st.median]), n
    assert r["after"] == {}  # generate_report reset the interval
