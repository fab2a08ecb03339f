"""GPU: Detector.kernel_individual_tail_score, this rank against its own history, in a world of
one without a process group (a fresh process under its own time limit).  Every interval's
IndividualTailScore equals the host twin ``histograms.history_scores`` applied to the profiler's
own histograms with the Detector's policy (name -> slot map, "ncclDev" left out, flagged intervals
not absorbed)."""
import numpy as np
import pytest

import _history_tail_workers as W
import _tail_ref as REF
from nvidia_resiliency_ext.straggler import histograms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    return W.run_solo(timeout=120)


class Twin:
    """The Detector's bookkeeping on the host: slots in order of first appearance."""

    def __init__(self):
        self.slots, self.hist, self.intervals = {}, np.zeros((1, 0, 240), np.uint32), 0

    def step(self, hists):
        names = sorted(hists)
        for n in names:
            self.slots.setdefault(n, len(self.slots))
        grown = np.zeros((1, len(self.slots), 240), np.uint32)
        grown[:, :self.hist.shape[1]] = self.hist
        c = np.asarray([hists[n] for n in names], np.uint32).reshape(1, len(names), 240)
        kw = dict(hist_index=[self.slots[n] for n in names],
                  col_valid=["ncclDev" not in n for n in names])
        s = histograms.history_scores(c, grown, W.PM, update=False, score_thr=W.THRESHOLD, **kw)
        self.hist = histograms.history_scores(c, grown, W.PM, score=False,
                                              skip_rows=s.stragglers, **kw).hist
        self.intervals += not s.stragglers[0]
        top = sorted(((n, int(v)) for n, v in zip(names, s.tail_calls[0]) if v),
                     key=lambda e: (-e[1], e[0]))[:W.TOP]
        return dict(score=float(s.score[0]), tail_ns=int(s.tail_ns[0]), total_ns=int(s.total_ns[0]),
                    history_share=float(s.history_share[0]), is_straggler=bool(s.stragglers[0]),
                    top=top, intervals=self.intervals), s


def assert_same(got, want):
    for key in ("tail_ns", "total_ns", "is_straggler", "top", "intervals"):
        assert got[key] == want[key], key
    for key in ("score", "history_share"):
        assert REF.bits(got[key]) == REF.bits(want[key]), key


def test_every_interval_equals_the_twin(run):
    twin = Twin()
    for i, got in enumerate(run[:3]):
        want, s = twin.step(got["hists"])
        assert_same(got["ts"], want)
        assert got["slots"] == twin.slots
        assert got["after"] == {}  # generate_report reset the interval
        names = sorted(got["hists"])
        assert s.threshold_bucket[0, names.index(W.NCCL)] == -1  # "ncclDev" is left out
    for got in run[3:]:  # after shutdown + initialize, and after reset_tail_history
        assert_same(got["ts"], Twin().step(got["hists"])[0])


def test_what_the_score_says(run):
    first, second, third, fresh, reset = (r["ts"] for r in run)
    assert first["score"] != first["score"] and not first["is_straggler"] and first["intervals"] == 1
    assert first["top"] == [] and first["tail_ns"] == 0 and first["total_ns"] == 0
    # identical intervals: within one bucket's effect (12.5 %) of 1 -- here the same histograms
    assert abs(second["score"] - 1.0) < 0.125 and second["score"] == 1.0
    assert not second["is_straggler"] and second["intervals"] == 2
    # the extra slow records are flagged, their kernel comes first, the interval is not absorbed
    assert third["is_straggler"] and third["score"] < W.THRESHOLD and third["intervals"] == 2
    assert third["top"][0][0] == W.SLOW and third["top"][0][1] >= W.EXTRA
    assert all(W.NCCL != n and W.NEW != n for n, _ in third["top"])
    # a name first seen in interval 3 got a slot; without history it is not in the score
    assert W.NEW in run[2]["slots"] and W.NEW not in run[1]["slots"]
    assert run[2]["slots"][W.NEW] == len(run[1]["slots"])
    # shutdown + initialize, and reset_tail_history, start from no history
    for ts in (fresh, reset):
        assert ts["score"] != ts["score"] and not ts["is_straggler"] and ts["intervals"] == 1
