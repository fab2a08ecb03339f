"""GPU: ``Detector.kernel_tail_score(attribute=3)`` and ``kernel_individual_tail_score(attribute=
3)`` in a world of one without a process group (a fresh process under its own time limit): names,
order and values equal the host twins applied to ``kernel_histograms()`` of the same interval, and
everything else in the results is what the calls return without ``attribute``."""
import numpy as np
import pytest

import _history_tail_workers as HW
import _tail_attr_workers as W
import _tail_ref as REF
from nvidia_resiliency_ext.straggler import histograms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    return W.run_solo(timeout=120)


def expected(names, att):
    edges = histograms.edges_us()
    return [dict(name=names[int(k)], loss_ns=float(att.loss[0, j]), tail_ns=int(att.tail_ns[0, j]),
                 total_ns=int(att.total_ns[0, j]), tail_calls=int(att.tail_calls[0, j]),
                 threshold_us=float(edges[int(att.thr_bucket[0, j]) + 1]),
                 base_share=float(att.base_share[0, j]))
            for j, k in enumerate(att.idx[0]) if k >= 0]


def assert_list(got, want):
    assert [g["name"] for g in got] == [w["name"] for w in want]
    for g, w in zip(got, want):
        for key in ("tail_ns", "total_ns", "tail_calls"):
            assert g[key] == w[key], key
        for key in ("loss_ns", "threshold_us", "base_share"):
            assert REF.bits(g[key]) == REF.bits(w[key]), key


def test_relative_attribution_equals_the_twin(run):
    for got in run:
        names = sorted(got["hists"])
        c = np.asarray([got["hists"][n] for n in names], np.uint32).reshape(1, len(names), 240)
        valid = ["ncclDev" not in n for n in names]
        want = expected(names, histograms.tail_attribution(c, W.PM, W.ATTRIBUTE, col_valid=valid))
        assert_list(got["rel"]["attribution"], want)
        assert len(want) == W.ATTRIBUTE and all(HW.NCCL != w["name"] for w in want)
        # a world of one is its own fleet: no kernel's tail exceeds the fleet's share of it
        assert all(abs(w["loss_ns"]) <= 1e-3 * w["total_ns"] for w in want)
        plain = dict(got["rel_plain"])
        assert plain.pop("attribution") is None
        with_att = dict(got["rel"])
        with_att.pop("attribution")
        assert REF.bits(with_att.pop("score")) == REF.bits(plain.pop("score"))
        assert REF.bits(with_att.pop("fleet_share")) == REF.bits(plain.pop("fleet_share"))
        assert with_att == plain


def test_individual_attribution_equals_the_twin(run):
    slots, hist, flagged = {}, np.zeros((1, 0, 240), np.uint32), []
    for i, got in enumerate(run):
        names = sorted(got["hists"])
        for n in names:
            slots.setdefault(n, len(slots))
        grown = np.zeros((1, len(slots), 240), np.uint32)
        grown[:, :hist.shape[1]] = hist
        c = np.asarray([got["hists"][n] for n in names], np.uint32).reshape(1, len(names), 240)
        kw = dict(hist_index=[slots[n] for n in names], col_valid=["ncclDev" not in n for n in names])
        want = expected(names, histograms.history_attribution(c, grown, W.PM, W.ATTRIBUTE, **kw))
        assert_list(got["ind"]["attribution"], want)
        s = histograms.history_scores(c, grown, W.PM, update=False, score_thr=W.THRESHOLD, **kw)
        assert REF.bits(got["ind"]["score"]) == REF.bits(float(s.score[0]))
        assert got["ind"]["is_straggler"] == bool(s.stragglers[0])
        flagged.append(bool(s.stragglers[0]))
        hist = histograms.history_scores(c, grown, W.PM, score=False, skip_rows=s.stragglers, **kw).hist
    assert run[0]["ind"]["attribution"] == []  # no history yet: nothing is taken
    assert flagged == [False, False, True]
    third = run[2]["ind"]["attribution"]
    assert third[0]["name"] == HW.SLOW and third[0]["loss_ns"] > 0
    assert third[0]["tail_calls"] >= HW.EXTRA
    assert all(a["name"] not in (HW.NCCL, HW.NEW) for a in third)
    assert all(a["loss_ns"] <= third[0]["loss_ns"] for a in third)
