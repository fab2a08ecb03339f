"""CPU: the launch plan of ``MatrixReporter.compact_tail_attribution(counts=)``, in the manner of
test_matrix_tail_launch_plan.py (its recorders over zero tensors on the CPU, plus one for the new
entry): exactly one ``histogram_history_attribution_compact(top=...)`` launch and one copy, no
bucketing and no score; the call without ``counts=`` keeps its old plan; the refusals come in the
stated order, before anything is allocated.  No device and no native library."""
import pytest
import torch

import test_matrix_tail_launch_plan as L
from nvidia_resiliency_ext.straggler import batch, histograms, ops

from test_matrix_tail_launch_plan import plan  # noqa: F401  (the fixture)

R, K, CAP = L.R, L.K, L.CAP
ENTRY = "histogram_history_attribution_compact"


@pytest.fixture
def plan2(plan, monkeypatch):  # noqa: F811
    def fn(*a, **kw):
        plan.calls.append((ENTRY, a, kw))
        return kw.get("out")
    monkeypatch.setattr(batch.ops, ENTRY, fn)
    return plan


def test_counts_is_one_launch_and_one_copy(plan2):
    rep = L.reporter()
    L.individual(rep, "counts", history="compact", permille=900, absorb="never")
    chist_before = rep._ctail["chist"].clone()
    plan2.clear()
    c = L.counts()
    res = rep.compact_tail_attribution(2, counts=c)
    assert plan2.lines == [ENTRY + "(top=2)", "copy()"]  # no bucketing, no score
    (_, a, kw), = plan2.of(ENTRY)
    assert a[0] is c and a[1] is rep._ctail["chist"] and len(a) == 2
    assert kw["permille"] == 900 and kw["col_valid"] is None
    out = kw["out"]
    assert out.loss_all is rep._ctail["loss_all"] and out.idx.shape == (R, 2)
    # the packed buffer behind _tail_attr_buffers, and the one copy moves exactly the attribution
    copied = plan2.of("copy")[0][1][0]
    abuf = rep._ctail["abuf"]
    assert copied.untyped_storage().data_ptr() == abuf.untyped_storage().data_ptr()
    assert copied.numel() == ops.TailAttribution.PACKED * R * 2
    assert out.loss.untyped_storage().data_ptr() == abuf.untyped_storage().data_ptr()
    assert isinstance(res, batch.BatchTailAttribution) and res.kernel.shape == (R, 2)
    assert res.loss_all is rep._ctail["loss_all"]  # stays where it is: not copied
    assert rep._rtail is None and rep._htail is None  # the bucketing work is not needed
    assert torch.equal(rep._ctail["chist"], chist_before)
    plan2.clear()
    rep.compact_tail_attribution(16, counts=c, permille=950)
    assert plan2.lines == [ENTRY + "(top=16)", "copy()"] and plan2.calls[0][2]["permille"] == 950


def test_permille_none_is_the_last_compact_counts_call_s(plan2):
    rep = L.reporter()
    L.individual(rep, "records", history="compact", permille=800)  # a history, but no counts call
    with pytest.raises(RuntimeError, match="permille=None"):
        rep.compact_tail_attribution(2, counts=L.counts())
    plan2.clear()
    rep.compact_tail_attribution(2, counts=L.counts(), permille=700)  # an explicit one is enough
    assert plan2.calls[0][2]["permille"] == 700
    L.individual(rep, "counts", history="compact", permille=910)
    L.individual(rep, "counts", history="dense", permille=920)   # not a compact call
    L.individual(rep, "records", history="compact", permille=930)  # not a counts call
    plan2.clear()
    rep.compact_tail_attribution(2, counts=L.counts())
    assert plan2.calls[0][2]["permille"] == 910
    # the record-stream form keeps its own permille and its old plan, across the counts form
    plan2.clear()
    rep.compact_tail_attribution(2)
    assert plan2.lines == ["segment_history_attribution_compact_ragged(top=2)", "copy()"]
    (_, a, kw), = plan2.of("segment_history_attribution_compact_ragged")
    seg_off, seg_len, out_ns, _ = rep._rtail["bucket"]
    assert a == (out_ns, seg_off, seg_len, K, CAP, rep._ctail["chist"]) and kw["permille"] == 930
    assert rep._rtail["owner"] == "compact"


def test_without_counts_the_old_refusals_stand(plan2):
    rep = L.reporter()
    with pytest.raises(RuntimeError, match="no individual_tail_scores_records"):
        rep.compact_tail_attribution()
    L.individual(rep, "counts", history="compact")
    with pytest.raises(RuntimeError, match="no individual_tail_scores_records"):
        rep.compact_tail_attribution()  # a counts call leaves nothing for the record-stream form


def test_refusals_in_their_order_before_anything_is_allocated(plan2):
    rep = L.reporter()
    bad = torch.zeros((R, K + 1, histograms.BINS), dtype=torch.int32)
    for top in (0, 17, True):
        with pytest.raises(ValueError, match="top"):
            rep.compact_tail_attribution(top, counts=bad)
    rep.exchange = True
    with pytest.raises(NotImplementedError, match="exchange"):  # 1: before the shape
        rep.compact_tail_attribution(2, counts=bad)
    rep.exchange = False
    with pytest.raises(ValueError, match="counts must have shape"):  # 2: before the history
        rep.compact_tail_attribution(2, counts=bad)
    with pytest.raises(RuntimeError, match="no compact history"):  # 3
        rep.compact_tail_attribution(2, counts=L.counts(), permille=950)
    assert plan2.calls == []
    assert rep._tail is None and rep._htail is None and rep._rtail is None and rep._ctail is None
    L.individual(rep, "counts", history="compact", absorb="never")
    plan2.clear()
    with pytest.raises(ValueError, match="counts must have shape"):
        rep.compact_tail_attribution(2, counts=bad)
    with pytest.raises(ValueError, match="permille"):
        rep.compact_tail_attribution(2, counts=L.counts(), permille=1001)
    assert plan2.calls == [] and "abuf" not in rep._ctail


def test_the_one_call_forms_still_refuse(plan2):
    rep = L.reporter()
    with pytest.raises(NotImplementedError, match=r"compact_tail_attribution\(counts="):
        rep.individual_tail_scores(L.counts(), attribute=2, history="compact")
    with pytest.raises(NotImplementedError, match=r"compact_tail_attribution\(\)"):
        rep.individual_tail_scores_records(*L.records(), attribute=2, history="compact")
    assert plan2.calls == [] and rep._ctail is None
