"""CPU: the launch plan of MatrixReporter's tail-score methods.  The GPU suites compare results bit
for bit and cannot see whether a call took one launch or three, so this pins, per method and
request, the sequence of ``ops`` launches the docstrings promise -- their order, the ``update=`` /
``score=`` / ``skip_rows=`` / ``top=`` / ``kind=`` / ``counts=`` arguments, the tensors they get --
and the one device-to-host copy per call.  The launching functions of ``batch.ops`` are replaced by
recorders over zero tensors on the CPU; everything that only computes (request checks, packed
layouts, dataclasses) stays real.  No device and no native library."""
import types

import numpy as np
import pytest
import torch

from nvidia_resiliency_ext.straggler import batch, histograms, ops

R, K, CAP, N = 2, 3, 4, 5
SHOWN = ("update", "score", "skip_rows", "top", "kind", "counts")  # the arguments a plan line shows
SCORES = ("histogram_tail_scores", "segment_tail_scores_ragged", "histogram_history_scores",
          "segment_history_scores_ragged")
COMPACT_SCORES = ("histogram_history_scores_compact", "segment_history_scores_compact_ragged")
ATTRIBUTIONS = ("histogram_tail_attribution", "segment_tail_attribution_ragged",
                "segment_history_attribution_ragged", "segment_history_attribution_compact_ragged")
OTHERS = ("histogram_sum", "segment_fleet_histogram_ragged", "histogram_tail_threshold",
          "histogram_tail_base", "histogram_history_age", "compact_history_age",
          "compact_history_from_dense", "compact_history_to_dense", "records_bucket")


class Plan:
    """What a reporter launched: ``lines`` as text, ``calls`` as (name, args, kwargs)."""

    def __init__(self):
        self.calls = []

    @property
    def lines(self):
        def show(k, v):
            return f"{k}=strag" if k == "skip_rows" and v is not None else f"{k}={v}"
        return [f"{n}({', '.join(show(k, kw[k]) for k in SHOWN if k in kw)})"
                for n, _, kw in self.calls]

    def of(self, name):
        return [c for c in self.calls if c[0] == name]

    def clear(self):
        del self.calls[:]


@pytest.fixture
def plan(monkeypatch):
    p = Plan()

    def recorder(name, result):
        def fn(*a, **kw):
            p.calls.append((name, a, kw))
            return result(a, kw)
        return fn

    scored = types.SimpleNamespace(tail_calls=None)
    for n in SCORES:
        monkeypatch.setattr(batch.ops, n, recorder(n, lambda a, kw: scored))
    for n in COMPACT_SCORES:
        monkeypatch.setattr(batch.ops, n, recorder(n, lambda a, kw: (scored, None)))
    for n in ATTRIBUTIONS + OTHERS:
        monkeypatch.setattr(batch.ops, n, recorder(n, lambda a, kw: kw.get("out")))
    monkeypatch.setattr(batch.ops, "records_bucket_capacity", lambda n, nstreams, nslots: 16)
    # the device-to-host copy and the in-place clear, seen where the reporter asks for them
    cpu, zero_ = torch.Tensor.cpu, torch.Tensor.zero_
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t: p.calls.append(("copy", (t,), {})) or cpu(t))
    monkeypatch.setattr(torch.Tensor, "zero_",
                        lambda t: p.calls.append(("zero_", (t,), {})) or zero_(t))
    return p


def reporter():
    rep = batch.MatrixReporter.__new__(batch.MatrixReporter)
    rep.R, rep.K, rep.cap, rep.device = R, K, CAP, torch.device("cpu")
    rep.exchange, rep.col_valid, rep.thr_rel, rep.thr_ind = False, None, 0.75, 0.7
    rep._pipes = set()
    rep._tail = rep._htail = rep._rtail = rep._ctail = None
    rep._absorbed = {"dense": 0, "compact": 0}
    return rep


def counts():
    return torch.zeros((R, K, histograms.BINS), dtype=torch.int32)


def records():
    return torch.zeros((N, 2), dtype=torch.int32), torch.zeros(R + 1, dtype=torch.int64)


def same(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype


def behind(attr, scores):
    """The attribution's outputs lie behind the score outputs, in the same buffer."""
    last = scores.strag
    return all(t.untyped_storage().data_ptr() == last.untyped_storage().data_ptr() and
               t.data_ptr() >= last.data_ptr() + last.numel()
               for t in (attr.idx, attr.loss, attr.tail_ns, attr.total_ns, attr.tail_calls,
                         attr.thr_bucket, attr.base_share))


# -- the fleet's tail scores ------------------------------------------------------------------
FLEET = {
    ("counts", 0): ["histogram_sum()", "histogram_tail_threshold()", "histogram_tail_scores()",
                    "copy()"],
    ("counts", 2): ["histogram_sum()", "histogram_tail_threshold()", "histogram_tail_scores()",
                    "histogram_tail_base()", "histogram_tail_attribution(top=2, kind=relative)",
                    "copy()"],
    ("records", 0): ["records_bucket()", "segment_fleet_histogram_ragged()",
                     "histogram_tail_threshold()", "segment_tail_scores_ragged()", "copy()"],
    ("records", 2): ["records_bucket()", "segment_fleet_histogram_ragged()",
                     "histogram_tail_threshold()", "segment_tail_scores_ragged()",
                     "histogram_tail_base()", "segment_tail_attribution_ragged(top=2)", "copy()"],
}


@pytest.mark.parametrize("source,attribute", sorted(FLEET))
def test_fleet_tail_scores(plan, source, attribute):
    rep = reporter()
    if source == "counts":
        c = counts()
        res = rep.tail_scores(c, attribute=attribute)
        t, score, attr = rep._tail, "histogram_tail_scores", "histogram_tail_attribution"
    else:
        recs, rec_off = records()
        res = rep.tail_scores_records(recs, rec_off, attribute=attribute)
        t, score, attr = rep._rtail, "segment_tail_scores_ragged", "segment_tail_attribution_ragged"
    assert plan.lines == FLEET[source, attribute]
    assert isinstance(res, batch.BatchTailScores) and res.score.shape == (R,)
    assert res.threshold_bucket.shape == (K,) and np.isnan(res.fleet_share)
    assert (res.attribution is None) == (attribute == 0) and ("abuf" in t) == (attribute > 0)
    # one buffer: the threshold pass writes thr and fleet_sums where the score pass reads them
    (_, ta, tkw), (_, sa, skw) = plan.of("histogram_tail_threshold")[0], plan.of(score)[0]
    fleet = plan.calls[1 if source == "records" else 0][2]["out"]
    assert ta[0] is fleet and tkw["col_valid"] is None and fleet.shape == (K, histograms.BINS)
    thr, sums = (sa[1], sa[2]) if source == "counts" else (sa[5], sa[6])
    assert same(thr, tkw["thr"]) and same(sums, tkw["fleet_sums"]) and skw["score_thr"] == 0.75
    out = skw["out"]
    if source == "records":
        seg_off, seg_len, out_ns, _ = rep._rtail["bucket"]
        assert plan.calls[0][2]["out"] is rep._rtail["bucket"]
        for _, a, kw in plan.calls[1:]:
            if a and a[0] is out_ns:
                assert a[1] is seg_off and a[2] is seg_len and a[3:5] == (K, CAP) and kw["aligned16"]
    else:
        assert sa[0] is c
    copied = plan.of("copy")[0][1][0]
    assert copied.untyped_storage().data_ptr() == out.score.untyped_storage().data_ptr()
    if attribute:
        (_, ba, bkw), (_, aa, akw) = plan.of("histogram_tail_base")[0], plan.of(attr)[0]
        assert ba[0] is fleet and same(ba[1], thr) and bkw["out"] is t["base"]
        assert behind(akw["out"], out) and akw["out"].loss_all is t["loss_all"]
        assert res.attribution.kernel.shape == (R, attribute)
        assert copied.numel() >= t["buf"].numel() + ops.TailAttribution.PACKED * R * attribute
    else:
        assert copied is t["buf"]


# -- the individual tail scores ---------------------------------------------------------------
def individual_plan(score, attribution, absorb, attribute, compact):
    fused = absorb == "always" and not attribute
    lines = [f"{score}(update={fused})"]
    if attribute:
        lines.append(attribution)
    if absorb == "healthy":
        lines.append(f"{score}(score=False, skip_rows=strag)")
    elif absorb == "always" and attribute:
        lines.append(f"{score}(score=False, skip_rows=None)")
    elif absorb == "never" and compact:
        lines.append("zero_()")  # no update: nothing folded
    return lines + ["copy()"]


def test_individual_plan_reads_as_the_docstrings_do():
    # the table above, spelled out for the requests the docstrings name
    s, a = "histogram_history_scores", "histogram_tail_attribution(top=1, kind=individual)"
    assert individual_plan(s, a, "always", 0, False) == [s + "(update=True)", "copy()"]
    assert individual_plan(s, a, "never", 0, False) == [s + "(update=False)", "copy()"]
    assert individual_plan(s, a, "healthy", 0, False) == [
        s + "(update=False)", s + "(score=False, skip_rows=strag)", "copy()"]
    assert individual_plan(s, a, "always", 1, False) == [
        s + "(update=False)", a, s + "(score=False, skip_rows=None)", "copy()"]
    assert individual_plan(s, a, "healthy", 1, False) == [
        s + "(update=False)", a, s + "(score=False, skip_rows=strag)", "copy()"]
    assert individual_plan(s, a, "never", 1, False) == [s + "(update=False)", a, "copy()"]
    c = "segment_history_scores_compact_ragged"
    assert individual_plan(c, None, "never", 0, True) == [c + "(update=False)", "zero_()", "copy()"]


PATHS = {  # (source, history): the score entry and the attribution line
    ("counts", "dense"): ("histogram_history_scores",
                          "histogram_tail_attribution(top=1, kind=individual)"),
    ("records", "dense"): ("segment_history_scores_ragged",
                           "segment_history_attribution_ragged(top=1)"),
    ("counts", "compact"): ("histogram_history_scores_compact", None),
    ("records", "compact"): ("segment_history_scores_compact_ragged", None),
}
REQUESTS = [(s, h, ab, at) for (s, h) in sorted(PATHS) for ab in batch.ABSORB_MODES
            for at in ((0, 1) if h == "dense" else (0,))]


def individual(rep, source, **kw):
    if source == "counts":
        return rep.individual_tail_scores(counts(), **kw)
    return rep.individual_tail_scores_records(*records(), **kw)


@pytest.mark.parametrize("source,history,absorb,attribute", REQUESTS)
def test_individual_tail_scores(plan, source, history, absorb, attribute):
    rep = reporter()
    res = individual(rep, source, history=history, absorb=absorb, attribute=attribute)
    score, attribution = PATHS[source, history]
    compact = history == "compact"
    bucket = ["records_bucket()"] if source == "records" else []
    assert plan.lines == bucket + individual_plan(score, attribution, absorb, attribute, compact)
    assert isinstance(res, batch.BatchIndividualTailScores) and res.score.shape == (R,)
    assert np.isnan(res.history_share).all() and (res.folded is not None) == compact
    assert (res.attribution is None) == (attribute == 0)
    t = rep._ctail if compact else rep._htail
    assert (rep._htail is None) == compact and (rep._ctail is None) == (not compact)
    assert (rep._rtail is None) == (source == "counts") and ("abuf" in t) == (attribute > 0)
    assert rep._absorbed == {"dense": 0, "compact": 0,
                             **({history: 1} if absorb != "never" else {})}
    hist = t["chist" if compact else "hist"]
    launches = plan.of(score)
    first, out = launches[0], launches[0][2]["out"]
    for _, a, kw in launches:  # every launch: this interval against the reporter's one history
        assert a[1 if source == "counts" else 5] is hist and kw["permille"] == 990
        assert kw["col_valid"] is None and (("folded" in kw) == compact)
        if source == "records":
            seg_off, seg_len, out_ns, _ = rep._rtail["bucket"]
            assert a[:5] == (out_ns, seg_off, seg_len, K, CAP) and kw["aligned16"]
    assert first[2]["score_thr"] == 0.7 and first[2]["tail_calls"] is False
    if absorb == "healthy":  # the update skips the rows this call's score flagged, on the device
        assert same(launches[1][2]["skip_rows"], out.strag)
    if compact:
        folded = first[2]["folded"]
        assert all(kw["folded"] is folded or same(kw["folded"], folded) for _, _, kw in launches)
        assert folded.data_ptr() == out.base_total_ns.data_ptr() + 8 * R
        assert out.strag.data_ptr() == folded.data_ptr() + 8 * R
        if absorb == "never":
            assert same(plan.of("zero_")[0][1][0], folded)
    if source == "records":
        assert rep._rtail["owner"] == history
    copied = plan.of("copy")[0][1][0]
    assert copied.untyped_storage().data_ptr() == out.score.untyped_storage().data_ptr()
    if attribute:
        name = attribution.split("(")[0]
        (_, a, kw), = plan.of(name)
        assert behind(kw["out"], out) and kw["out"].loss_all is t["loss_all"]
        assert kw["permille"] == 990 and (kw["hist"] if source == "counts" else a[5]) is hist
    else:
        assert copied is t["buf"]


@pytest.mark.parametrize("source,history", sorted(PATHS))
def test_half_life_ages_before_everything_else(plan, source, history):
    age = "histogram_history_age()" if history == "dense" else "compact_history_age(counts=False)"
    score = PATHS[source, history][0]
    rest = (["records_bucket()"] if source == "records" else []) + [score + "(update=True)", "copy()"]
    rep = reporter()
    individual(rep, source, history=history, absorb="always", half_life=1)
    assert plan.lines == rest  # nothing absorbed yet: nothing to age
    plan.clear()
    individual(rep, source, history=history, absorb="always", half_life=None)
    assert plan.lines == rest and rep._absorbed[history] == 2  # None: no aging launch, ever
    plan.clear()
    individual(rep, source, history=history, absorb="always", half_life=1)
    assert plan.lines == [age] + rest and rep._absorbed[history] == 1
    _, a, _ = plan.calls[0]
    t = rep._ctail if history == "compact" else rep._htail
    assert a[0] is t["chist" if history == "compact" else "hist"] and a[1] == 1
    plan.clear()
    individual(rep, source, history=history, absorb="never", half_life=2)
    assert plan.lines[0] != age and rep._absorbed[history] == 1  # one absorbing call since


def test_buffers_are_allocated_once(plan):
    rep = reporter()
    held = None
    for _ in range(2):
        rep.tail_scores(counts(), attribute=2, tail_calls=True)
        rep.tail_scores_records(*records(), attribute=2, tail_calls=True)
        individual(rep, "counts", attribute=1, tail_calls=True)
        individual(rep, "records", attribute=1)
        individual(rep, "counts", history="compact", tail_calls=True)
        individual(rep, "records", history="compact")
        rep.compact_tail_attribution(3)
        now = {(n, k): v.data_ptr() for n in ("_tail", "_htail", "_rtail", "_ctail")
               for k, v in getattr(rep, n).items() if isinstance(v, torch.Tensor)}
        now["_rtail", "bucket"] = tuple(b.data_ptr() for b in rep._rtail["bucket"])
        assert held is None or held == now
        held = now
    assert {k for _, k in held if _ == "_tail"} == {"buf", "fleet", "calls", "abuf", "loss_all", "base"}
    assert {k for _, k in held if _ == "_htail"} == {"buf", "hist", "calls", "abuf", "loss_all"}
    assert {k for _, k in held if _ == "_ctail"} == {"buf", "chist", "calls", "abuf", "loss_all"}
    assert rep._tail["buf"].numel() == rep._rtail["buf"].numel() == 8 * (3 * R + 2) + 4 * 4 + R
    assert rep._htail["buf"].numel() == 41 * R and rep._ctail["buf"].numel() == 49 * R
    assert len(rep._rtail["bucket"]) == 4 and rep._rtail["bucket"][3] is not None  # push counts


def test_compact_tail_attribution(plan):
    rep = reporter()
    with pytest.raises(RuntimeError, match="no individual_tail_scores_records"):
        rep.compact_tail_attribution()
    individual(rep, "records", history="compact", permille=900)
    plan.clear()
    res = rep.compact_tail_attribution(2)
    assert plan.lines == ["segment_history_attribution_compact_ragged(top=2)", "copy()"]
    (_, a, kw), = plan.of("segment_history_attribution_compact_ragged")
    seg_off, seg_len, out_ns, _ = rep._rtail["bucket"]
    assert a == (out_ns, seg_off, seg_len, K, CAP, rep._ctail["chist"]) and kw["aligned16"]
    assert kw["permille"] == 900 and kw["out"].loss_all is rep._ctail["loss_all"]
    assert isinstance(res, batch.BatchTailAttribution) and res.kernel.shape == (R, 2)
    assert plan.of("copy")[0][1][0].numel() == ops.TailAttribution.PACKED * R * 2
    plan.clear()
    rep.compact_tail_attribution(2, permille=950)
    assert plan.calls[0][2]["permille"] == 950
    individual(rep, "counts", history="compact")  # leaves the buckets alone
    rep.compact_tail_attribution(1)
    rep.tail_scores_records(*records())
    with pytest.raises(RuntimeError, match="re-used the buckets"):
        rep.compact_tail_attribution()


def test_convert_tail_history(plan):
    rep = reporter()
    individual(rep, "counts", absorb="always")
    hist = rep._htail["hist"]
    plan.clear()
    folded = rep.convert_tail_history("compact")
    assert plan.lines == ["compact_history_from_dense()", "copy()"]
    (_, a, kw), = plan.of("compact_history_from_dense")
    assert a[0] is hist and kw["out"] is rep._ctail["chist"] and rep._htail is None
    # the folded counts land where the compact scores keep theirs
    buf = rep._ctail["buf"]
    assert kw["folded"].data_ptr() == buf.data_ptr() + 40 * R and kw["folded"].shape == (R,)
    assert same(plan.of("copy")[0][1][0], kw["folded"])
    assert folded.dtype == np.uint64 and folded.shape == (R,)
    assert rep._absorbed == {"dense": 0, "compact": 1}
    chist = rep._ctail["chist"]
    plan.clear()
    assert rep.convert_tail_history("dense") is None
    assert plan.lines == ["compact_history_to_dense()"]  # nothing synchronizes
    (_, a, kw), = plan.calls
    assert a[0] is chist and kw["out"] is rep._htail["hist"] and rep._ctail is None
    assert rep._htail["buf"].numel() == 41 * R and rep._htail["calls"] is None
    assert rep._absorbed == {"dense": 1, "compact": 0}
    plan.clear()
    individual(rep, "counts", absorb="never")  # the calls that follow continue on the target
    assert plan.calls[0][1][1] is rep._htail["hist"]


def test_age_tail_history(plan):
    rep = reporter()
    assert rep.age_tail_history() == batch.TailHistoryAging() and plan.lines == []
    individual(rep, "counts", absorb="always")
    plan.clear()
    res = rep.age_tail_history(2)
    assert plan.lines == ["histogram_history_age()"] and res.evicted is None
    assert plan.calls[0][1] == (rep._htail["hist"], 2) and rep._absorbed["dense"] == 0
    individual(rep, "records", history="compact", absorb="always")
    plan.clear()
    res = rep.age_tail_history(history="both")
    assert plan.lines == ["histogram_history_age()", "compact_history_age()", "copy()"]
    _, a, kw = plan.calls[1]
    assert a == (rep._ctail["chist"], 1) and kw["evicted"].shape == kw["full"].shape == (R,)
    assert res.evicted.shape == res.full.shape == (R,) and rep._absorbed["compact"] == 0
    plan.clear()
    rep.age_tail_history(history="compact")
    assert plan.lines == ["compact_history_age()", "copy()"]


def test_refusals_launch_and_allocate_nothing(plan):
    rep = reporter()
    recs, rec_off = records()
    for call in (lambda: rep.tail_scores(counts()[:1]),
                 lambda: rep.tail_scores_records(recs, rec_off[:2]),
                 lambda: rep.individual_tail_scores(counts()[:1]),
                 lambda: rep.individual_tail_scores_records(recs, rec_off[:2]),
                 lambda: rep.individual_tail_scores(counts(), absorb="sometimes"),
                 lambda: rep.individual_tail_scores_records(recs, rec_off, half_life=0)):
        with pytest.raises(ValueError):
            call()
    rep.exchange = True
    for call, name in ((lambda: rep.tail_scores(counts()), "tail_scores"),
                       (lambda: rep.tail_scores_records(recs, rec_off), "tail_scores_records"),
                       (lambda: individual(rep, "counts"), "individual_tail_scores"),
                       (lambda: individual(rep, "records"), "individual_tail_scores_records"),
                       (lambda: rep.compact_tail_attribution(), "compact_tail_attribution"),
                       (lambda: rep.convert_tail_history("dense"), "convert_tail_history"),
                       (lambda: rep.age_tail_history(), "age_tail_history")):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert " ".join(str(e.value).split()) == (
            f"MatrixReporter.{name}: tail scores across kernel shards (exchange=True) are not "
            "supported")
    assert plan.calls == []
    assert rep._tail is None and rep._htail is None and rep._rtail is None and rep._ctail is None
