"""GPU: nvrx_histogram_tail_base / nvrx_histogram_tail_attribution equal the host twins
(``histograms.tail_attribution`` / ``history_attribution``) bit for bit on every output over the
shared case list of ``_tail_attr_cases``; the two entries in a captured graph equal eager; and
``MatrixReporter.tail_scores`` / ``individual_tail_scores`` with ``attribute`` equal the twins and
leave scores and history what they are without it."""
import numpy as np
import pytest
import torch

import _tail_attr_cases as C
from nvidia_resiliency_ext.straggler import histograms, ops, synth
from nvidia_resiliency_ext.straggler.batch import MatrixReporter

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share", "loss_all")


def dev(a, dtype=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    t = torch.from_numpy(a).to(DEV)
    return t if dtype is None else t.to(dtype)


def twin(case):
    if case["kind"] == "relative":
        return histograms.tail_attribution(case["counts"], case["pm"], case["top"],
                                           col_valid=case["col_valid"], fleet=case["fleet"],
                                           thr_index=case["thr_index"])
    return histograms.history_attribution(case["counts"], case["hist"], case["pm"], case["top"],
                                          hist_index=case["hist_index"], col_valid=case["col_valid"])


def device(case, out=None):
    counts = dev(case["counts"])
    if case["kind"] == "relative":
        fleet = ops.histogram_sum(counts) if case["fleet"] is None else dev(case["fleet"])
        thr, _ = ops.histogram_tail_threshold(fleet, case["pm"], col_valid=dev(case["col_valid"]))
        return ops.histogram_tail_attribution(counts, top=case["top"], kind="relative", thr=thr,
                                              thr_index=dev(case["thr_index"]),
                                              base=ops.histogram_tail_base(fleet, thr), out=out)
    hist = dev(case["hist"])
    before = hist.clone()
    res = ops.histogram_tail_attribution(
        counts, top=case["top"], kind="individual", hist=hist, permille=case["pm"],
        hist_index=dev(case["hist_index"]),
        hist_stride=0 if case["hist_index"] is None else case["hist"].shape[1],
        col_valid=dev(case["col_valid"]), out=out)
    assert torch.equal(hist, before)  # the history is read only
    return res


def assert_same(got, want, what=""):
    """Device tensors / numpy arrays against the twin's arrays, bit for bit (NaN: one pattern)."""
    for f in FIELDS:
        g = getattr(got, f)
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        w = np.asarray(getattr(want, f))
        assert g.shape == w.shape, (what, f)
        if w.dtype == np.float64:
            gn, wn = np.isnan(g), np.isnan(w)
            assert np.array_equal(gn, wn), (what, f)
            assert np.array_equal(g.view(np.uint64)[~gn], w.view(np.uint64)[~wn]), (what, f)
        else:
            assert np.array_equal(g.view(w.dtype) if g.dtype.itemsize == w.dtype.itemsize else g, w), (what, f)


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_device_equals_the_host_twin(case):
    assert_same(device(case), twin(case), case["name"])


def test_tail_base_is_what_the_threshold_call_adds_up():
    fleet = dev(C.synth(np.random.default_rng(5), 40, 37).astype(np.uint64).sum(0))
    valid = torch.ones(37, dtype=torch.uint8, device=DEV)
    valid[3] = 0
    thr, sums = ops.histogram_tail_threshold(fleet, 950, col_valid=valid)
    base = ops.histogram_tail_base(fleet, thr)
    assert torch.equal(base.sum(0), sums)
    assert base[3].tolist() == [0, 0] and int(thr[3]) == -1


def test_outputs_hold_no_stale_values_and_two_calls_agree():
    case = next(c for c in C.CASES if c["name"] == "rel-shape-64x1-top16")
    R, K, top = 64, 1, 16
    out = ops.TailAttribution.empty(R, K, top, DEV)
    for f in FIELDS:
        getattr(out, f).view(torch.uint8).fill_(0x5A)
    a = device(case, out=out)
    assert_same(a, twin(case))
    b = device(case)
    for f in FIELDS:
        assert torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), f


@pytest.mark.parametrize("name", ["rel-thr-index", "ind-hist-index", "rel-shape-2x2049-top16"])
def test_graph_capture_and_replay(name):
    case = next(c for c in C.CASES if c["name"] == name)
    eager = device(case)  # the kernels are loaded before the capture
    torch.cuda.synchronize()
    counts = dev(case["counts"])
    R, K = counts.shape[:2]
    out = ops.TailAttribution.empty(R, K, case["top"], DEV)
    if case["kind"] == "relative":
        fleet = ops.histogram_sum(counts) if case["fleet"] is None else dev(case["fleet"])
        thr, _ = ops.histogram_tail_threshold(fleet, case["pm"], col_valid=dev(case["col_valid"]))
        base = torch.empty((fleet.shape[0], 2), dtype=torch.int64, device=DEV)
        index = dev(case["thr_index"])

        def both():
            ops.histogram_tail_base(fleet, thr, out=base)
            ops.histogram_tail_attribution(counts, top=case["top"], kind="relative", thr=thr,
                                           thr_index=index, base=base, out=out)
    else:
        hist, index, valid = dev(case["hist"]), dev(case["hist_index"]), dev(case["col_valid"])

        def both():
            ops.histogram_tail_attribution(counts, top=case["top"], kind="individual", hist=hist,
                                           permille=case["pm"], hist_index=index,
                                           hist_stride=case["hist"].shape[1], col_valid=valid, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    for f in FIELDS:
        getattr(out, f).view(torch.uint8).fill_(0x5A)
    g.replay()
    torch.cuda.synchronize()
    for f in FIELDS:
        assert torch.equal(getattr(eager, f).view(torch.uint8), getattr(out, f).view(torch.uint8)), f
    assert_same(out, twin(case))


# ------------------------------------------------------------------ MatrixReporter
R_, K_, S_ = 6, 21, 96


def reporter_counts(seed):
    rep = MatrixReporter(R_, K_, cap=S_, device=DEV)
    ns = synth.synth_matrix(R_, K_, S_, seed=seed, device=DEV)
    ns[2, :, ::7] *= 3  # a rank slow on every 7th call
    return rep, rep.histograms(ns, S_)


def assert_attribution(att, want, loss_all=True):
    pairs = dict(kernel="idx", loss_ns="loss", tail_ns="tail_ns", total_ns="total_ns",
                 tail_calls="tail_calls", threshold_bucket="thr_bucket", base_share="base_share")
    for mine, theirs in pairs.items():
        g, w = getattr(att, mine), getattr(want, theirs)
        assert g.shape == w.shape and g.dtype == w.dtype, mine
        assert np.array_equal(g, w, equal_nan=True), mine
        if w.dtype == np.float64:
            ok = ~np.isnan(w)
            assert np.array_equal(g.view(np.uint64)[ok], w.view(np.uint64)[ok]), mine
    got = att.loss_all.cpu().numpy()
    assert np.array_equal(got.view(np.uint64)[~np.isnan(got)],
                          want.loss_all.view(np.uint64)[~np.isnan(want.loss_all)])
    assert np.array_equal(np.isnan(got), np.isnan(want.loss_all))


def same_fields(a, b, skip=("attribution", "tail_calls")):
    for f, v in vars(a).items():
        if f in skip:
            continue
        w = getattr(b, f)
        if isinstance(v, np.ndarray):
            assert v.dtype == w.dtype and np.array_equal(v.view(np.uint8), w.view(np.uint8)), f
        else:
            assert v == w or (v != v and w != w), f


def test_reporter_tail_scores_attribute():
    rep, counts = reporter_counts(11)
    plain = rep.tail_scores(counts, permille=950)
    assert plain.attribution is None
    got = rep.tail_scores(counts, permille=950, attribute=4)
    same_fields(got, plain)
    again = rep.tail_scores(counts, permille=950, attribute=0)
    same_fields(again, plain)
    assert again.attribution is None
    c = counts.cpu().numpy().view(np.uint32)
    assert_attribution(got.attribution, histograms.tail_attribution(c, 950, 4))
    assert got.attribution.kernel.shape == (R_, 4) and got.attribution.kernel[2, 0] >= 0
    # another top reuses the reporter's buffers
    assert_attribution(rep.tail_scores(counts, permille=950, attribute=16).attribution,
                       histograms.tail_attribution(c, 950, 16))


@pytest.mark.parametrize("absorb", ["always", "healthy", "never"])
def test_reporter_individual_tail_scores_attribute(absorb):
    rep_a, c0 = reporter_counts(21)
    rep_b, _ = reporter_counts(21)
    ns1 = synth.synth_matrix(R_, K_, S_, seed=22, device=DEV)
    ns1[2, :, ::7] *= 3
    c1 = rep_a.histograms(ns1, S_)
    h = np.zeros((R_, K_, 240), np.uint32)
    for c in (c0, c1, c1):
        a = rep_a.individual_tail_scores(c, permille=950, threshold=0.9, absorb=absorb, attribute=4)
        b = rep_b.individual_tail_scores(c, permille=950, threshold=0.9, absorb=absorb)
        assert b.attribution is None
        same_fields(a, b)
        assert torch.equal(rep_a._htail["hist"], rep_b._htail["hist"])
        ch = c.cpu().numpy().view(np.uint32)
        assert_attribution(a.attribution, histograms.history_attribution(ch, h, 950, 4))
        skip = a.stragglers if absorb == "healthy" else None
        if absorb != "never":
            h = histograms.history_scores(ch, h, 950, score=False, skip_rows=skip).hist
        assert np.array_equal(rep_a._htail["hist"].cpu().numpy().view(np.uint32), h)
    assert bool((a.attribution.kernel >= 0).all()) == (absorb != "never")


def test_reporter_rejects_a_bad_attribute():
    rep, counts = reporter_counts(31)
    for bad in (17, -1, True, 2.5):
        with pytest.raises(ValueError, match="top"):
            rep.tail_scores(counts, attribute=bad)
        with pytest.raises(ValueError, match="top"):
            rep.individual_tail_scores(counts, attribute=bad)
