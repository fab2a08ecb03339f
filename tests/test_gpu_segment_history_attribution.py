"""GPU: nvrx_segment_history_attribution_ragged against the dense chain it is defined by
(``segment_histogram_ragged`` into a zeroed matrix, then ``histogram_tail_attribution(kind=
"individual")``) and against the host twin, on every case and interval of
``_segment_history_attr_cases`` with the history before that interval: integers equal, f64 bit
patterns equal, the NaN pattern of the whole ``loss_all`` equal; no tolerance.  Every output is
pre-filled with garbage, ``hist`` (sentinel slots included) carries a guard word and is
bit-identical after the call."""
import numpy as np
import pytest
import torch

import _segment_history_attr_cases as C
from nvidia_resiliency_ext.straggler import ops

pytestmark = pytest.mark.gpu

BINS = 240
DEV = "cuda"
GUARD = 0x5EED5EED
CASES = C.cases()
FIELDS = ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share", "loss_all")


def dev(a, dt=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV)


def guarded(a):
    """A device copy of a u32 array with a guard word behind it: (the view, the whole)."""
    whole = torch.full((a.size + 4,), GUARD, dtype=torch.int32, device=DEV)
    view = whole[:a.size].view(a.shape)
    view.copy_(dev(a))
    return view, whole


def guard_ok(whole):
    return whole[-4:].cpu().tolist() == [GUARD] * 4


def garbage_out(R, K, top):
    out = ops.TailAttribution.empty(R, K, top, DEV)
    for f in FIELDS:
        getattr(out, f).view(torch.uint8).fill_(0x5A)
    return out


def _arrays(res):
    out = {}
    for f in FIELDS:
        v = getattr(res, f)
        out[f] = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return out


def assert_same(got, want, what=""):
    """Bit for bit; NaN is one pattern ("not taken")."""
    g, w = _arrays(got), _arrays(want)
    for f in FIELDS:
        a, b = g[f], w[f]
        assert a.shape == b.shape, (what, f)
        if b.dtype == np.float64:
            an, bn = np.isnan(a), np.isnan(b)
            assert np.array_equal(an, bn), (what, f)
            assert np.array_equal(a.view(np.uint64)[~an], b.view(np.uint64)[~bn]), (what, f)
        else:
            assert a.dtype.itemsize == b.dtype.itemsize, (what, f)
            assert np.array_equal(a.view(b.dtype), b), (what, f)


class Interval:
    """One interval of a case on the device: the ragged triple and the history keywords."""

    def __init__(self, c, iv):
        h = c.h
        self.c, self.h, self.iv = c, h, iv
        self.keys, self.off, self.lens = dev(iv.keys), dev(iv.off, np.int64), dev(iv.lens)
        self.max_len = max(iv.max_len, 1)
        opt = lambda v, dt: None if v is None else torch.as_tensor(np.asarray(v), dtype=dt).to(DEV)  # noqa: E731
        self.kw = dict(hist_index=opt(h.hist_index, torch.int32), hist_stride=h.stride,
                       col_valid=opt(h.col_valid, torch.uint8))

    def new(self, d_hist, out=None, lens="own", off=None, keys=None):
        return ops.segment_history_attribution_ragged(
            self.keys if keys is None else keys, self.off if off is None else off,
            self.lens if isinstance(lens, str) else lens, self.h.K, self.max_len, d_hist,
            permille=self.h.pm, top=self.c.top, cap=self.iv.cap, aligned16=self.iv.aligned16, out=out,
            **self.kw)

    def dense(self, d_hist):
        h = self.h
        counts = torch.zeros((h.R * h.K, BINS), dtype=torch.int32, device=DEV)
        ops.segment_histogram_ragged(self.keys, self.off, self.lens, self.max_len, cap=self.iv.cap,
                                     aligned16=self.iv.aligned16, out=counts)
        return ops.histogram_tail_attribution(counts.view(h.R, h.K, BINS), top=self.c.top,
                                              kind="individual", hist=d_hist, permille=h.pm, **self.kw)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_equals_the_dense_chain_and_the_host_twin(c):
    h = c.h
    for i, (iv, (_, before, _), twin) in enumerate(zip(h.intervals, C.walk(c.name), C.twin(c.name))):
        I = Interval(c, iv)
        d_hist, whole = guarded(before)
        out = garbage_out(h.R, h.K, c.top)
        got = I.new(d_hist, out=out)
        assert got is out
        assert guard_ok(whole)
        assert np.array_equal(d_hist.cpu().numpy().view(np.uint32), before)  # read only, sentinels included
        assert_same(got, I.dense(dev(before)), (iv.name, "dense"))
        assert_same(got, twin, (iv.name, "twin"))
        idx = got.idx.cpu().numpy()
        for (pi, r, j), k in c.planted.items():
            assert pi != i or idx[r, j] == k


@pytest.mark.parametrize("name", ["few_and_none", "bucket0_history", "negative_lengths"])
def test_outputs_hold_no_stale_values(name):
    c = C.case(name)
    h, iv, (_, before, _), twin = c.h, c.h.intervals[0], C.walk(name)[0], C.twin(name)[0]
    got = _arrays(Interval(c, iv).new(dev(before), out=garbage_out(h.R, h.K, c.top)))
    pad = got["idx"] == -1
    assert pad.any()
    assert np.isnan(got["loss"][pad]).all() and np.isnan(got["base_share"][pad]).all()
    assert not got["tail_ns"][pad].any() and not got["total_ns"][pad].any() and not got["tail_calls"][pad].any()
    assert (got["thr_bucket"][pad] == -1).all()
    assert np.array_equal(np.isnan(got["loss_all"]), np.isnan(twin.loss_all))


@pytest.mark.parametrize("name", ["winner_lengths", "ties", "empty_and_filled"])
def test_offsets_without_lengths(name):
    """seg_len NULL: seg_off holds R * K + 1 offsets of back-to-back segments."""
    c = C.case(name)
    h = c.h
    for iv, (_, before, _), twin in zip(h.intervals, C.walk(name), C.twin(name)):
        lens = np.maximum(iv.lens, 0).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        parts = [iv.keys[int(o):int(o) + int(n)] for o, n in zip(iv.off, lens)] + [np.zeros(8, np.uint32)]
        I = Interval(c, iv)
        I.iv = iv._replace(aligned16=False)
        got = I.new(dev(before), lens=None, off=dev(off, np.int64), keys=dev(np.concatenate(parts)))
        assert_same(got, twin, iv.name)


@pytest.mark.parametrize("name", ["R70_K33", "K4100"])
def test_two_identical_calls_give_identical_bits(name):
    c = C.case(name)
    iv, (_, before, _) = c.h.intervals[-1], C.walk(name)[-1]
    I = Interval(c, iv)
    d_hist = dev(before)
    a, b = I.new(d_hist), I.new(d_hist)
    for f in FIELDS:
        assert torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), f


def test_graph_capture_of_score_attribution_update():
    """score -> attribution -> update on one stream, captured: two replays from the restored
    history give the eager bits, and the attribution saw the history the score saw."""
    c = C.case("R70_K33")
    h = c.h
    iv, (_, before, score_twin), twin = h.intervals[-1], C.walk(c.name)[-1], C.twin(c.name)[-1]
    I = Interval(c, iv)
    d_hist = dev(before)
    scores = ops.HistoryTailScores.empty(h.R, DEV)
    attr = garbage_out(h.R, h.K, c.top)

    def chain():
        kw = dict(permille=h.pm, cap=iv.cap, aligned16=iv.aligned16, **I.kw)
        ops.segment_history_scores_ragged(I.keys, I.off, I.lens, h.K, I.max_len, d_hist, update=False,
                                          score_thr=0.9, out=scores, **kw)
        I.new(d_hist, out=attr)
        ops.segment_history_scores_ragged(I.keys, I.off, I.lens, h.K, I.max_len, d_hist, score=False, **kw)

    chain()  # the kernels are loaded before the capture
    torch.cuda.synchronize()
    assert_same(attr, twin, "eager")
    assert np.array_equal(d_hist.cpu().numpy().view(np.uint32), score_twin.hist)
    first = [getattr(attr, f).view(torch.uint8).clone() for f in FIELDS]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    for _ in range(2):
        d_hist.copy_(dev(before))  # the history is restored between replays
        for f in FIELDS:
            getattr(attr, f).view(torch.uint8).fill_(0x5A)
        g.replay()
        torch.cuda.synchronize()
        for f, x in zip(FIELDS, first):
            assert torch.equal(getattr(attr, f).view(torch.uint8), x), f
        assert scores.score.cpu().numpy().tobytes() == score_twin.score.tobytes()
        assert np.array_equal(d_hist.cpu().numpy().view(np.uint32), score_twin.hist)
