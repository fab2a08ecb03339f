"""GPU: nvrx_histogram_history_attribution_compact against the host twin and against the dense
entry it is defined by (``ops.histogram_tail_attribution(kind="individual")`` on the expanded
history, uploaded dense), on every case of ``_histogram_compact_attr_cases`` -- the table of
``_histogram_compact_cases`` with ``top`` cycling through 1, 4, 8, 16: R x K = 1 x 18 (a trip's
first and last element, a short trip), 1 x 1, 1 x 17, 3 x 37, 2 x 50 (several splits, a short last
split), 2049 x 1 (one split per row, more than 2,048 rows), ``hist_stride > K``, a permuted
``hist_index`` with negative entries, ``col_valid`` zeros, permille 0 / 500 / 990 / 1000, and the
full-u32 bins record streams cannot produce -- and, on the counts of their segments, on every case
and step of ``_compact_attr_cases`` against the record-stream twin (K = 4,100: the select's second
batch; ties).  Every field byte for byte, so NaN and the sign of zero count; no tolerance.  Every
output is pre-filled with 0x5A; ``chist`` (sentinel slots included) carries a 64-byte guard behind
it and is bit-identical after the call."""
import numpy as np
import pytest
import torch

import _compact_attr_cases as X
import _histogram_compact_attr_cases as A
from nvidia_resiliency_ext.straggler import histograms, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 0x5E
FIELDS = A.FIELDS


def dev(a, dt=np.int32):
    return torch.from_numpy(np.array(a).view(dt)).to(DEV)  # a copy: the cases are read only


def opt(v, dt):
    return None if v is None else torch.as_tensor(np.asarray(v), dtype=dt).to(DEV)


def guarded(chist):
    """A device copy of a compact history with 64 guard bytes behind it: (the view, the whole)."""
    whole = torch.full((chist.size + 64,), GUARD, dtype=torch.uint8, device=DEV)
    view = whole[:chist.size].view(chist.shape)
    view.copy_(torch.from_numpy(chist.copy()).to(DEV))
    return view, whole


def garbage_out(R, K, top):
    out = ops.TailAttribution.empty(R, K, top, DEV)
    for f in FIELDS:
        getattr(out, f).view(torch.uint8).fill_(0x5A)
    return out


def _bytes(res):
    out = {}
    for f in FIELDS:
        v = getattr(res, f)
        out[f] = np.ascontiguousarray(v.cpu().numpy() if isinstance(v, torch.Tensor) else v)
    return out


def assert_same(got, want, what=""):
    g, w = _bytes(got), _bytes(want)
    for f in FIELDS:
        assert g[f].shape == w[f].shape and g[f].dtype.itemsize == w[f].dtype.itemsize, (what, f)
        assert g[f].tobytes() == w[f].tobytes(), (what, f)


def kwargs(c, top):
    return dict(permille=c.pm, top=top, hist_index=opt(c.hist_index, torch.int32),
                hist_stride=c.stride, col_valid=opt(c.col_valid, torch.uint8))


def untouched(whole, chist):
    after = whole.cpu().numpy()
    assert after[:chist.size].tobytes() == chist.tobytes()  # read only, sentinels included
    assert (after[chist.size:] == GUARD).all()


@pytest.mark.parametrize("c", A.cases(), ids=lambda c: c.name)
def test_equals_the_host_twin_and_the_dense_entry(c):
    top = A.top_of(c.name)
    kw = kwargs(c, top)
    d_counts = dev(c.counts)
    d_chist, whole = guarded(c.chist0)
    out = garbage_out(c.R, c.K, top)
    got = ops.histogram_history_attribution_compact(d_counts, d_chist, out=out, **kw)
    assert got is out
    assert_same(got, A.twin(c.name), "twin")
    dense = ops.histogram_tail_attribution(d_counts, kind="individual", hist=dev(A.dense_of(c)), **kw)
    assert_same(got, dense, "dense")
    untouched(whole, c.chist0)


@pytest.mark.parametrize("c", X.cases(), ids=lambda c: c.name)
def test_on_segment_counts_equals_the_record_stream_twin(c):
    kw = kwargs(c, c.top)
    for s, twin in zip(c.steps, X.twin(c.name)):
        iv = s.iv
        counts = histograms.segment_counts(iv.keys, iv.off, iv.lens, c.K, iv.cap).astype(np.uint32)
        d_chist, whole = guarded(s.chist)
        got = ops.histogram_history_attribution_compact(dev(counts), d_chist,
                                                        out=garbage_out(c.R, c.K, c.top), **kw)
        assert_same(got, twin, iv.name)
        untouched(whole, s.chist)


@pytest.mark.parametrize("name", ["R2_K50", "all_three", "elem_all_240_bins", "R2049_K1"])
def test_two_identical_calls_give_identical_bytes(name):
    c = A.case(name)
    kw = kwargs(c, A.top_of(name))
    d_counts, d_chist = dev(c.counts), dev(c.chist0, np.uint8)
    a = ops.histogram_history_attribution_compact(d_counts, d_chist, **kw)
    b = ops.histogram_history_attribution_compact(d_counts, d_chist, **kw)
    for f in FIELDS:
        assert torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), f


@pytest.mark.parametrize("name", ["R3_K37", "stride_and_index", "weightless_history"])
def test_packed_out_equals_unpacked(name):
    c = A.case(name)
    R, K, top = c.R, c.K, A.top_of(name)
    kw = kwargs(c, top)
    d_counts, d_chist = dev(c.counts), dev(c.chist0, np.uint8)
    plain = ops.histogram_history_attribution_compact(d_counts, d_chist, **kw)
    buf = torch.full((ops.TailAttribution.PACKED * R * top,), 0x5A, dtype=torch.uint8, device=DEV)
    loss_all = torch.full((R, K), 7.0, dtype=torch.float64, device=DEV)
    got = ops.histogram_history_attribution_compact(
        d_counts, d_chist, out=ops.TailAttribution.packed(buf, R, top, loss_all), **kw)
    assert_same(got, plain)
    host = ops.TailAttribution.unpack(buf.cpu().numpy(), R, top)
    want = _bytes(plain)
    for f, a in zip(FIELDS[:-1], host):
        assert a.tobytes() == want[f].tobytes(), f


def test_captured_once_as_a_linear_chain_and_replayed_on_changed_inputs():
    first, second = A.case("R3_K37"), A.case("col_valid")  # one shape, other elements and validity
    assert (first.R, first.K) == (second.R, second.K)
    top = 8
    d_counts, d_chist = dev(first.counts), dev(first.chist0, np.uint8)
    valid = torch.ones(first.K, dtype=torch.uint8, device=DEV)
    kw = dict(permille=first.pm, top=top, col_valid=valid)
    out = garbage_out(first.R, first.K, top)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm up outside the capture
        ops.histogram_history_attribution_compact(d_counts, d_chist, out=out, **kw)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.histogram_history_attribution_compact(d_counts, d_chist, out=out, **kw)
    for c in (first, second, first):
        d_counts.copy_(dev(np.roll(c.counts, 1, axis=0)))
        d_chist.copy_(dev(np.roll(c.chist0, 1, axis=0), np.uint8))
        valid.copy_(torch.ones_like(valid) if c.col_valid is None else opt(c.col_valid, torch.uint8))
        for f in FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0x5A)
        g.replay()
        torch.cuda.synchronize()
        eager = ops.histogram_history_attribution_compact(d_counts, d_chist, **kw)
        assert_same(out, eager, c.name)
        want = histograms.compact_history_attribution(
            np.roll(c.counts, 1, axis=0), np.roll(c.chist0, 1, axis=0), first.pm, top,
            col_valid=valid.cpu().numpy())
        assert_same(out, want, c.name)


def test_wrapper_refuses_a_dense_history_and_a_wrong_shape():
    c = A.case("R1_K17")
    d_counts = dev(c.counts)
    with pytest.raises(ValueError, match="chist"):
        ops.histogram_history_attribution_compact(d_counts, dev(A.dense_of(c)), permille=950, top=4)
    with pytest.raises(ValueError, match="chist"):
        ops.histogram_history_attribution_compact(
            d_counts, torch.zeros((c.R, c.K + 1, 64), dtype=torch.uint8, device=DEV), permille=950, top=4)
    with pytest.raises(ValueError, match="chist"):
        ops.histogram_history_attribution_compact(
            d_counts, torch.zeros((c.R, c.K, 64), dtype=torch.int32, device=DEV), permille=950, top=4)
