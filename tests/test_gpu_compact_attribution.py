"""GPU: nvrx_segment_history_attribution_compact_ragged against the host twin and against the
dense entry it is defined by (``ops.segment_history_attribution_ragged`` on the expanded history,
uploaded dense), on every case and step of ``_compact_attr_cases``: every field byte for byte, so
NaN and the sign of zero count; no tolerance.  Every output is pre-filled with garbage; ``chist``
(sentinel slots included) carries a guard behind it and is bit-identical after the call."""
import numpy as np
import pytest
import torch

import _compact_attr_cases as X
from nvidia_resiliency_ext.straggler import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 0x5E
CASES = X.cases()
FIELDS = ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share", "loss_all")


def dev(a, dt=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV)


def guarded(chist):
    """A device copy of a compact history with 64 guard bytes behind it: (the view, the whole)."""
    whole = torch.full((chist.size + 64,), GUARD, dtype=torch.uint8, device=DEV)
    view = whole[:chist.size].view(chist.shape)
    view.copy_(torch.from_numpy(chist.copy()).to(DEV))  # the case's array is read only
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


class OnDevice:
    """One step of a case on the device: the ragged triple and the history keywords."""

    def __init__(self, c, s):
        iv = s.iv
        self.c, self.s, self.iv = c, s, iv
        self.keys, self.off, self.lens = dev(iv.keys), dev(iv.off, np.int64), dev(iv.lens)
        self.max_len = max(iv.max_len, 1)
        opt = lambda v, dt: None if v is None else torch.as_tensor(np.asarray(v), dtype=dt).to(DEV)  # noqa: E731
        self.kw = dict(permille=c.pm, top=c.top, cap=iv.cap, aligned16=iv.aligned16,
                       hist_index=opt(c.hist_index, torch.int32), hist_stride=c.stride,
                       col_valid=opt(c.col_valid, torch.uint8))

    def compact(self, d_chist, out=None):
        return ops.segment_history_attribution_compact_ragged(self.keys, self.off, self.lens, self.c.K,
                                                              self.max_len, d_chist, out=out, **self.kw)

    def dense(self):
        d_hist = dev(X.dense_of(self.c, self.s.chist))
        return ops.segment_history_attribution_ragged(self.keys, self.off, self.lens, self.c.K,
                                                      self.max_len, d_hist, **self.kw)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_equals_the_host_twin_and_the_dense_entry(c):
    for s, twin in zip(c.steps, X.twin(c.name)):
        D = OnDevice(c, s)
        d_chist, whole = guarded(s.chist)
        out = garbage_out(c.R, c.K, c.top)
        got = D.compact(d_chist, out=out)
        assert got is out
        assert_same(got, twin, (s.iv.name, "twin"))
        assert_same(got, D.dense(), (s.iv.name, "dense"))
        after = whole.cpu().numpy()
        assert after[:s.chist.size].tobytes() == s.chist.tobytes()  # read only, sentinels included
        assert (after[s.chist.size:] == GUARD).all()


@pytest.mark.parametrize("name", ["hist/R70_K33", "attr/K4100", "hist/fold_rule", "new/K17_rows_past_K"])
def test_two_identical_calls_give_identical_bytes(name):
    c = X.case(name)
    s = c.steps[-1]
    D = OnDevice(c, s)
    d_chist = torch.from_numpy(s.chist.copy()).to(DEV)
    a, b = D.compact(d_chist), D.compact(d_chist)
    for f in FIELDS:
        assert torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), f


@pytest.mark.parametrize("name", ["attr/ties", "hist/hist_index_permuted", "new/four_rows_four_rotations"])
def test_packed_out_equals_unpacked(name):
    c = X.case(name)
    R, K, top = c.R, c.K, c.top
    for s in c.steps:
        D = OnDevice(c, s)
        d_chist = torch.from_numpy(s.chist.copy()).to(DEV)
        plain = D.compact(d_chist)
        buf = torch.full((ops.TailAttribution.PACKED * R * top,), 0x5A, dtype=torch.uint8, device=DEV)
        loss_all = torch.full((R, K), 7.0, dtype=torch.float64, device=DEV)
        got = D.compact(d_chist, out=ops.TailAttribution.packed(buf, R, top, loss_all))
        assert_same(got, plain, s.iv.name)
        host = ops.TailAttribution.unpack(buf.cpu().numpy(), R, top)
        want = _bytes(plain)
        for f, a in zip(FIELDS[:-1], host):
            assert a.tobytes() == want[f].tobytes(), (s.iv.name, f)


def test_wrapper_refuses_a_dense_history_and_a_wrong_shape():
    c = X.case("new/rank_on_entry_boundary")
    s = c.steps[0]
    D = OnDevice(c, s)
    with pytest.raises(ValueError, match="chist"):
        D.compact(dev(X.dense_of(c, s.chist)))
    with pytest.raises(ValueError, match="chist"):
        D.compact(torch.zeros((c.R, c.K + 1, 64), dtype=torch.uint8, device=DEV))
