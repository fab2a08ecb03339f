"""GPU: the tail score attribution straight from ragged segments (segment_tail_attribution.hip)
against the dense chain it replaces (``segment_histogram_ragged`` counts ->
``histogram_tail_attribution(kind="relative")``) and against the host twin.  Every sum is an exact
integer, so every comparison is equality: integers as they are, f64 by bit pattern, NaN against
NaN.  The cases (``_segment_tail_attr_cases``) sit on the kernels' boundaries."""
import numpy as np
import pytest
import torch

import _segment_tail_attr_cases as C
import _tail_ref as ref
from nvidia_resiliency_ext.straggler import ops

pytestmark = pytest.mark.gpu
CASES = C.cases()
FIELDS = ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share", "loss_all")
DEV = "cuda"


def _dev(s):
    return (torch.from_numpy(s.keys.view(np.int32)).to(DEV), torch.from_numpy(s.off).to(DEV),
            torch.from_numpy(s.lens).to(DEV))


def _opt(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def _chain(c, ns, off, lens, out=None):
    """fleet -> threshold -> base -> attribution, every input the device chain's own."""
    s = c.seg
    fleet = ops.segment_fleet_histogram_ragged(ns, off, lens, s.K, s.max_len, cap=s.cap,
                                               aligned16=s.aligned16)
    thr, _ = ops.histogram_tail_threshold(fleet, s.pm, col_valid=_opt(s.col_valid))
    base = ops.histogram_tail_base(fleet, thr)
    got = ops.segment_tail_attribution_ragged(ns, off, lens, s.K, s.max_len, thr, base, top=c.top,
                                              cap=s.cap, aligned16=s.aligned16,
                                              thr_index=_opt(s.thr_index), out=out)
    return got, thr, base


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


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_equals_the_dense_chain_and_the_host_twin(c):
    s = c.seg
    ns, off, lens = _dev(s)
    got, thr, base = _chain(c, ns, off, lens)
    counts = torch.zeros((s.R * s.K, 240), dtype=torch.int32, device=DEV)
    ops.segment_histogram_ragged(ns, off, lens, s.max_len, cap=s.cap, aligned16=s.aligned16, out=counts)
    dense = ops.histogram_tail_attribution(counts.view(s.R, s.K, 240), top=c.top, kind="relative",
                                           thr=thr, thr_index=_opt(s.thr_index), base=base)
    assert_same(got, dense, c.name + " dense")
    assert_same(got, C.twin(c.name), c.name + " twin")
    idx = got.idx.cpu().numpy()
    for (r, j), k in c.planted.items():
        assert idx[r, j] == k


@pytest.mark.parametrize("name", ["only_negative_losses", "fewer_than_top16", "K2100_second_batch"])
def test_outputs_hold_no_stale_values_and_two_calls_agree(name):
    c = C.case(name)
    s = c.seg
    ns, off, lens = _dev(s)
    out = ops.TailAttribution.empty(s.R, s.K, c.top, DEV)
    for f in FIELDS:
        getattr(out, f).view(torch.uint8).fill_(0x5A)
    a, _, _ = _chain(c, ns, off, lens, out=out)
    assert a is out
    assert_same(a, C.twin(name))
    pad = a.idx.cpu().numpy() == -1
    assert pad.any() or name == "K2100_second_batch"
    h = _arrays(a)
    assert np.isnan(h["loss"][pad]).all() and np.isnan(h["base_share"][pad]).all()
    assert not h["tail_ns"][pad].any() and not h["total_ns"][pad].any() and not h["tail_calls"][pad].any()
    assert (h["thr_bucket"][pad] == -1).all()
    b, _, _ = _chain(c, ns, off, lens)
    for f in FIELDS:
        assert torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), f


def test_run_to_run_identity_and_graph_replay():
    """fleet -> threshold -> scores -> base -> attribution, captured, equals eager."""
    c = C.case("R70_K33")
    s = c.seg
    ns, off, lens = _dev(s)
    R, K = s.R, s.K

    def outputs():
        return dict(fleet=torch.empty((K, 240), dtype=torch.int64, device=DEV),
                    thr=torch.empty(K, dtype=torch.int32, device=DEV),
                    sums=torch.zeros(2, dtype=torch.int64, device=DEV),
                    score=ops.TailScores(torch.empty(R, dtype=torch.float64, device=DEV),
                                         torch.empty(R, dtype=torch.int64, device=DEV),
                                         torch.empty(R, dtype=torch.int64, device=DEV),
                                         torch.empty(R, dtype=torch.uint8, device=DEV)),
                    base=torch.empty((K, 2), dtype=torch.int64, device=DEV),
                    attr=ops.TailAttribution.empty(R, K, c.top, DEV))

    def chain(o):
        ops.segment_fleet_histogram_ragged(ns, off, lens, K, s.max_len, cap=s.cap,
                                           aligned16=s.aligned16, out=o["fleet"])
        ops.histogram_tail_threshold(o["fleet"], s.pm, thr=o["thr"], fleet_sums=o["sums"])
        ops.segment_tail_scores_ragged(ns, off, lens, K, s.max_len, o["thr"], o["sums"], cap=s.cap,
                                       aligned16=s.aligned16, out=o["score"])
        ops.histogram_tail_base(o["fleet"], o["thr"], out=o["base"])
        ops.segment_tail_attribution_ragged(ns, off, lens, K, s.max_len, o["thr"], o["base"],
                                            top=c.top, cap=s.cap, aligned16=s.aligned16, out=o["attr"])

    def tensors(o):
        return [o["fleet"], o["thr"], o["sums"], o["score"].score, o["score"].tail_ns,
                o["score"].total_ns, o["score"].strag, o["base"]] + [getattr(o["attr"], f) for f in FIELDS]

    def snapshot(o):
        torch.cuda.synchronize()
        return [t.view(torch.uint8).clone() for t in tensors(o)]

    eager = outputs()
    chain(eager)
    first = snapshot(eager)
    assert_same(eager["attr"], C.twin(c.name))
    chain(eager)
    for x, y in zip(first, snapshot(eager)):
        assert torch.equal(x, y)
    held = outputs()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        chain(held)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(st)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(held)
    for _ in range(2):
        for t in tensors(held):
            t.view(torch.uint8).fill_(0x5A)
        g.replay()
        for x, y in zip(first, snapshot(held)):
            assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["lengths_unaligned", "cap_trims", "long_winner_cap3000",
                                  "K2100_second_batch", "thr_index_permuted"])
def test_winners_equal_python_integer_sums_over_their_windows(name):
    """Independent of the dense chain and of the twin: plain integers over the retained keys."""
    c = C.case(name)
    s = c.seg
    got, thr, _ = _chain(c, *_dev(s))
    h, T = _arrays(got), thr.cpu().tolist()
    win = C.S.windows(s)
    checked = 0
    for r, j in zip(*np.nonzero(h["idx"] >= 0)):
        k = int(h["idx"][r, j])
        t = T[k if s.thr_index is None else int(s.thr_index[k])]
        b = [ref.bucket(int(x)) for x in win[r * s.K + k]]
        assert len(b) > 0 and t >= 0 and h["thr_bucket"][r, j] == t
        assert int(h["total_ns"].view(np.uint64)[r, j]) == sum(ref.W[v] for v in b) & ref.M64
        assert int(h["tail_ns"].view(np.uint64)[r, j]) == sum(ref.W[v] for v in b if v > t) & ref.M64
        assert int(h["tail_calls"].view(np.uint32)[r, j]) == sum(v > t for v in b)
        checked += 1
    assert checked >= 4
