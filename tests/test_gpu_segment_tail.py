"""GPU: the tail scores straight from ragged segments (segment_tail.hip) against the dense chain
they replace and against the host twin.  Every sum is an exact integer, so every comparison is
equality: u64, u32, u8, and f64 by bit pattern.  The cases (``_segment_tail_cases``) sit on the
kernels' boundaries."""
import numpy as np
import pytest
import torch

import _segment_tail_cases as C
import _tail_ref as ref
from nvidia_resiliency_ext.straggler import histograms, ops

pytestmark = pytest.mark.gpu
CASES = C.cases()


def _dev(c):
    d = "cuda"
    return (torch.from_numpy(c.keys.view(np.int32)).to(d), torch.from_numpy(c.off).to(d),
            torch.from_numpy(c.lens).to(d))


def _dense(c, ns, off, lens):
    """The dense chain's counts: segment_histogram_ragged into a zeroed matrix."""
    counts = torch.zeros((c.R * c.K, 240), dtype=torch.int32, device=ns.device)
    ops.segment_histogram_ragged(ns, off, lens, c.max_len, cap=c.cap, aligned16=c.aligned16, out=counts)
    return counts.view(c.R, c.K, 240)


def _fleet(c, ns, off, lens, **kw):
    return ops.segment_fleet_histogram_ragged(ns, off, lens, c.K, c.max_len, cap=c.cap,
                                              aligned16=c.aligned16, **kw)


def _tail(c, ns, off, lens, thr, sums, ti, **kw):
    return ops.segment_tail_scores_ragged(ns, off, lens, c.K, c.max_len, thr, sums, cap=c.cap,
                                          aligned16=c.aligned16, thr_index=ti, **kw)


def _same(a: ops.TailScores, b: ops.TailScores):
    assert torch.equal(a.score.view(torch.int64), b.score.view(torch.int64))
    assert torch.equal(a.tail_ns, b.tail_ns) and torch.equal(a.total_ns, b.total_ns)
    assert torch.equal(a.strag, b.strag)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_equals_the_dense_chain_and_the_host_twin(c):
    ns, off, lens = _dev(c)
    counts = _dense(c, ns, off, lens)
    fleet = _fleet(c, ns, off, lens)
    assert torch.equal(fleet, ops.histogram_sum(counts))
    valid = None if c.col_valid is None else torch.from_numpy(c.col_valid).cuda()
    ti = None if c.thr_index is None else torch.from_numpy(c.thr_index).cuda()
    thr, sums = ops.histogram_tail_threshold(fleet, c.pm, col_valid=valid)
    dense = ops.histogram_tail_scores(counts, thr, sums, thr_index=ti, tail_calls=True, score_thr=0.97)
    new = _tail(c, ns, off, lens, thr, sums, ti, tail_calls=True, score_thr=0.97)
    _same(new, dense)
    assert torch.equal(new.tail_calls, dense.tail_calls)
    # tail_calls off: the other instantiation gives the same scores
    bare = _tail(c, ns, off, lens, thr, sums, ti, score_thr=0.97)
    assert bare.tail_calls is None
    _same(bare, dense)
    # zeros where a column is skipped
    T = thr.cpu().numpy()
    tk = T if c.thr_index is None else np.where(c.thr_index >= 0, T[np.maximum(c.thr_index, 0)], -1)
    assert not new.tail_calls.cpu().numpy()[:, tk < 0].any()
    # the definition in Python integers, and the host twin
    win = C.windows(c)
    hc = [[ref.hist_of(w) for w in win[r * c.K:(r + 1) * c.K]] for r in range(c.R)]
    rows = ref.scores(hc, T.tolist(), tuple(int(v) & ref.M64 for v in sums.cpu().tolist()), 0.97,
                      None if c.thr_index is None else c.thr_index.tolist())
    assert new.tail_ns.cpu().numpy().view(np.uint64).tolist() == [r["tail_ns"] for r in rows]
    assert new.total_ns.cpu().numpy().view(np.uint64).tolist() == [r["total_ns"] for r in rows]
    assert [ref.bits(s) for s in new.score.cpu().tolist()] == [ref.bits(r["score"]) for r in rows]
    assert new.strag.cpu().numpy().astype(bool).tolist() == [r["strag"] for r in rows]
    assert new.tail_calls.cpu().numpy().view(np.uint32).tolist() == [r["calls"] for r in rows]
    assert fleet.cpu().numpy().tolist() == histograms.segment_counts(c.keys, c.off, c.lens, c.K, c.cap).sum(0).tolist()
    if c.thr_index is None:
        twin = histograms.segment_tail_scores(c.keys, c.off, c.lens, c.K, c.pm, c.cap, c.col_valid)
        assert twin.threshold_bucket.tolist() == T.tolist()
        assert twin.tail_ns.tolist() == [r["tail_ns"] for r in rows]
        assert twin.total_ns.tolist() == [r["total_ns"] for r in rows]
        assert [ref.bits(s) for s in twin.score] == [ref.bits(r["score"]) for r in rows]
        assert twin.tail_calls.tolist() == [r["calls"] for r in rows]


def test_all_zero_world_is_nan_and_never_flagged():
    c = next(c for c in CASES if c.name == "all_zero_world")
    ns, off, lens = _dev(c)
    fleet = _fleet(c, ns, off, lens)
    thr, sums = ops.histogram_tail_threshold(fleet, c.pm)
    got = _tail(c, ns, off, lens, thr, sums, None, score_thr=2.0)
    assert torch.isnan(got.score).all() and not got.strag.any() and not got.total_ns.any()
    assert int(fleet[:, 0].sum()) == int(fleet.sum()) > 0


def test_a_column_wholly_in_bucket_zero_adds_nothing():
    c = next(c for c in CASES if c.name == "special_keys")
    ns, off, lens = _dev(c)
    fleet = _fleet(c, ns, off, lens).cpu().numpy()
    assert fleet[0, 1:].sum() == 0 and fleet[0, 0] > 0 and fleet[2, 237:].all()
    assert fleet[1, 7] > 0 and fleet[1, 8] > 0 and fleet[1].sum() == fleet[1, 7] + fleet[1, 8]


def test_accumulate_adds_two_intervals():
    a, b = (next(c for c in CASES if c.name == n) for n in ("lengths_unaligned", "lengths_aligned16"))
    fa, fb = _fleet(a, *_dev(a)), _fleet(b, *_dev(b))
    both = fa.clone()
    assert _fleet(b, *_dev(b), out=both, accumulate=True) is both
    assert torch.equal(both, fa + fb)
    with pytest.raises(ValueError, match="accumulate"):
        _fleet(a, *_dev(a), accumulate=True)


def test_run_to_run_identity_and_graph_replay():
    c = next(c for c in CASES if c.name == "R70_K33")
    ns, off, lens = _dev(c)
    d = ns.device

    def outputs():
        return (torch.empty((c.K, 240), dtype=torch.int64, device=d),
                torch.empty(c.K, dtype=torch.int32, device=d), torch.zeros(2, dtype=torch.int64, device=d),
                ops.TailScores(torch.empty(c.R, dtype=torch.float64, device=d),
                               torch.empty(c.R, dtype=torch.int64, device=d),
                               torch.empty(c.R, dtype=torch.int64, device=d),
                               torch.empty(c.R, dtype=torch.uint8, device=d),
                               torch.empty((c.R, c.K), dtype=torch.int32, device=d)))

    def chain(fleet, thr, sums, out):
        _fleet(c, ns, off, lens, out=fleet)
        ops.histogram_tail_threshold(fleet, c.pm, thr=thr, fleet_sums=sums)
        _tail(c, ns, off, lens, thr, sums, None, out=out, tail_calls=True)

    def snapshot(fleet, thr, sums, out):
        torch.cuda.synchronize()
        return [t.clone() for t in (fleet, thr, sums, out.score.view(torch.int64), out.tail_ns,
                                    out.total_ns, out.strag, out.tail_calls)]

    eager = outputs()
    chain(*eager)
    first = snapshot(*eager)
    chain(*eager)
    for x, y in zip(first, snapshot(*eager)):
        assert torch.equal(x, y)
    held = outputs()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain(*held)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(*held)
    for _ in range(2):
        for t in (held[0], held[1], held[2], held[3].tail_ns, held[3].tail_calls):
            t.fill_(-7)
        g.replay()
        for x, y in zip(first, snapshot(*held)):
            assert torch.equal(x, y)
