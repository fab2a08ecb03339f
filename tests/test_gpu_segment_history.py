"""GPU: nvrx_segment_history_scores_ragged against the dense chain it is defined by
(``segment_histogram_ragged`` into a zeroed matrix, then ``histogram_history_scores``) on two
copies of the same history, and against the host twin and the plain-Python definition
(``_history_tail_ref``): integers equal, f64 bit patterns equal (NaN as NaN), the whole history
tensor equal, sentinel slots included; no tolerance.  Every output is pre-filled with a sentinel,
and a guard word follows ``hist`` and ``tail_calls``."""
import numpy as np
import pytest
import torch

import _history_tail_ref as HREF
import _segment_history_cases as C
from nvidia_resiliency_ext.straggler import ops

pytestmark = pytest.mark.gpu

BINS = 240
DEV = "cuda"
SENT = -7
GUARD = 0x5EED5EED
THR = 0.9
BOTH = HREF.SCORE | HREF.UPDATE
MODES = (HREF.SCORE, HREF.UPDATE, BOTH)
CASES = C.cases()
SUMS = ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns")


def dev(a, dt=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV)


def guarded(a):
    """A device copy of a u32 / i32 array with a guard word behind it: (the view, the whole)."""
    whole = torch.full((a.size + 4,), GUARD, dtype=torch.int32, device=DEV)
    view = whole[:a.size].view(a.shape)
    view.copy_(dev(a))
    return view, whole


def guard_ok(whole):
    return whole[-4:].cpu().tolist() == [GUARD] * 4


def sentinel_out(R):
    i = lambda: torch.full((R,), SENT, dtype=torch.int64, device=DEV)  # noqa: E731
    return ops.HistoryTailScores(torch.full((R,), float(SENT), dtype=torch.float64, device=DEV),
                                 i(), i(), i(), i(), torch.full((R,), 9, dtype=torch.uint8, device=DEV))


def untouched(out):
    R = out.score.numel()
    return (out.score.cpu().tolist() == [float(SENT)] * R and out.strag.cpu().tolist() == [9] * R and
            all(getattr(out, n).cpu().tolist() == [SENT] * R for n in SUMS))


class Interval:
    """One interval of a case on the device: the ragged triple, uploaded once."""

    def __init__(self, c, iv):
        self.c, self.iv = c, iv
        self.keys, self.off, self.lens = dev(iv.keys), dev(iv.off, np.int64), dev(iv.lens)
        self.max_len = max(iv.max_len, 1)
        opt = lambda v, dt: None if v is None else torch.as_tensor(np.asarray(v), dtype=dt).to(DEV)  # noqa: E731
        self.kw = dict(hist_index=opt(c.hist_index, torch.int32), hist_stride=c.stride,
                       col_valid=opt(c.col_valid, torch.uint8))
        self.skip = opt(c.skip_rows, torch.uint8)

    def new(self, d_hist, mode, calls, skip="case", out=None):
        c = self.c
        out = sentinel_out(c.R) if out is None else out
        tc = whole = None
        if calls:
            tc, whole = guarded(np.full((c.R, c.K), SENT, np.int32))
        res = ops.segment_history_scores_ragged(
            self.keys, self.off, self.lens, c.K, self.max_len, d_hist, permille=c.pm,
            score=bool(mode & HREF.SCORE), update=bool(mode & HREF.UPDATE), cap=self.iv.cap,
            aligned16=self.iv.aligned16, skip_rows=self.skip if isinstance(skip, str) else skip,
            score_thr=THR, tail_calls=tc if calls else False, out=out, **self.kw)
        assert whole is None or guard_ok(whole)
        return res, out, tc

    def counts(self):
        c = self.c
        counts = torch.zeros((c.R, c.K, BINS), dtype=torch.int32, device=DEV)
        ops.segment_histogram_ragged(self.keys, self.off, self.lens, self.max_len, cap=self.iv.cap,
                                     aligned16=self.iv.aligned16, out=counts.view(-1, BINS))
        return counts

    def dense(self, counts, d_hist, mode, calls, skip="case"):
        c = self.c
        out = sentinel_out(c.R)
        tc = torch.full((c.R, c.K), SENT, dtype=torch.int32, device=DEV) if calls else False
        res = ops.histogram_history_scores(
            counts, d_hist, permille=c.pm, score=bool(mode & HREF.SCORE),
            update=bool(mode & HREF.UPDATE), skip_rows=self.skip if isinstance(skip, str) else skip,
            score_thr=THR, tail_calls=tc, out=out, **self.kw)
        return res, out


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def assert_same_outputs(a, b, calls):
    for n in SUMS + ("score", "strag"):
        assert same_bits(getattr(a, n), getattr(b, n)), n
    if calls:
        assert same_bits(a.tail_calls, b.tail_calls)
    else:
        assert a.tail_calls is None and b.tail_calls is None


def assert_rows(res, rows, calls):
    for n in SUMS:
        assert getattr(res, n).cpu().numpy().view(np.uint64).tolist() == [r[n] for r in rows], n
    assert [HREF.bits(s) for s in res.score.cpu().tolist()] == [HREF.bits(r["score"]) for r in rows]
    assert res.strag.cpu().tolist() == [int(r["strag"]) for r in rows]
    if calls:
        assert res.tail_calls.cpu().numpy().view(np.uint32).tolist() == [r["calls"] for r in rows]


def reference_rows(c, counts, h):
    ls = lambda a: np.ascontiguousarray(a).astype(np.uint32).tolist()  # noqa: E731
    return HREF.history_scores(
        ls(counts), ls(h), c.pm, BOTH, score_thr=THR,
        hist_index=None if c.hist_index is None else c.hist_index.tolist(),
        col_valid=None if c.col_valid is None else c.col_valid.tolist(),
        skip_rows=None if c.skip_rows is None else c.skip_rows.tolist())


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_equals_the_dense_chain_the_twin_and_the_definition(c):
    for iv, (counts, h, twin) in zip(c.intervals, C.walk(c.name)):
        I = Interval(c, iv)
        d_counts = I.counts()
        assert np.array_equal(d_counts.cpu().numpy(), counts)  # the chain's counts are the twin's
        rows, new = reference_rows(c, counts, h)
        assert twin.hist.tolist() == new
        for mode in MODES:
            for calls in (False, True):
                h_new, whole = guarded(h)
                h_dense = dev(h)
                got, out, _ = I.new(h_new, mode, calls)
                want, _ = I.dense(d_counts, h_dense, mode, calls)
                assert guard_ok(whole)
                assert torch.equal(h_new, h_dense), (mode, calls)  # the whole tensor, sentinels included
                assert np.array_equal(h_new.cpu().numpy().view(np.uint32), twin.hist if mode & HREF.UPDATE else h)
                if mode & HREF.SCORE:
                    assert_same_outputs(got, want, calls)
                    assert_rows(got, rows, calls)
                    assert got.score.cpu().numpy().tobytes() == twin.score.tobytes()
                else:
                    assert untouched(out) and got.tail_calls is None


@pytest.mark.parametrize("name", ["lengths_unaligned", "hist_index_permuted", "R70_K33"])
def test_skip_rows_from_the_previous_call_on_the_device(name):
    """absorb="healthy" on the device: a SCORE call, then an UPDATE call whose skip_rows is the
    strag the first wrote; the threshold is put between the rows' scores so that some are flagged."""
    c = C.case(name)
    iv, (counts, h, twin) = c.intervals[-1], C.walk(name)[-1]
    I = Interval(c, iv)
    d_hist, whole = guarded(h)
    res, out, _ = I.new(d_hist, HREF.SCORE, False, skip=None)
    score = res.score.cpu().numpy()
    mid = float(np.nanmedian(score))
    out.strag.copy_((res.score < mid).to(torch.uint8))
    flagged = out.strag.cpu().numpy().astype(bool)
    assert flagged.any() and not flagged.all()
    I.new(d_hist, HREF.UPDATE, False, skip=out.strag, out=out)
    d_dense = dev(h)
    I.dense(I.counts(), d_dense, HREF.UPDATE, False, skip=out.strag)
    assert torch.equal(d_hist, d_dense) and guard_ok(whole)
    got = d_hist.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[flagged], h[flagged]) and not np.array_equal(got[~flagged], h[~flagged])


def test_one_history_continued_by_both_entries():
    """Dense, new, dense over the three intervals equals the dense entry alone."""
    c = C.case("lengths_unaligned")
    a, b = dev(c.hist0), dev(c.hist0)
    for i, iv in enumerate(c.intervals):
        I = Interval(c, iv)
        counts = I.counts()
        want, _ = I.dense(counts, a, BOTH, True)
        got = I.new(b, BOTH, True)[0] if i % 2 else I.dense(counts, b, BOTH, True)[0]
        assert_same_outputs(got, want, True)
        assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), C.walk(c.name)[-1][2].hist)


def test_two_identical_calls_give_identical_bits():
    c = C.case("R70_K33")
    iv, (_, h, _) = c.intervals[-1], C.walk(c.name)[-1]
    I = Interval(c, iv)
    ha, hb = dev(h), dev(h)
    a, _, _ = I.new(ha, BOTH, True)
    b, _, _ = I.new(hb, BOTH, True)
    assert_same_outputs(a, b, True)
    assert torch.equal(ha, hb)


@pytest.mark.parametrize("mode", [HREF.SCORE, BOTH])
def test_graph_capture_and_replay(mode):
    c = C.case("R70_K33")
    iv, (counts, h, twin) = c.intervals[-1], C.walk(c.name)[-1]
    I = Interval(c, iv)
    d_hist = dev(h)
    out = sentinel_out(c.R)
    calls = torch.full((c.R, c.K), SENT, dtype=torch.int32, device=DEV)

    def launch():
        return ops.segment_history_scores_ragged(
            I.keys, I.off, I.lens, c.K, I.max_len, d_hist, permille=c.pm, score=True,
            update=bool(mode & HREF.UPDATE), cap=iv.cap, aligned16=iv.aligned16, score_thr=THR,
            tail_calls=calls, out=out, **I.kw)

    launch()  # the kernels are loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = launch()
    rows, new = reference_rows(c, counts, h)
    for _ in range(2):
        d_hist.copy_(dev(h))  # the history is restored between replays
        for t in (out.tail_ns, out.total_ns, out.base_tail_ns, out.base_total_ns, calls):
            t.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        assert_rows(res, rows, True)
        assert np.array_equal(d_hist.cpu().numpy().view(np.uint32), twin.hist if mode & HREF.UPDATE else h)
