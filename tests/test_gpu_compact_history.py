"""GPU: nvrx_segment_history_scores_compact_ragged against the compact host twin
(``histograms.compact_history_scores``) over every case of ``_compact_history_cases`` -- the cases
of ``_segment_history_cases`` with their history converted, and the directed fold cases -- interval
by interval in SCORE, UPDATE, SCORE|UPDATE and SCORE|UPDATE with tail_calls: integers equal, f64
bit patterns equal (NaN as NaN), the whole history tensor equal, sentinel slots and a guard region
behind it included; no tolerance.  Where a case never folds, the history's dense expansion and
every output also equal what ``ops.segment_history_scores_ragged`` gives on the dense history on
the device."""
import numpy as np
import pytest
import torch

import _compact_history_cases as C
from nvidia_resiliency_ext.straggler import histograms, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -7
GUARD = 0x5E
SCORE, UPDATE = 1, 2
BOTH = SCORE | UPDATE
RUNS = ((SCORE, False), (UPDATE, False), (BOTH, False), (BOTH, True))
SUMS = ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns")
CASES = C.cases()


def dev(a, dt=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV)


def guarded_chist(ch):
    """A device copy of a compact history with 64 guard bytes behind it: (the view, the whole)."""
    whole = torch.full((ch.size + C.CB,), GUARD, dtype=torch.uint8, device=DEV)
    view = whole[:ch.size].view(ch.shape)
    view.copy_(torch.from_numpy(ch).to(DEV))
    return view, whole


def guard_ok(whole):
    return whole[-C.CB:].cpu().tolist() == [GUARD] * C.CB


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
                       col_valid=opt(c.col_valid, torch.uint8), skip_rows=opt(c.skip_rows, torch.uint8),
                       permille=c.pm, cap=iv.cap, aligned16=iv.aligned16, score_thr=C.THR)

    def compact(self, d_chist, mode, calls, out=None, folded=None):
        c = self.c
        out = sentinel_out(c.R) if out is None else out
        folded = torch.full((c.R,), SENT, dtype=torch.int64, device=DEV) if folded is None else folded
        tc = torch.full((c.R * c.K + 4,), SENT, dtype=torch.int32, device=DEV) if calls else None
        res, f = ops.segment_history_scores_compact_ragged(
            self.keys, self.off, self.lens, c.K, self.max_len, d_chist, score=bool(mode & SCORE),
            update=bool(mode & UPDATE), tail_calls=tc[:c.R * c.K].view(c.R, c.K) if calls else False,
            out=out, folded=folded, **self.kw)
        assert tc is None or tc[-4:].cpu().tolist() == [SENT] * 4
        assert (f is folded) if mode & UPDATE else (f is None)
        return res, out, folded

    def dense(self, d_hist, mode, calls):
        c = self.c
        return ops.segment_history_scores_ragged(
            self.keys, self.off, self.lens, c.K, self.max_len, d_hist, score=bool(mode & SCORE),
            update=bool(mode & UPDATE), tail_calls=bool(calls), out=sentinel_out(c.R), **self.kw)


def assert_twin(res, twin, calls):
    for n in SUMS:
        assert np.array_equal(getattr(res, n).cpu().numpy().view(np.uint64), getattr(twin, n)), n
    assert res.score.cpu().numpy().tobytes() == twin.score.tobytes()
    assert res.strag.cpu().numpy().astype(bool).tolist() == twin.stragglers.tolist()
    if calls:
        assert np.array_equal(res.tail_calls.cpu().numpy().view(np.uint32), twin.tail_calls)
    else:
        assert res.tail_calls is None


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def dense_start(c, chist):
    """The dense history (used slots expanded, the others zero) of a compact one, on the host."""
    used = C.used_slots(c)
    d = np.zeros(chist.shape[:2] + (C.BINS,), np.uint32)
    d[:, used] = histograms.compact_to_dense(chist[:, used])
    return d


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_equals_the_twin_and_where_nothing_folds_the_dense_entry(c):
    walk = C.walk(c.name)
    fold_free = not any(int(t.folded.sum()) for _, _, t in walk)
    used = C.used_slots(c)
    for iv, (_, h, twin) in zip(c.intervals, walk):
        I = Interval(c, iv)
        for mode, calls in RUNS:
            d_chist, whole = guarded_chist(h)
            res, out, folded = I.compact(d_chist, mode, calls)
            assert guard_ok(whole)
            # the whole tensor, sentinel slots included
            assert np.array_equal(d_chist.cpu().numpy(), twin.hist if mode & UPDATE else h), (mode, calls)
            if mode & UPDATE:
                assert np.array_equal(folded.cpu().numpy().view(np.uint64), twin.folded)
            else:
                assert folded.cpu().tolist() == [SENT] * c.R
            if mode & SCORE:
                assert_twin(res, twin, calls)
            else:
                assert untouched(out) and res.tail_calls is None
            if fold_free:  # the bit-exact oracle: the dense entry on the dense history
                d_hist = dev(dense_start(c, h))
                want = I.dense(d_hist, mode, calls)
                got = dense_start(c, d_chist.cpu().numpy())
                assert np.array_equal(got[:, used], d_hist.cpu().numpy().view(np.uint32)[:, used])
                if mode & SCORE:
                    for n in SUMS + ("score", "strag"):
                        assert same_bits(getattr(res, n), getattr(want, n)), n
                    if calls:
                        assert same_bits(res.tail_calls, want.tail_calls)


def test_enough_cases_fold_and_enough_do_not():
    folds = [c.name for c in CASES if any(int(t.folded.sum()) for _, _, t in C.walk(c.name))]
    assert len(folds) >= 5 and len(CASES) - len(folds) >= 12


@pytest.mark.parametrize("name", ["R70_K33", "fold_rule"])
def test_two_identical_calls_give_identical_bits(name):
    c = C.case(name)
    iv, (_, h, _) = c.intervals[-1], C.walk(name)[-1]
    I = Interval(c, iv)
    ha, hb = dev(h, np.uint8), dev(h, np.uint8)
    a, _, fa = I.compact(ha, BOTH, True)
    b, _, fb = I.compact(hb, BOTH, True)
    for n in SUMS + ("score", "strag", "tail_calls"):
        assert same_bits(getattr(a, n), getattr(b, n)), n
    assert torch.equal(ha, hb) and torch.equal(fa, fb)


@pytest.mark.parametrize("name", ["R70_K33", "fold_rule"])
def test_graph_capture_and_replay(name):
    c = C.case(name)
    iv, (_, h, twin) = c.intervals[-1], C.walk(name)[-1]
    I = Interval(c, iv)
    d_chist = dev(h, np.uint8)
    out = sentinel_out(c.R)
    folded = torch.full((c.R,), SENT, dtype=torch.int64, device=DEV)
    calls = torch.full((c.R, c.K), SENT, dtype=torch.int32, device=DEV)

    def launch():
        return ops.segment_history_scores_compact_ragged(
            I.keys, I.off, I.lens, c.K, I.max_len, d_chist, tail_calls=calls, out=out,
            folded=folded, **I.kw)[0]

    launch()  # the kernels are loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = launch()
    for _ in range(2):
        d_chist.copy_(dev(h, np.uint8))  # the history is restored between replays
        for t in (out.tail_ns, out.total_ns, out.base_tail_ns, out.base_total_ns, calls, folded):
            t.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        assert_twin(res, twin, True)
        assert np.array_equal(folded.cpu().numpy().view(np.uint64), twin.folded)
        assert np.array_equal(d_chist.cpu().numpy(), twin.hist)


def test_wrapper_rejects_a_history_of_the_wrong_shape_or_type():
    c = C.case("fold_rule")
    I = Interval(c, c.intervals[0])
    for bad in (torch.zeros((c.R, c.K, 60), dtype=torch.uint8, device=DEV),
                torch.zeros((c.R, c.K, 16), dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError, match="chist"):
            ops.segment_history_scores_compact_ragged(I.keys, I.off, I.lens, c.K, I.max_len, bad, **I.kw)
