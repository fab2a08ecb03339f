"""GPU: MatrixReporter.individual_tail_scores over ``histograms()`` of two small synthetic matrices
(R = 8, K = 5, 256 samples pushed); in the second one row's every 8th sample is doubled.  Each of
the three ``absorb`` modes equals the host twin ``histograms.history_scores`` applied the same way:
integers equal, f64 bit patterns equal."""
import numpy as np
import pytest
import torch

import _tail_ref as REF
import oracle as O
from nvidia_resiliency_ext.straggler import batch, histograms

pytestmark = pytest.mark.gpu

DEV = "cuda"
R, K, S, SLOW, EVERY, PM, THR = 8, 5, 256, 3, 8, 950, 0.9


def matrices():
    a = O.gen_matrix(R, K, S, straggler=np.zeros(R, np.uint8)).reshape(R, K, S).astype(np.uint64)
    b = a.copy()
    b[SLOW, :, ::EVERY] *= 2
    return a.astype(np.uint32), b.astype(np.uint32)


def twin_step(c, hist, absorb):
    """One interval of the reporter's policy on the host twin; returns (scores, new history)."""
    if absorb == "always":
        s = histograms.history_scores(c, hist, PM, score_thr=THR)
        return s, s.hist
    s = histograms.history_scores(c, hist, PM, update=False, score_thr=THR)
    if absorb == "never":
        return s, hist
    return s, histograms.history_scores(c, hist, PM, score=False, skip_rows=s.stragglers).hist


def assert_equal(got, want):
    for name in ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns"):
        assert getattr(got, name).tolist() == getattr(want, name).tolist(), name
    assert [REF.bits(s) for s in got.score] == [REF.bits(s) for s in want.score]
    assert [REF.bits(s) for s in got.history_share] == [REF.bits(s) for s in want.history_share]
    assert got.stragglers.tolist() == want.stragglers.tolist()


@pytest.mark.parametrize("absorb", batch.ABSORB_MODES)
def test_absorb_modes_equal_the_twin(absorb):
    a, b = matrices()
    rep = batch.MatrixReporter(R, K, cap=8192, thr_ind=THR, device=DEV)
    hist = np.zeros((R, K, histograms.BINS), np.uint32)
    results = []
    for keys in (a, a, b, b):
        ns = torch.from_numpy(keys.view(np.int32)).to(DEV)
        h = rep.histograms(ns, S)
        got = rep.individual_tail_scores(h, permille=PM, absorb=absorb, tail_calls=True)
        want, hist = twin_step(h.cpu().numpy(), hist, absorb)
        assert_equal(got, want)
        assert got.tail_calls.is_cuda
        assert got.tail_calls.cpu().numpy().view(np.uint32).tolist() == want.tail_calls.tolist()
        assert np.array_equal(rep._htail["hist"].cpu().numpy().view(np.uint32), hist)
        results.append(got)
    first, second, third, fourth = results
    assert all(s != s for s in first.score) and not first.stragglers.any()  # no history yet
    if absorb == "never":  # nothing was ever absorbed
        assert all(s != s for r in results for s in r.score)
        return
    assert all(abs(s - 1.0) < 0.05 for s in second.score) and not second.stragglers.any()
    assert np.nonzero(third.stragglers)[0].tolist() == [SLOW] and third.score[SLOW] < 0.85
    # a flagged interval is kept out of the history ("healthy"): the row scores the same again;
    # absorbed ("always"), the slow samples dilute the history and the score drifts back up
    if absorb == "healthy":
        assert REF.bits(fourth.score[SLOW]) == REF.bits(third.score[SLOW])
    else:
        assert fourth.score[SLOW] > third.score[SLOW]


def test_reset_and_bad_requests():
    a, _ = matrices()
    rep = batch.MatrixReporter(R, K, cap=8192, device=DEV)
    h = rep.histograms(torch.from_numpy(a.view(np.int32)).to(DEV), S)
    rep.reset_tail_history()  # nothing allocated yet: a no-op
    assert all(s != s for s in rep.individual_tail_scores(h).score)
    again = rep.individual_tail_scores(h, threshold=2.0, absorb="never")
    assert again.score.tolist() == [1.0] * R and again.stragglers.all() and again.tail_calls is None
    rep.reset_tail_history()
    assert all(s != s for s in rep.individual_tail_scores(h).score)  # NaN again
    with pytest.raises(ValueError, match="permille"):
        rep.individual_tail_scores(h, permille=1001)
    with pytest.raises(ValueError, match="absorb"):
        rep.individual_tail_scores(h, absorb="sometimes")
    with pytest.raises(ValueError, match="shape"):
        rep.individual_tail_scores(h[:1])


def test_kernel_shards_are_not_supported():
    # (the constructor wants a process group for exchange=True; the refusal reads the attribute)
    rep = batch.MatrixReporter(2, 3, device=DEV)
    rep.exchange = True
    h = torch.zeros((2, 3, histograms.BINS), dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError, match="exchange=True"):
        rep.individual_tail_scores(h)
    assert rep._htail is None  # refused before anything was allocated
