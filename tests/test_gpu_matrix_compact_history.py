"""GPU: MatrixReporter.individual_tail_scores_records(history="compact") -- the individual tail
scores of record streams against a compact history of 64 B per (rank, kernel) -- over three
intervals of small synthetic streams, rank 5 slow on every 8th call of the hottest kernel from the
second interval on: scores and flags equal ``history="dense"`` on a second reporter bit for bit
(nothing folds there), the compact history equals the host twin's and expands to the dense one;
attribution is refused, reset clears both histories, and the dense path is left as it was."""
import numpy as np
import pytest
import torch

from nvidia_resiliency_ext.straggler import batch, histograms, synth

pytestmark = pytest.mark.gpu

R, K, CAP, SLOW, PM, THR = 8, 64, 32, 5, 950, 0.95
FIELDS = ("score", "tail_ns", "total_ns", "history_share", "stragglers", "base_tail_ns", "base_total_ns")


@pytest.fixture(scope="module")
def intervals():
    counts = synth.zipf_counts(K, top=256)
    slot, occ = synth.zipf_order(counts)
    t32 = lambda a: torch.from_numpy(a.view(np.int32)).cuda()  # noqa: E731
    none = torch.zeros(R, dtype=torch.uint8, device="cuda")  # no uniformly slow rank
    N = slot.size
    rec_off = torch.arange(R + 1, dtype=torch.int64, device="cuda") * N
    out = []
    for i in range(3):
        # the same streams every interval: a healthy rank's interval is its history
        recs = synth.synth_records(R, t32(slot), t32(occ), K, int(counts.max()), straggler=none)
        if i >= 1:  # the degradation
            host = recs.cpu().numpy().view(np.uint32).copy()
            mine = host[SLOW * N:(SLOW + 1) * N]
            hot = np.flatnonzero(mine[:, 0] == 0)
            mine[hot[7::8], 1] *= 16
            recs = torch.from_numpy(host.view(np.int32)).cuda()
        out.append((recs, rec_off))
    return out


def _same(a, b, calls=False):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f
    if calls:
        assert torch.equal(a.tail_calls, b.tail_calls)
    assert a.attribution is None and b.attribution is None


def _twin(rep, chist, absorb):
    """The host twin on the buckets the reporter's last record-stream call laid out."""
    seg_off, seg_len, out_ns, _ = rep._rtail["bucket"]
    args = (out_ns.cpu().numpy().view(np.uint32), seg_off.cpu().numpy(), seg_len.cpu().numpy(), K,
            chist, PM, CAP)
    if absorb != "healthy":
        return histograms.segment_compact_history_scores(*args, update=absorb == "always", score_thr=THR)
    s = histograms.segment_compact_history_scores(*args, update=False, score_thr=THR)
    u = histograms.segment_compact_history_scores(*args, score=False, skip_rows=s.stragglers)
    s.hist, s.folded = u.hist, u.folded
    return s


@pytest.mark.parametrize("absorb", batch.ABSORB_MODES)
def test_equals_the_dense_history_and_the_twin(intervals, absorb):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    dense = batch.MatrixReporter(R, K, cap=CAP)
    assert rep.compact_tail_history() is None
    chist = np.zeros((R, K, histograms.CHIST_BYTES), np.uint8)
    for i, (recs, rec_off) in enumerate(intervals):
        got = rep.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR,
                                                 absorb=absorb, tail_calls=True, history="compact")
        want = dense.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR,
                                                    absorb=absorb, tail_calls=True)
        _same(got, want, calls=True)
        assert want.folded is None and got.folded.dtype == np.uint64 and not got.folded.any()
        twin = _twin(rep, chist, absorb)
        assert got.score.tobytes() == twin.score.tobytes()
        assert got.stragglers.tolist() == twin.stragglers.tolist()
        chist = twin.hist
        mine = rep.compact_tail_history()
        assert mine.dtype == torch.uint8 and tuple(mine.shape) == (R, K, 64)
        assert np.array_equal(mine.cpu().numpy(), chist)
        assert np.array_equal(histograms.compact_to_dense(chist),
                              dense._htail["hist"].cpu().numpy().view(np.uint32))
        assert rep._htail is None  # the dense history is not even allocated
        if i == 0 or absorb == "never":
            assert np.isnan(got.score).all() and not got.stragglers.any()
    if absorb != "never":
        print(absorb, "scores", got.score)
        assert got.stragglers.tolist() == [r == SLOW for r in range(R)]
    else:
        assert not chist.any()


def test_attribution_is_refused_and_arguments_are_checked(intervals):
    recs, rec_off = intervals[0]
    rep = batch.MatrixReporter(R, K, cap=CAP)
    with pytest.raises(NotImplementedError, match="compact"):
        rep.individual_tail_scores_records(recs, rec_off, permille=PM, attribute=4, history="compact")
    with pytest.raises(ValueError, match="history"):
        rep.individual_tail_scores_records(recs, rec_off, permille=PM, history="sparse")
    assert rep.compact_tail_history() is None  # refused before anything is allocated


def test_reset_tail_history_clears_the_compact_history(intervals):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    for recs, rec_off in intervals[:2]:
        res = rep.individual_tail_scores_records(recs, rec_off, permille=PM, absorb="always",
                                                 history="compact")
    assert not np.isnan(res.score).any() and rep.compact_tail_history().any()
    rep.reset_tail_history()
    assert not rep.compact_tail_history().any()
    res = rep.individual_tail_scores_records(*intervals[2], permille=PM, absorb="always",
                                             history="compact")
    assert np.isnan(res.score).all() and not res.stragglers.any()


def test_the_dense_path_is_unchanged_by_compact_calls(intervals):
    plain = batch.MatrixReporter(R, K, cap=CAP)
    rep = batch.MatrixReporter(R, K, cap=CAP)
    for recs, rec_off in intervals:
        want = plain.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR)
        rep.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR, history="compact")
        got = rep.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR)
        _same(got, want)
        assert got.folded is None
        assert torch.equal(rep._htail["hist"], plain._htail["hist"])
