"""GPU: MatrixReporter.individual_tail_scores(history="compact") -- the individual tail scores of
[R, K, 240] counts against the compact history -- and MatrixReporter.convert_tail_history, over
four intervals of small synthetic streams (rank 2 slow on every 8th call of the hottest kernel
from the second interval on) and the histograms of their retained windows: the results and the
history equal the host twin's for each ``absorb``; counts and record streams continue ONE compact
history; ``half_life`` ages it; a reporter converted in mid-run goes on bit for bit as the dense
one does, and back; every refusal comes before anything is allocated."""
import numpy as np
import pytest
import torch

from nvidia_resiliency_ext.straggler import batch, histograms, synth

pytestmark = pytest.mark.gpu

R, K, CAP, SLOW, PM, THR = 4, 50, 32, 2, 950, 0.95
FIELDS = ("score", "tail_ns", "total_ns", "history_share", "stragglers", "base_tail_ns", "base_total_ns")


@pytest.fixture(scope="module")
def intervals():
    """Per interval (recs, rec_off, counts on the device, counts on the host): the counts are the
    histograms of the windows the record-stream methods retain."""
    zc = synth.zipf_counts(K, top=256)
    slot, occ = synth.zipf_order(zc)
    t32 = lambda a: torch.from_numpy(a.view(np.int32)).cuda()  # noqa: E731
    none = torch.zeros(R, dtype=torch.uint8, device="cuda")  # no uniformly slow rank
    N = slot.size
    rec_off = torch.arange(R + 1, dtype=torch.int64, device="cuda") * N
    helper = batch.MatrixReporter(R, K, cap=CAP)
    out = []
    for i in range(4):
        # the same streams every interval: a healthy rank's interval is its history
        recs = synth.synth_records(R, t32(slot), t32(occ), K, int(zc.max()), straggler=none)
        if i >= 1:  # the degradation
            host = recs.cpu().numpy().view(np.uint32).copy()
            mine = host[SLOW * N:(SLOW + 1) * N]
            hot = np.flatnonzero(mine[:, 0] == 0)
            mine[hot[7::8], 1] *= 16
            recs = torch.from_numpy(host.view(np.int32)).cuda()
        helper.individual_tail_scores_records(recs, rec_off, permille=PM, absorb="never")
        seg_off, seg_len, out_ns, _ = helper._rtail["bucket"]
        counts = histograms.segment_counts(out_ns.cpu().numpy().view(np.uint32), seg_off.cpu().numpy(),
                                           seg_len.cpu().numpy(), K, CAP).astype(np.uint32)
        out.append((recs, rec_off, torch.from_numpy(counts.view(np.int32)).cuda(), counts))
    return out


def _same(a, b, calls=False):
    for f in FIELDS + ("folded",):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f
    if calls:
        assert torch.equal(a.tail_calls, b.tail_calls)
    assert a.attribution is None and b.attribution is None


def _twin(counts, chist, absorb):
    if absorb != "healthy":
        return histograms.compact_history_scores(counts, chist, PM, update=absorb == "always", score_thr=THR)
    s = histograms.compact_history_scores(counts, chist, PM, update=False, score_thr=THR)
    u = histograms.compact_history_scores(counts, chist, PM, score=False, skip_rows=s.stragglers)
    s.hist, s.folded = u.hist, u.folded
    return s


def _assert_twin(got, twin):
    assert got.score.tobytes() == twin.score.tobytes()
    assert got.stragglers.tolist() == twin.stragglers.tolist()
    for f in ("tail_ns", "total_ns", "base_tail_ns", "base_total_ns"):
        assert np.array_equal(getattr(got, f), getattr(twin, f)), f
    assert got.history_share.tobytes() == twin.history_share.tobytes()
    want = twin.folded if twin.folded is not None else np.zeros(R, np.uint64)
    assert got.folded.dtype == np.uint64 and np.array_equal(got.folded, want)


@pytest.mark.parametrize("absorb", batch.ABSORB_MODES)
def test_four_intervals_equal_the_twin(intervals, absorb):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    chist = np.zeros((R, K, histograms.CHIST_BYTES), np.uint8)
    for i, (_, _, d_counts, counts) in enumerate(intervals):
        got = rep.individual_tail_scores(d_counts, permille=PM, threshold=THR, absorb=absorb,
                                         tail_calls=True, history="compact")
        twin = _twin(counts, chist, absorb)
        _assert_twin(got, twin)
        assert np.array_equal(got.tail_calls.cpu().numpy().view(np.uint32), twin.tail_calls)
        chist = twin.hist
        assert np.array_equal(rep.compact_tail_history().cpu().numpy(), chist)
        assert rep._htail is None and rep._rtail is None  # neither the dense history nor the buckets
        if i == 0 or absorb == "never":
            assert np.isnan(got.score).all() and not got.stragglers.any()
        elif i == 1 or absorb == "healthy":
            # against a healthy history; under "always" the later histories have learnt the slow calls
            assert got.stragglers.tolist() == [r == SLOW for r in range(R)]
    assert chist.any() == (absorb != "never")


def test_counts_and_record_streams_continue_one_compact_history(intervals):
    mixed, by_counts, by_records = (batch.MatrixReporter(R, K, cap=CAP) for _ in range(3))
    kw = dict(permille=PM, threshold=THR, history="compact")
    for i, (recs, rec_off, d_counts, _) in enumerate(intervals):
        a = by_counts.individual_tail_scores(d_counts, **kw)
        b = by_records.individual_tail_scores_records(recs, rec_off, **kw)
        m = (mixed.individual_tail_scores(d_counts, **kw) if i % 2 == 0 else
             mixed.individual_tail_scores_records(recs, rec_off, **kw))
        _same(a, b)
        _same(a, m)
        assert torch.equal(mixed.compact_tail_history(), by_counts.compact_tail_history())
        assert torch.equal(mixed.compact_tail_history(), by_records.compact_tail_history())
    assert mixed._absorbed == by_counts._absorbed == {"dense": 0, "compact": 4}
    # the counts call leaves the buckets of the last record-stream call to compact_tail_attribution
    mixed.individual_tail_scores(intervals[0][2], absorb="never", **kw)
    want = by_records.compact_tail_attribution(top=4)
    got = mixed.compact_tail_attribution(top=4)
    assert got.kernel.tobytes() == want.kernel.tobytes() and got.loss_ns.tobytes() == want.loss_ns.tobytes()


def test_half_life_ages_the_history_at_the_third_absorbing_call(intervals):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    chist = np.zeros((R, K, histograms.CHIST_BYTES), np.uint8)
    for i, (_, _, d_counts, counts) in enumerate(intervals[:3]):
        got = rep.individual_tail_scores(d_counts, permille=PM, threshold=THR, absorb="always",
                                         history="compact", half_life=2)
        if i == 2:
            aged = histograms.compact_age(chist, 1)[0]
            assert not np.array_equal(aged, chist)
            chist = aged
        twin = _twin(counts, chist, "always")
        _assert_twin(got, twin)
        chist = twin.hist
        assert np.array_equal(rep.compact_tail_history().cpu().numpy(), chist)
    assert rep._absorbed["compact"] == 1


def test_convert_in_mid_run_goes_on_as_the_dense_reporter_does_and_back(intervals):
    dense, rep = batch.MatrixReporter(R, K, cap=CAP), batch.MatrixReporter(R, K, cap=CAP)
    kw = dict(permille=PM, threshold=THR, tail_calls=True)
    for _, _, d_counts, _ in intervals[:2]:
        want = dense.individual_tail_scores(d_counts, half_life=3, **kw)
        got = rep.individual_tail_scores(d_counts, half_life=3, **kw)
    folded = rep.convert_tail_history("compact")
    assert folded.dtype == np.uint64 and folded.tolist() == [0] * R
    assert rep._htail is None and rep._absorbed == {"dense": 0, "compact": 2}
    assert np.array_equal(histograms.compact_to_dense(rep.compact_tail_history().cpu().numpy()),
                          dense._htail["hist"].cpu().numpy().view(np.uint32))
    recs, rec_off, d_counts, _ = intervals[2]
    want = dense.individual_tail_scores(d_counts, half_life=3, **kw)
    got = rep.individual_tail_scores(d_counts, half_life=3, history="compact", **kw)
    for f in FIELDS:
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
    assert torch.equal(got.tail_calls, want.tail_calls) and not got.folded.any()
    assert got.stragglers.tolist() == [r == SLOW for r in range(R)]
    assert rep.convert_tail_history("dense") is None
    assert rep._ctail is None and rep.compact_tail_history() is None
    assert rep._absorbed == dense._absorbed == {"dense": 3, "compact": 0}
    assert torch.equal(rep._htail["hist"], dense._htail["hist"])
    # the fourth call finds three absorbing calls: both reporters age first
    want = dense.individual_tail_scores(intervals[3][2], half_life=3, **kw)
    got = rep.individual_tail_scores(intervals[3][2], half_life=3, **kw)
    for f in FIELDS:
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
    assert torch.equal(rep._htail["hist"], dense._htail["hist"])


def test_refusals_come_before_anything_is_allocated(intervals):
    d_counts = intervals[0][2]
    rep = batch.MatrixReporter(R, K, cap=CAP)
    with pytest.raises(NotImplementedError, match="attribute"):
        rep.individual_tail_scores(d_counts, permille=PM, attribute=4, history="compact")
    with pytest.raises(ValueError, match="history"):
        rep.individual_tail_scores(d_counts, permille=PM, history="sparse")
    for to in ("compact", "dense"):
        with pytest.raises(RuntimeError, match="history to convert"):
            rep.convert_tail_history(to)
    with pytest.raises(ValueError, match="to must be"):
        rep.convert_tail_history("sparse")
    rep.exchange = True
    with pytest.raises(NotImplementedError, match="exchange"):
        rep.individual_tail_scores(d_counts, permille=PM, history="compact")
    with pytest.raises(NotImplementedError, match="exchange"):
        rep.convert_tail_history("compact")
    assert rep._htail is None and rep._ctail is None and rep._rtail is None
