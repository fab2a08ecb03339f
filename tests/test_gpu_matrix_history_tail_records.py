"""GPU: MatrixReporter.individual_tail_scores_records -- the individual tail scores of record
streams without the [R, K, 240] counts -- equals, every field and the device history included,
MatrixReporter.individual_tail_scores fed the histograms of the same buckets on a second reporter,
over three intervals of small streams with kernels missing per rank and rings above cap; the two
methods continue one history; reset, queueing behind a report in flight, the refusal of kernel
shards; and tail_scores_records is left as it was."""
import numpy as np
import pytest
import torch

from nvidia_resiliency_ext.straggler import batch, ops

pytestmark = pytest.mark.gpu

R, K, CAP, PM, THR, BINS = 5, 40, 16, 950, 0.97, 240
FIELDS = ("score", "tail_ns", "total_ns", "history_share", "stragglers", "base_tail_ns", "base_total_ns")


def _interval(i):
    """Interleaved records of R ranks: per rank some kernels missing, some rings above CAP; rank 3
    is 4x slower on every 4th call of its costliest kernel in the last interval (0.2 % jitter: with
    the host twin the healthy ranks score 1.0, rank 3 0.909)."""
    rng = np.random.default_rng(100 + i)
    recs, off = [], [0]
    for r in range(R):
        calls = rng.choice([0, 0, 1, 3, CAP, CAP + 1, 40], K)
        calls[K - 1] = 40
        calls[(r + i) % K] = 0
        slot = rng.permutation(np.repeat(np.arange(K), calls))
        ns = (2_000 * (1 + slot) * (1.0 + 0.002 * rng.standard_normal(slot.size))).astype(np.int64)
        if i == 2 and r == 3:
            hot = np.flatnonzero(slot == K - 1)
            ns[hot[3::4]] *= 4
        recs.append(np.stack([slot, ns], 1))
        off.append(off[-1] + slot.size)
    return (torch.from_numpy(np.concatenate(recs).astype(np.int32)).cuda(),
            torch.tensor(off, dtype=torch.int64, device="cuda"))


@pytest.fixture(scope="module")
def intervals():
    return [_interval(i) for i in range(3)]


def _bucket_counts(rep):
    """The histograms of the buckets the reporter's last record-stream tail call laid out."""
    seg_off, seg_len, out_ns, _ = rep._rtail["bucket"]
    assert int(seg_len.min()) == 0 and int(seg_len.max()) == CAP  # kernels missing, rings trimmed
    counts = torch.zeros((R * K, BINS), dtype=torch.int32, device="cuda")
    ops.segment_histogram_ragged(out_ns, seg_off, seg_len, CAP, aligned16=True, out=counts)
    return counts.view(R, K, BINS)


def _same(a, b, calls=True):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f
    if calls:
        assert torch.equal(a.tail_calls, b.tail_calls)
    else:
        assert a.tail_calls is None and b.tail_calls is None
    assert a.attribution is None and b.attribution is None


@pytest.mark.parametrize("absorb", batch.ABSORB_MODES)
@pytest.mark.parametrize("calls", (False, True))
def test_equals_individual_tail_scores_on_the_buckets_histograms(intervals, absorb, calls):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    dense = batch.MatrixReporter(R, K, cap=CAP)
    for i, (recs, rec_off) in enumerate(intervals):
        got = rep.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR,
                                                 absorb=absorb, tail_calls=calls)
        want = dense.individual_tail_scores(_bucket_counts(rep), permille=PM, threshold=THR,
                                            absorb=absorb, tail_calls=calls)
        _same(got, want, calls)
        assert torch.equal(rep._htail["hist"], dense._htail["hist"])
        if i == 0 or absorb == "never":
            assert np.isnan(got.score).all() and not got.stragglers.any()
    if absorb != "never":
        print(absorb, "scores", got.score)
        assert got.stragglers.tolist() == [r == 3 for r in range(R)]
        # rank 1 did not run kernel 1 in the first interval: at most two intervals in its slot
        assert int(rep._htail["hist"][1, 1].sum()) <= 2 * CAP
    else:
        assert not rep._htail["hist"].any()


def test_both_methods_continue_one_history(intervals):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    dense = batch.MatrixReporter(R, K, cap=CAP)
    probe = batch.MatrixReporter(R, K, cap=CAP)  # lays the buckets out for the dense calls
    for i, (recs, rec_off) in enumerate(intervals):
        probe.individual_tail_scores_records(recs, rec_off, absorb="never")
        counts = _bucket_counts(probe)
        want = dense.individual_tail_scores(counts, permille=PM, threshold=THR, absorb="always")
        if i == 1:
            got = rep.individual_tail_scores(counts, permille=PM, threshold=THR, absorb="always")
        else:
            got = rep.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR,
                                                     absorb="always")
        _same(got, want, calls=False)
        assert torch.equal(rep._htail["hist"], dense._htail["hist"])
    assert not np.isnan(got.score).any()


def test_reset_tail_history(intervals):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    rep.reset_tail_history()  # nothing allocated yet
    for recs, rec_off in intervals[:2]:
        res = rep.individual_tail_scores_records(recs, rec_off, permille=PM, absorb="always")
    assert not np.isnan(res.score).any()
    rep.reset_tail_history()
    res = rep.individual_tail_scores_records(*intervals[2], permille=PM, absorb="always")
    assert np.isnan(res.score).all() and not res.stragglers.any()


def test_queues_behind_a_report_in_flight(intervals):
    recs, rec_off = intervals[0]
    plain = batch.MatrixReporter(R, K, cap=CAP)
    want_report = plain.report_records(recs, rec_off)
    want = plain.individual_tail_scores_records(recs, rec_off, permille=PM, absorb="always")
    rep = batch.MatrixReporter(R, K, cap=CAP)
    pipe = rep.pipelined_records(recs, rec_off)
    pipe.submit()
    got = rep.individual_tail_scores_records(recs, rec_off, permille=PM, absorb="always")
    res = pipe.collect()[0]
    _same(got, want, calls=False)
    assert torch.equal(rep._htail["hist"], plain._htail["hist"])
    for f in ("gpu_relative", "gpu_individual"):
        assert np.array_equal(getattr(res, f).view(np.uint64), getattr(want_report, f).view(np.uint64))
    assert res.err == want_report.err


def test_requests_are_checked(intervals):
    recs, rec_off = intervals[0]
    rep = batch.MatrixReporter(R, K, cap=CAP)
    with pytest.raises(ValueError, match="permille"):
        rep.individual_tail_scores_records(recs, rec_off, permille=1001)
    with pytest.raises(ValueError, match="rec_off"):
        rep.individual_tail_scores_records(recs, rec_off[:-1])
    with pytest.raises(ValueError, match="absorb"):
        rep.individual_tail_scores_records(recs, rec_off, absorb="sometimes")
    rep.exchange = True  # as a reporter over kernel shards
    with pytest.raises(NotImplementedError):
        rep.individual_tail_scores_records(recs, rec_off)


def test_tail_scores_records_gives_what_it_gave(intervals):
    recs, rec_off = intervals[2]
    rep = batch.MatrixReporter(R, K, cap=CAP)
    before = rep.tail_scores_records(recs, rec_off, permille=PM, threshold=THR, tail_calls=True)
    calls_before = before.tail_calls.clone()
    for r, o in intervals:
        rep.individual_tail_scores_records(r, o, permille=PM, tail_calls=True)
    after = rep.tail_scores_records(recs, rec_off, permille=PM, threshold=THR, tail_calls=True)
    fresh = batch.MatrixReporter(R, K, cap=CAP).tail_scores_records(recs, rec_off, permille=PM,
                                                                   threshold=THR, tail_calls=True)
    for res in (after, fresh):
        for f in ("score", "tail_ns", "total_ns", "stragglers", "threshold_bucket"):
            assert getattr(res, f).tobytes() == getattr(before, f).tobytes(), f
        assert np.float64(res.fleet_share).tobytes() == np.float64(before.fleet_share).tobytes()
        assert torch.equal(res.tail_calls, calls_before)
