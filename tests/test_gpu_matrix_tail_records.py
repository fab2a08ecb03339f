"""GPU: MatrixReporter.tail_scores_records -- the tail scores of record streams without the
[R, K, 240] counts -- equals, every field included, MatrixReporter.tail_scores fed the dense
counts of the same buckets, and the host twin run over the bucketing contract
(``_records_model.retain``); a rank slow on every 8th call of the hottest kernel is the only one
flagged; a report's buffers are not touched."""
import numpy as np
import pytest
import torch

import _records_model as model
import _tail_ref as ref
from nvidia_resiliency_ext.straggler import batch, histograms, ops, synth

pytestmark = pytest.mark.gpu

R, K, CAP, SLOW, PM, THR = 8, 64, 32, 5, 950, 0.95


@pytest.fixture(scope="module")
def streams():
    counts = synth.zipf_counts(K, top=256)
    assert (counts > CAP).sum() >= 3  # several hot slots overflow the ring
    slot, occ = synth.zipf_order(counts)
    t32 = lambda a: torch.from_numpy(a.view(np.int32)).cuda()  # noqa: E731
    none = torch.zeros(R, dtype=torch.uint8, device="cuda")  # no uniformly slow rank
    recs = synth.synth_records(R, t32(slot), t32(occ), K, int(counts.max()), straggler=none)
    N = slot.size
    host = recs.cpu().numpy().view(np.uint32).copy()
    mine = host[SLOW * N:(SLOW + 1) * N]
    hot = np.flatnonzero(mine[:, 0] == 0)
    mine[hot[7::8], 1] *= 16  # slow on every 8th call of the hottest kernel
    recs = torch.from_numpy(host.view(np.int32)).cuda()
    rec_off = torch.arange(R + 1, dtype=torch.int64, device="cuda") * N
    return recs, rec_off, host


def _same_report(a: batch.BatchResult, b: batch.BatchResult):
    for f in ("gpu_relative", "gpu_individual"):
        assert np.array_equal(getattr(a, f).view(np.uint64), getattr(b, f).view(np.uint64))
    assert np.array_equal(a.stragglers_relative, b.stragglers_relative)
    assert np.array_equal(a.stragglers_individual, b.stragglers_individual) and a.err == b.err


def test_equals_the_dense_chain_and_the_twin_and_leaves_the_report_alone(streams):
    recs, rec_off, host = streams
    plain = batch.MatrixReporter(R, K, cap=CAP)
    want = [plain.report_records(recs, rec_off) for _ in range(2)]

    rep = batch.MatrixReporter(R, K, cap=CAP)
    before = rep.report_records(recs, rec_off)
    got = rep.tail_scores_records(recs, rec_off, permille=PM, threshold=THR, tail_calls=True)
    after = rep.report_records(recs, rec_off)
    _same_report(before, want[0])
    _same_report(after, want[1])
    print("tail scores", got.score)

    # every bucket materialised: none reduced on chip and marked seg_len < 0
    seg_off, seg_len, out_ns, pushes = rep._rtail["bucket"]
    assert int(seg_len.min()) >= 0 and int(seg_len.max()) == CAP
    assert rep._rtail["bucket"] is not rep.own.bucket

    # MatrixReporter.tail_scores on the dense counts of the same buckets
    counts = torch.zeros((R * K, 240), dtype=torch.int32, device="cuda")
    ops.segment_histogram_ragged(out_ns, seg_off, seg_len, CAP, aligned16=True, out=counts)
    dense = batch.MatrixReporter(R, K, cap=CAP).tail_scores(counts.view(R, K, 240), permille=PM,
                                                           threshold=THR, tail_calls=True)
    assert np.array_equal(got.score.view(np.uint64), dense.score.view(np.uint64))
    assert np.array_equal(got.tail_ns, dense.tail_ns) and np.array_equal(got.total_ns, dense.total_ns)
    assert ref.bits(got.fleet_share) == ref.bits(dense.fleet_share)
    assert np.array_equal(got.stragglers, dense.stragglers)
    assert np.array_equal(got.threshold_bucket, dense.threshold_bucket)
    assert torch.equal(got.tail_calls, dense.tail_calls)
    assert got.attribution is None and dense.attribution is None

    # the host twin over the bucketing contract
    kept = model.retain(host, rec_off.cpu().numpy(), K, CAP).kept
    lens = np.array([k.size for k in kept])
    off = np.cumsum(np.concatenate([[0], lens[:-1]]))
    twin = histograms.segment_tail_scores(np.concatenate(kept), off, lens, K, PM)
    assert np.array_equal(got.score.view(np.uint64), twin.score.view(np.uint64))
    assert np.array_equal(got.tail_ns, twin.tail_ns) and np.array_equal(got.total_ns, twin.total_ns)
    assert ref.bits(got.fleet_share) == ref.bits(twin.fleet_share)
    assert np.array_equal(got.threshold_bucket, twin.threshold_bucket)
    assert np.array_equal(got.tail_calls.cpu().numpy().view(np.uint32), twin.tail_calls)
    assert np.array_equal(got.stragglers, twin.score < THR)

    # the injected rank is the only one flagged
    assert got.stragglers.tolist() == [r == SLOW for r in range(R)]

    # without tail_calls: the same scores, no calls
    bare = rep.tail_scores_records(recs, rec_off, permille=PM, threshold=THR)
    assert bare.tail_calls is None
    assert np.array_equal(bare.score.view(np.uint64), got.score.view(np.uint64))


def test_requests_are_checked(streams):
    recs, rec_off, _ = streams
    rep = batch.MatrixReporter(R, K, cap=CAP)
    with pytest.raises(ValueError, match="permille"):
        rep.tail_scores_records(recs, rec_off, permille=1001)
    with pytest.raises(ValueError, match="rec_off"):
        rep.tail_scores_records(recs, rec_off[:-1])


def test_exchange_is_not_supported(streams):
    recs, rec_off, _ = streams
    rep = batch.MatrixReporter(R, K, cap=CAP)
    rep.exchange = True  # as a reporter over kernel shards
    with pytest.raises(NotImplementedError):
        rep.tail_scores_records(recs, rec_off)
