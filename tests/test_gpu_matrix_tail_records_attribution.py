"""GPU: MatrixReporter.tail_scores_records(attribute=top) -- the kernels behind the tail scores of
record streams, without the [R, K, 240] counts -- equals MatrixReporter.tail_scores(attribute=top)
fed the dense counts of the same buckets and the host twin run over the bucketing contract
(``_records_model.retain``); it names the slowed kernel of the slow rank first, leaves the scores
what they are without it, and leaves a report's buffers alone.  The streams are those of
``test_gpu_matrix_tail_records``: rank 5 slow on every 8th call of the hottest kernel."""
import numpy as np
import pytest
import torch

import _records_model as model
from nvidia_resiliency_ext.straggler import batch, histograms, ops, synth

pytestmark = pytest.mark.gpu

R, K, CAP, SLOW, PM, THR = 8, 64, 32, 5, 950, 0.95
PAIRS = dict(kernel="idx", loss_ns="loss", tail_ns="tail_ns", total_ns="total_ns",
             tail_calls="tail_calls", threshold_bucket="thr_bucket", base_share="base_share")


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


def _bits(a):
    """Every NaN one pattern, everything else its bytes."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return np.where(np.isnan(a), np.uint64(0x7FF8 << 48), a.view(np.uint64))
    return a


def assert_attribution(att, want, top):
    """A BatchTailAttribution against a host TailAttribution / another BatchTailAttribution."""
    for mine, theirs in PAIRS.items():
        g = getattr(att, mine)
        w = getattr(want, theirs if hasattr(want, theirs) else mine)
        assert g.shape == w.shape == (R, top) and g.dtype == w.dtype, mine
        assert np.array_equal(_bits(g), _bits(w)), mine
    g = att.loss_all.cpu().numpy()
    w = want.loss_all.cpu().numpy() if isinstance(want.loss_all, torch.Tensor) else want.loss_all
    assert g.shape == (R, K) and np.array_equal(_bits(g), _bits(w))


def _same_scores(a: batch.BatchTailScores, b: batch.BatchTailScores):
    assert np.array_equal(a.score.view(np.uint64), b.score.view(np.uint64))
    assert np.array_equal(a.tail_ns, b.tail_ns) and np.array_equal(a.total_ns, b.total_ns)
    assert np.float64(a.fleet_share).view(np.uint64) == np.float64(b.fleet_share).view(np.uint64)
    assert np.array_equal(a.stragglers, b.stragglers)
    assert np.array_equal(a.threshold_bucket, b.threshold_bucket)
    assert torch.equal(a.tail_calls, b.tail_calls)


def _same_report(a: batch.BatchResult, b: batch.BatchResult):
    for f in ("gpu_relative", "gpu_individual"):
        assert np.array_equal(getattr(a, f).view(np.uint64), getattr(b, f).view(np.uint64))
    assert np.array_equal(a.stragglers_relative, b.stragglers_relative)
    assert np.array_equal(a.stragglers_individual, b.stragglers_individual) and a.err == b.err


def _twin(host, rec_off, top):
    kept = model.retain(host, rec_off.cpu().numpy(), K, CAP).kept
    lens = np.array([k.size for k in kept])
    off = np.cumsum(np.concatenate([[0], lens[:-1]]))
    return histograms.segment_tail_attribution(np.concatenate(kept), off, lens, K, PM, top)


def test_equals_the_dense_chain_and_the_twin_and_leaves_scores_and_report_alone(streams):
    recs, rec_off, host = streams
    plain = batch.MatrixReporter(R, K, cap=CAP)
    want = [plain.report_records(recs, rec_off) for _ in range(2)]

    rep = batch.MatrixReporter(R, K, cap=CAP)
    before = rep.report_records(recs, rec_off)
    bare = rep.tail_scores_records(recs, rec_off, permille=PM, threshold=THR, tail_calls=True)
    assert bare.attribution is None and "abuf" not in rep._rtail
    calls = bare.tail_calls.clone()
    got = rep.tail_scores_records(recs, rec_off, permille=PM, threshold=THR, tail_calls=True,
                                  attribute=4)
    after = rep.report_records(recs, rec_off)
    _same_report(before, want[0])
    _same_report(after, want[1])
    print("attribution of the slow rank", got.attribution.kernel[SLOW], got.attribution.loss_ns[SLOW])

    # scores, flags, thresholds and tail_calls: what they are without the attribution
    _same_scores(got, bare)
    assert torch.equal(got.tail_calls, calls)
    assert got.stragglers.tolist() == [r == SLOW for r in range(R)]

    # MatrixReporter.tail_scores(attribute=4) on the dense counts of the same buckets
    seg_off, seg_len, out_ns, _ = rep._rtail["bucket"]
    counts = torch.zeros((R * K, 240), dtype=torch.int32, device="cuda")
    ops.segment_histogram_ragged(out_ns, seg_off, seg_len, CAP, aligned16=True, out=counts)
    dense = batch.MatrixReporter(R, K, cap=CAP).tail_scores(counts.view(R, K, 240), permille=PM,
                                                           threshold=THR, tail_calls=True, attribute=4)
    _same_scores(got, dense)
    assert_attribution(got.attribution, dense.attribution, 4)

    # the host twin over the bucketing contract
    assert_attribution(got.attribution, _twin(host, rec_off, 4), 4)

    # the hottest kernel of the slow rank leads
    assert got.attribution.kernel[SLOW][0] == 0 and got.attribution.loss_ns[SLOW][0] > 0

    # a second call with another top reuses the buffers and agrees
    held = {k: rep._rtail[k].data_ptr() for k in ("abuf", "loss_all", "base")}
    again = rep.tail_scores_records(recs, rec_off, permille=PM, threshold=THR, tail_calls=True,
                                    attribute=16)
    assert held == {k: rep._rtail[k].data_ptr() for k in held}
    _same_scores(again, bare)
    assert_attribution(again.attribution, _twin(host, rec_off, 16), 16)
    assert np.array_equal(again.attribution.kernel[:, :4], got.attribution.kernel)

    # and attribute=0 afterwards is the bare call again
    last = rep.tail_scores_records(recs, rec_off, permille=PM, threshold=THR, tail_calls=True)
    assert last.attribution is None
    _same_scores(last, bare)


def test_requests_are_checked(streams):
    recs, rec_off, _ = streams
    rep = batch.MatrixReporter(R, K, cap=CAP)
    for bad in (17, -1, True, 2.5):
        with pytest.raises(ValueError, match="top"):
            rep.tail_scores_records(recs, rec_off, attribute=bad)
    assert rep._rtail is None  # checked before anything is allocated or launched


def test_exchange_is_not_supported(streams):
    recs, rec_off, _ = streams
    rep = batch.MatrixReporter(R, K, cap=CAP)
    rep.exchange = True  # as a reporter over kernel shards
    with pytest.raises(NotImplementedError):
        rep.tail_scores_records(recs, rec_off, attribute=4)
