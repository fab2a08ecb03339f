"""GPU: MatrixReporter.individual_tail_scores_records(attribute=top) -- the kernels behind the
individual tail scores of record streams, without the [R, K, 240] counts -- equals
MatrixReporter.individual_tail_scores(attribute=top) fed the histograms of the same buckets on a
second reporter, for every ``absorb`` mode over three intervals: scores, attribution, the device
history and tail_calls.  ``attribute=0`` is byte for byte the call without the argument; the
slowed kernel of the slowed rank leads its row; bad requests and kernel shards are refused.  The
streams are those of ``test_gpu_matrix_history_tail_records``: rank 3 is 4x slower on every 4th
call of its costliest kernel in the last interval."""
import numpy as np
import pytest
import torch

from nvidia_resiliency_ext.straggler import batch, ops

pytestmark = pytest.mark.gpu

R, K, CAP, PM, THR, BINS, SLOW = 5, 40, 16, 950, 0.97, 240, 3
FIELDS = ("score", "tail_ns", "total_ns", "history_share", "stragglers", "base_tail_ns", "base_total_ns")
ATTR = ("kernel", "loss_ns", "tail_ns", "total_ns", "tail_calls", "threshold_bucket", "base_share")


def _interval(i):
    rng = np.random.default_rng(100 + i)
    recs, off = [], [0]
    for r in range(R):
        calls = rng.choice([0, 0, 1, 3, CAP, CAP + 1, 40], K)
        calls[K - 1] = 40
        calls[(r + i) % K] = 0
        slot = rng.permutation(np.repeat(np.arange(K), calls))
        ns = (2_000 * (1 + slot) * (1.0 + 0.002 * rng.standard_normal(slot.size))).astype(np.int64)
        if i == 2 and r == SLOW:
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
    counts = torch.zeros((R * K, BINS), dtype=torch.int32, device="cuda")
    ops.segment_histogram_ragged(out_ns, seg_off, seg_len, CAP, aligned16=True, out=counts)
    return counts.view(R, K, BINS)


def _bits(a):
    """Every NaN one pattern, everything else its bytes."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return np.where(np.isnan(a), np.uint64(0x7FF8 << 48), a.view(np.uint64))
    return a


def _same_scores(a, b, calls):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f
    if calls:
        assert torch.equal(a.tail_calls, b.tail_calls)
    else:
        assert a.tail_calls is None and b.tail_calls is None


def _same_attribution(a, b, top):
    for f in ATTR:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape == (R, top) and x.dtype == y.dtype, f
        assert np.array_equal(_bits(x), _bits(y)), f
    x, y = a.loss_all.cpu().numpy(), b.loss_all.cpu().numpy()
    assert x.shape == (R, K) and np.array_equal(_bits(x), _bits(y))


@pytest.mark.parametrize("absorb", batch.ABSORB_MODES)
@pytest.mark.parametrize("top,calls", [(4, True), (16, False)])
def test_equals_individual_tail_scores_on_the_buckets_histograms(intervals, absorb, top, calls):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    dense = batch.MatrixReporter(R, K, cap=CAP)
    for i, (recs, rec_off) in enumerate(intervals):
        got = rep.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR,
                                                 absorb=absorb, tail_calls=calls, attribute=top)
        want = dense.individual_tail_scores(_bucket_counts(rep), permille=PM, threshold=THR,
                                            absorb=absorb, tail_calls=calls, attribute=top)
        _same_scores(got, want, calls)
        _same_attribution(got.attribution, want.attribution, top)
        assert torch.equal(rep._htail["hist"], dense._htail["hist"])
        if i == 0 or absorb == "never":  # no history: nothing to attribute
            assert (got.attribution.kernel == -1).all()
    if absorb != "never":
        print(absorb, "attribution of the slowed rank", got.attribution.kernel[SLOW], got.attribution.loss_ns[SLOW])
        assert got.stragglers.tolist() == [r == SLOW for r in range(R)]
        # the planted slow kernel of the slowed rank leads its row
        assert got.attribution.kernel[SLOW][0] == K - 1 and got.attribution.loss_ns[SLOW][0] > 0
    else:
        assert not rep._htail["hist"].any()


@pytest.mark.parametrize("absorb", batch.ABSORB_MODES)
def test_attribute_zero_is_the_call_without_the_argument(intervals, absorb):
    a = batch.MatrixReporter(R, K, cap=CAP)
    b = batch.MatrixReporter(R, K, cap=CAP)
    for recs, rec_off in intervals:
        x = a.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR, absorb=absorb,
                                             tail_calls=True)
        y = b.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR, absorb=absorb,
                                             tail_calls=True, attribute=0)
        _same_scores(x, y, True)
        assert x.attribution is None and y.attribution is None and "abuf" not in b._htail
        assert torch.equal(a._htail["hist"], b._htail["hist"])


def test_the_attribution_leaves_the_scores_and_the_history_what_they_are(intervals):
    """With and without attribute= the scores, flags and history agree in every mode, and
    attribute=0 afterwards is the bare call again."""
    for absorb in batch.ABSORB_MODES:
        bare = batch.MatrixReporter(R, K, cap=CAP)
        rep = batch.MatrixReporter(R, K, cap=CAP)
        for i, (recs, rec_off) in enumerate(intervals):
            x = bare.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR, absorb=absorb)
            y = rep.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR, absorb=absorb,
                                                   attribute=8 if i != 1 else 0)
            _same_scores(x, y, False)
            assert (y.attribution is None) == (i == 1)
            assert torch.equal(bare._htail["hist"], rep._htail["hist"])


def test_requests_are_checked(intervals):
    recs, rec_off = intervals[0]
    rep = batch.MatrixReporter(R, K, cap=CAP)
    for bad in (17, -1, True, 2.5):
        with pytest.raises(ValueError, match="top"):
            rep.individual_tail_scores_records(recs, rec_off, attribute=bad)
    assert rep._htail is None and rep._rtail is None  # checked before anything is allocated or launched


def test_exchange_is_not_supported(intervals):
    recs, rec_off = intervals[0]
    rep = batch.MatrixReporter(R, K, cap=CAP)
    rep.exchange = True  # as a reporter over kernel shards
    with pytest.raises(NotImplementedError):
        rep.individual_tail_scores_records(recs, rec_off, attribute=4)
