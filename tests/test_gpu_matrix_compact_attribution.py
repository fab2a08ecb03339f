"""GPU: MatrixReporter.compact_tail_attribution -- the kernels behind the individual tail scores of
record streams against the compact history, on request -- on the shapes and streams of
test_gpu_matrix_compact_history.py (R 8, K 64, cap 32, rank 5 slow on every 8th call of the hottest
kernel from the second interval on), a compact and a dense reporter side by side: for the rows the
last call did not absorb the result equals the dense reporter's ``attribute=`` field for field;
after an absorbing call it equals the host twin on the updated history; the history is left
bit-identical; the method refuses to run without a compact call to explain, and the dense path is
what it was."""
import numpy as np
import pytest
import torch

from nvidia_resiliency_ext.straggler import batch, histograms, synth

pytestmark = pytest.mark.gpu

R, K, CAP, SLOW, PM, THR = 8, 64, 32, 5, 950, 0.95
FIELDS = ("kernel", "loss_ns", "tail_ns", "total_ns", "tail_calls", "threshold_bucket", "base_share")
TWIN = ("idx", "loss", "tail_ns", "total_ns", "tail_calls", "thr_bucket", "base_share")


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


def _rows_equal(got, want, rows):
    assert isinstance(got, batch.BatchTailAttribution)
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, f
        assert a[rows].tobytes() == b[rows].tobytes(), f
    assert got.loss_all[rows].cpu().numpy().tobytes() == want.loss_all[rows].cpu().numpy().tobytes()


def _pair(intervals, first):
    """A compact and a dense reporter after one interval absorbed under ``first``."""
    rep, dense = batch.MatrixReporter(R, K, cap=CAP), batch.MatrixReporter(R, K, cap=CAP)
    kw = dict(permille=PM, threshold=THR, absorb=first)
    rep.individual_tail_scores_records(*intervals[0], history="compact", **kw)
    dense.individual_tail_scores_records(*intervals[0], **kw)
    return rep, dense


def test_flagged_row_equals_the_dense_attribute_under_healthy(intervals):
    rep, dense = _pair(intervals, "healthy")  # no history yet: nothing flagged, all absorbed
    kw = dict(permille=PM, threshold=THR, absorb="healthy")
    got = rep.individual_tail_scores_records(*intervals[1], history="compact", **kw)
    want = dense.individual_tail_scores_records(*intervals[1], attribute=4, **kw)
    assert got.stragglers.tolist() == want.stragglers.tolist() == [r == SLOW for r in range(R)]
    assert not got.folded.any()
    before = rep.compact_tail_history().clone()
    attr = rep.compact_tail_attribution(4)
    assert torch.equal(rep.compact_tail_history(), before)  # read only
    _rows_equal(attr, want.attribution, [SLOW])
    assert attr.kernel[SLOW, 0] == 0 and attr.loss_ns[SLOW, 0] > 0  # the hottest kernel, degraded
    # asked again, the same bytes
    _rows_equal(rep.compact_tail_attribution(4), attr, list(range(R)))


def test_every_row_equals_the_dense_attribute_under_never(intervals):
    rep, dense = _pair(intervals, "always")
    kw = dict(permille=PM, threshold=THR, absorb="never")
    rep.individual_tail_scores_records(*intervals[1], history="compact", **kw)
    want = dense.individual_tail_scores_records(*intervals[1], attribute=4, **kw)
    _rows_equal(rep.compact_tail_attribution(4), want.attribution, list(range(R)))


def test_equals_the_host_twin_on_the_updated_history(intervals):
    rep, _ = _pair(intervals, "always")
    rep.individual_tail_scores_records(*intervals[1], permille=PM, threshold=THR, absorb="always",
                                       history="compact")
    before = rep.compact_tail_history().clone()
    seg_off, seg_len, out_ns, _ = rep._rtail["bucket"]
    args = (out_ns.cpu().numpy().view(np.uint32), seg_off.cpu().numpy(), seg_len.cpu().numpy(), K,
            before.cpu().numpy())
    for top, pm in ((8, None), (3, 900)):
        got = rep.compact_tail_attribution(permille=pm) if top == 8 else rep.compact_tail_attribution(top, permille=pm)
        twin = histograms.segment_compact_history_attribution(*args, PM if pm is None else pm, top, CAP)
        for f, t in zip(FIELDS, TWIN):
            a, b = getattr(got, f), getattr(twin, t)
            assert a.shape == (R, top) and a.dtype.itemsize == b.dtype.itemsize, f
            assert a.tobytes() == b.tobytes(), f
        assert got.loss_all.cpu().numpy().tobytes() == twin.loss_all.tobytes()
        assert torch.equal(rep.compact_tail_history(), before)
    assert (got.kernel >= 0).any()


def test_refused_without_a_compact_call_to_explain(intervals):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    with pytest.raises(RuntimeError, match="compact"):
        rep.compact_tail_attribution()
    rep.individual_tail_scores_records(*intervals[0], permille=PM)  # the dense history
    with pytest.raises(RuntimeError, match="compact"):
        rep.compact_tail_attribution()
    rep.individual_tail_scores_records(*intervals[0], permille=PM, history="compact")
    rep.compact_tail_attribution()
    rep.tail_scores_records(*intervals[1], permille=PM)  # buckets other records into the work tensors
    with pytest.raises(RuntimeError, match="re-used"):
        rep.compact_tail_attribution()
    rep.individual_tail_scores_records(*intervals[1], permille=PM, history="compact")
    rep.compact_tail_attribution()
    rep.individual_tail_scores_records(*intervals[2], permille=PM)
    with pytest.raises(RuntimeError, match="re-used"):
        rep.compact_tail_attribution()


def test_arguments_are_checked(intervals):
    rep = batch.MatrixReporter(R, K, cap=CAP)
    rep.individual_tail_scores_records(*intervals[0], permille=PM, history="compact")
    for bad in (0, 17, True, 1.5):
        with pytest.raises(ValueError, match="top"):
            rep.compact_tail_attribution(bad)
    with pytest.raises(ValueError, match="permille"):
        rep.compact_tail_attribution(4, permille=1001)
    with pytest.raises(NotImplementedError, match="compact"):  # the one-call form stays refused
        rep.individual_tail_scores_records(*intervals[0], permille=PM, attribute=4, history="compact")
    rep.exchange = True  # as a reporter over kernel shards
    with pytest.raises(NotImplementedError, match="exchange=True"):
        rep.compact_tail_attribution()


def test_the_dense_path_is_what_it_was(intervals):
    plain = batch.MatrixReporter(R, K, cap=CAP)
    rep = batch.MatrixReporter(R, K, cap=CAP)
    for recs, rec_off in intervals:
        want = plain.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR, attribute=4)
        rep.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR, history="compact")
        rep.compact_tail_attribution(4)
        got = rep.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR, attribute=4)
        for f in ("score", "tail_ns", "total_ns", "history_share", "stragglers", "base_tail_ns", "base_total_ns"):
            assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
        _rows_equal(got.attribution, want.attribution, list(range(R)))
        assert torch.equal(rep._htail["hist"], plain._htail["hist"])
