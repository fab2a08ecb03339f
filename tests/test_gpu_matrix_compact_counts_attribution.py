"""GPU: ``MatrixReporter.compact_tail_attribution(counts=)`` -- the kernels behind the individual
tail scores of [R, K, 240] counts against the compact history -- on a small reporter over
clustered counts (``_histogram_compact_cases.clustered``: nothing folds): it equals, byte for
byte, the ``.attribution`` of a second reporter's ``individual_tail_scores(counts, attribute=top)``
against the dense history built from the same intervals; under ``absorb="healthy"`` for the rank
that was flagged; the compact history is bit-identical across the method; a pending record-stream
``compact_tail_attribution()`` stays valid; the refusals fire as specified."""
import numpy as np
import pytest
import torch

import _histogram_compact_cases as HC
from nvidia_resiliency_ext.straggler import batch, histograms, synth

pytestmark = pytest.mark.gpu

R, K, CAP, SLOW, PM, THR, TOP = 4, 50, 32, 2, 950, 0.95, 8


def up(c):
    return torch.from_numpy(c.view(np.int32)).cuda()


@pytest.fixture(scope="module")
def intervals():
    """Three intervals of the same clustered counts (a healthy rank's interval is its history);
    in the last, rank SLOW has a tenth of its calls of every kernel 24 buckets (8 x) higher."""
    base = HC.clustered(np.random.default_rng(11), R, K)
    out = [base, base.copy(), base.copy()]
    slow = out[2]
    for k in range(K):
        b = int(np.flatnonzero(slow[SLOW, k])[-1])
        slow[SLOW, k, min(b + 24, 239)] += max(int(slow[SLOW, k, b]) // 10, 1)
    return out


def fields_of(a):
    out = []
    for f in vars(a):
        v = getattr(a, f)
        if isinstance(v, np.ndarray):
            out.append((f, v))
    assert len(out) >= 7
    return out


def same_rows(got, want, rows):
    for (f, g), (_, w) in zip(fields_of(got), fields_of(want)):
        assert g.dtype == w.dtype and g.shape == w.shape, f
        assert g[rows].tobytes() == w[rows].tobytes(), f
    assert torch.equal(got.loss_all[rows].view(torch.int64), want.loss_all[rows].view(torch.int64))


def test_equals_the_dense_reporter_s_attribution(intervals):
    compact, dense = batch.MatrixReporter(R, K, cap=CAP), batch.MatrixReporter(R, K, cap=CAP)
    for c in intervals[:2]:
        a = compact.individual_tail_scores(up(c), permille=PM, threshold=THR, absorb="always",
                                           history="compact")
        dense.individual_tail_scores(up(c), permille=PM, threshold=THR, absorb="always")
        assert not a.folded.any()
    d = up(intervals[2])
    got_s = compact.individual_tail_scores(d, permille=PM, threshold=THR, absorb="never", history="compact")
    assert got_s.folded.tolist() == [0] * R and got_s.attribution is None
    before = compact.compact_tail_history().clone()
    want_s = dense.individual_tail_scores(d, permille=PM, threshold=THR, absorb="never", attribute=TOP)
    assert got_s.score.tobytes() == want_s.score.tobytes()
    got = compact.compact_tail_attribution(TOP, counts=d)  # permille: the score call's
    same_rows(got, want_s.attribution, slice(None))
    assert (got.kernel[SLOW] >= 0).all() and (got.loss_ns[SLOW] > 0).all()
    assert torch.equal(compact.compact_tail_history(), before)  # bit-identical
    assert compact._rtail is None  # the bucketing work tensors: not needed, not touched
    # an explicit permille, and the host twin on the history as it stands
    got = compact.compact_tail_attribution(4, counts=d, permille=900)
    twin = histograms.compact_history_attribution(intervals[2], before.cpu().numpy(), 900, 4)
    assert got.kernel.tobytes() == twin.idx.tobytes() and got.loss_ns.tobytes() == twin.loss.tobytes()
    assert got.loss_all.cpu().numpy().tobytes() == twin.loss_all.tobytes()
    assert torch.equal(compact.compact_tail_history(), before)


def test_healthy_absorb_the_flagged_rank_s_rows_equal_the_dense_reporter_s(intervals):
    compact, dense = batch.MatrixReporter(R, K, cap=CAP), batch.MatrixReporter(R, K, cap=CAP)
    kw = dict(permille=PM, threshold=THR, absorb="healthy")
    for c in intervals[:2]:
        compact.individual_tail_scores(up(c), history="compact", **kw)
        dense.individual_tail_scores(up(c), **kw)
    d = up(intervals[2])
    got_s = compact.individual_tail_scores(d, history="compact", **kw)
    want_s = dense.individual_tail_scores(d, attribute=TOP, **kw)
    assert got_s.stragglers.tolist() == want_s.stragglers.tolist() == [r == SLOW for r in range(R)]
    assert not got_s.folded.any()
    before = compact.compact_tail_history().clone()
    got = compact.compact_tail_attribution(TOP, counts=d)
    # the flagged rank was not absorbed: its history is the one the score saw
    same_rows(got, want_s.attribution, slice(SLOW, SLOW + 1))
    assert torch.equal(compact.compact_tail_history(), before)


def test_a_pending_record_stream_attribution_stays_valid(intervals):
    zc = synth.zipf_counts(K, top=256)
    slot, occ = synth.zipf_order(zc)
    t32 = lambda a: torch.from_numpy(a.view(np.int32)).cuda()  # noqa: E731
    none = torch.zeros(R, dtype=torch.uint8, device="cuda")
    rec_off = torch.arange(R + 1, dtype=torch.int64, device="cuda") * slot.size
    recs = synth.synth_records(R, t32(slot), t32(occ), K, int(zc.max()), straggler=none)
    rep = batch.MatrixReporter(R, K, cap=CAP)
    for _ in range(2):
        rep.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR, absorb="always",
                                           history="compact")
    rep.individual_tail_scores_records(recs, rec_off, permille=PM, threshold=THR, absorb="never",
                                       history="compact")
    want = rep.compact_tail_attribution(4)
    want = {f: v.copy() for f, v in fields_of(want)}
    d = up(intervals[0])
    with pytest.raises(RuntimeError, match="permille=None"):  # no compact counts call ran
        rep.compact_tail_attribution(4, counts=d)
    rep.compact_tail_attribution(4, counts=d, permille=900)
    again = rep.compact_tail_attribution(4)
    for f, v in fields_of(again):
        assert v.tobytes() == want[f].tobytes(), f
    assert rep._rtail["owner"] == "compact"


def test_refusals(intervals):
    d = up(intervals[0])
    rep = batch.MatrixReporter(R, K, cap=CAP)
    with pytest.raises(ValueError, match="counts must have shape"):
        rep.compact_tail_attribution(4, counts=d[:, :K - 1])
    with pytest.raises(RuntimeError, match="no compact history"):
        rep.compact_tail_attribution(4, counts=d, permille=PM)
    with pytest.raises(ValueError, match="top"):
        rep.compact_tail_attribution(17, counts=d)
    assert rep._ctail is None and rep._rtail is None and rep._htail is None
    with pytest.raises(NotImplementedError, match=r"compact_tail_attribution\(counts="):
        rep.individual_tail_scores(d, permille=PM, attribute=4, history="compact")
    rep.exchange = True
    with pytest.raises(NotImplementedError, match="exchange"):
        rep.compact_tail_attribution(4, counts=d)
