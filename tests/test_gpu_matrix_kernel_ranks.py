"""``MatrixReporter.kernel_ranks`` -- per kernel the ranks behind its tail loss -- on a reporter of
8 ranks x 6 kernels whose rank 5 is slow on every 4th call of kernel 2 only.  The ``loss_all`` of
every attribution family goes in, and what comes out equals the host twin
(``histograms.rank_attribution``) on a host copy of that matrix: integers, and f64 as bits.

950, not 990: the slow rank's calls are 100 of the 3,200 samples of kernel 2 (3.1 %), and the
quantile must leave more room than that share (the first test checks it on the CPU)."""
import numpy as np
import pytest
import torch

from nvidia_resiliency_ext.straggler import batch, histograms

R, K, CALLS, SLOW, HOT, PM, THR = 8, 6, 400, 5, 2, 950, 0.95
BASE_NS = [20_000, 55_000, 100_000, 150_000, 310_000, 700_000]  # per kernel


def durations(slow=True):
    """ns [R, K, CALLS]: every call of kernel k takes BASE_NS[k]; rank SLOW's every 4th call of
    kernel HOT takes four times as long."""
    ns = np.broadcast_to(np.array(BASE_NS, np.uint32)[None, :, None], (R, K, CALLS)).copy()
    if slow:
        ns[SLOW, HOT, ::4] *= 4
    return ns


def counts_of(ns):
    c = np.zeros((R, K, histograms.BINS), np.uint32)
    b = histograms.bucket_of(ns)
    for r in range(R):
        for k in range(K):
            c[r, k] = np.bincount(b[r, k], minlength=histograms.BINS)
    return c


def records_of(ns):
    """The same calls as push-ordered record streams {slot, ns}, one per rank."""
    recs = np.empty((R, CALLS, K, 2), np.uint32)
    recs[..., 0] = np.arange(K, dtype=np.uint32)[None, None, :]
    recs[..., 1] = ns.transpose(0, 2, 1)
    off = np.arange(R + 1, dtype=np.int64) * (CALLS * K)
    return (torch.from_numpy(recs.reshape(-1, 2).view(np.int32)).cuda(), torch.from_numpy(off).cuda())


def up(c):
    return torch.from_numpy(c.view(np.int32)).cuda()


def same(got, loss_all, top, rows=None):
    ref = histograms.rank_attribution(loss_all.cpu().numpy(), top, rows)
    assert got.rank.dtype == np.int32 and got.rank.shape == (K, top)
    assert np.array_equal(got.rank, ref.idx)
    assert np.array_equal(got.loss_ns.view(np.uint64), ref.loss.view(np.uint64))
    assert np.array_equal(got.taken, ref.taken) and np.array_equal(got.positive, ref.positive)
    return ref


def test_the_fixture_on_the_cpu():
    c = counts_of(durations())
    s = histograms.tail_scores(c, PM)
    assert [r for r in range(R) if s.score[r] < THR] == [SLOW]
    a = histograms.tail_attribution(c, PM, 4)
    assert a.idx[SLOW, 0] == HOT and a.loss[SLOW, 0] > 0
    ranks = histograms.rank_attribution(a.loss_all, 3)
    assert ranks.idx[HOT, 0] == SLOW and ranks.positive[HOT] == 1 and ranks.taken[HOT] == R
    # at 990 the slow calls (3.1 % of the kernel's samples) ARE the quantile's bucket: no tail
    assert not (histograms.tail_scores(c, 990).score < THR).any()


@pytest.mark.gpu
def test_fleet_counts_flagged_and_buffer_reuse():
    rep = batch.MatrixReporter(R, K)
    res = rep.tail_scores(up(counts_of(durations())), permille=PM, threshold=THR, attribute=4)
    assert res.stragglers.tolist() == [r == SLOW for r in range(R)]
    la = res.attribution.loss_all
    got = rep.kernel_ranks(la, top=3)
    same(got, la, 3)
    assert got.rank[HOT, 0] == SLOW and got.positive[HOT] >= 1 and got.loss_ns[HOT, 0] > 0
    ptrs = {k: v.data_ptr() for k, v in rep._kranks[3].items() if v is not None}
    # restricted to the flagged ranks: a numpy mask, a device tensor, bool and uint8
    for flagged in (res.stragglers, torch.from_numpy(res.stragglers).cuda(),
                    res.stragglers.astype(np.uint8)):
        only = rep.kernel_ranks(la, top=3, flagged=flagged)
        same(only, la, 3, res.stragglers)
        assert only.taken.tolist() == [1] * K and only.rank[:, 0].tolist() == [SLOW] * K
        assert (only.rank[:, 1:] == -1).all()
    # the second call reused the buffers, another top has its own
    assert {k: v.data_ptr() for k, v in rep._kranks[3].items() if v is not None} == ptrs
    same(rep.kernel_ranks(la, top=16), la, 16)
    assert sorted(rep._kranks) == [3, 16]
    # the default top
    assert rep.kernel_ranks(la).rank.shape == (K, 8)


@pytest.mark.gpu
def test_the_other_families_loss_all():
    healthy, slow = durations(False), durations()
    # individual leg, dense history
    rep = batch.MatrixReporter(R, K)
    rep.individual_tail_scores(up(counts_of(healthy)), permille=PM, threshold=THR, absorb="always")
    res = rep.individual_tail_scores(up(counts_of(slow)), permille=PM, threshold=THR, attribute=4)
    got = rep.kernel_ranks(res.attribution.loss_all, top=3)
    same(got, res.attribution.loss_all, 3)
    assert got.rank[HOT, 0] == SLOW and got.positive[HOT] == 1
    # record streams, fleet leg
    rep = batch.MatrixReporter(R, K)
    res = rep.tail_scores_records(*records_of(slow), permille=PM, threshold=THR, attribute=4)
    got = rep.kernel_ranks(res.attribution.loss_all, top=3, flagged=res.stragglers)
    same(got, res.attribution.loss_all, 3, res.stragglers)
    assert got.rank[HOT].tolist() == [SLOW, -1, -1]
    # record streams, individual leg
    rep = batch.MatrixReporter(R, K)
    rep.individual_tail_scores_records(*records_of(healthy), permille=PM, threshold=THR, absorb="always")
    res = rep.individual_tail_scores_records(*records_of(slow), permille=PM, threshold=THR, attribute=4)
    got = rep.kernel_ranks(res.attribution.loss_all, top=3)
    same(got, res.attribution.loss_all, 3)
    assert got.rank[HOT, 0] == SLOW
    # the compact history
    rep = batch.MatrixReporter(R, K)
    rep.individual_tail_scores_records(*records_of(healthy), permille=PM, threshold=THR, absorb="always",
                                       history="compact")
    rep.individual_tail_scores_records(*records_of(slow), permille=PM, threshold=THR, absorb="never",
                                       history="compact")
    att = rep.compact_tail_attribution(4)
    got = rep.kernel_ranks(att.loss_all, top=3)
    same(got, att.loss_all, 3)
    assert got.rank[HOT, 0] == SLOW


@pytest.mark.gpu
def test_refusals_allocate_and_launch_nothing():
    rep = batch.MatrixReporter(R, K)
    good = torch.zeros((R, K), dtype=torch.float64, device="cuda")
    wide = torch.zeros((K, R), dtype=torch.float64, device="cuda").t()  # [R, K], columns contiguous
    bad = [(good.cpu(), {}, "device"), (good.float(), {}, "float64"), (good[:, :5], {}, "shape"),
           (good[:4], {}, "shape"), (good.reshape(K, R), {}, "shape"), (wide, {}, "contiguous rows"),
           (good, dict(flagged=np.ones(R + 1, bool)), "flagged"),
           (good, dict(flagged=np.ones(R, np.int32)), "flagged"),
           (good, dict(flagged=torch.ones(R, dtype=torch.float32, device="cuda")), "flagged"),
           (good, dict(top=0), "top"), (good, dict(top=17), "top")]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for t, kw, word in bad:
        with pytest.raises(ValueError, match=word):
            rep.kernel_ranks(t, **kw)
    assert rep._kranks == {} and torch.cuda.memory_allocated() == before
    # a row stride above K is no refusal
    padded = torch.full((R, K + 3), 1e300, dtype=torch.float64, device="cuda")
    padded[:, :K] = torch.arange(R * K, dtype=torch.float64, device="cuda").view(R, K)
    got = rep.kernel_ranks(padded[:, :K], top=2)
    assert got.rank.tolist() == [[R - 1, R - 2]] * K
