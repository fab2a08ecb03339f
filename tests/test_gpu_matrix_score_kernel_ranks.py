"""``MatrixReporter.score_kernel_ranks`` -- per kernel the ranks behind its score loss -- on a
reporter of 8 ranks x 6 kernels whose rank 5 runs every call of kernel 2 at 1.5x (a median shift,
not a tail).  What comes out equals the host twin (``histograms.score_rank_attribution``) on the
reporter's statistics copied to the host: integers, and f64 as bits.

0.97, not the default 0.75: kernel 2 is 150 of the slow rank's 1,385 us per step, and a third of
that is lost, so its score is about 0.964 (the first test checks it on the CPU)."""
import numpy as np
import pytest
import torch

from nvidia_resiliency_ext.straggler import batch, histograms

R, K, CALLS, SLOW, HOT, THR = 8, 6, 32, 5, 2, 0.97
BASE_NS = [20_000, 55_000, 100_000, 150_000, 310_000, 700_000]  # per kernel


def durations(slow=True):
    """ns [R, K, CALLS]: every call of kernel k takes BASE_NS[k]; rank SLOW's calls of kernel HOT
    take 1.5 times as long."""
    ns = np.broadcast_to(np.array(BASE_NS, np.int32)[None, :, None], (R, K, CALLS)).copy()
    if slow:
        ns[SLOW, HOT] = ns[SLOW, HOT] * 3 // 2
    return ns


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def reference(num, med):
    """The relative reference of a report: per kernel the least MED, NaN unless every rank has it."""
    present = (num > 0).all(0)
    return np.where(present, np.where(num > 0, med, np.inf).min(0), np.nan).astype(np.float32)


def same(got, rep, top, kind, rows=None):
    st = rep.stats.cpu()
    num, med, avg = (getattr(st, f).numpy().reshape(R, K) for f in ("num", "med", "avg"))
    kw = dict(ref=reference(num, med)) if kind == "relative" else dict(hist=rep.hist.cpu().numpy())
    ref = histograms.score_rank_attribution(num, med, avg, top, kind, rows=rows, **kw)
    assert got.rank.dtype == np.int32 and got.rank.shape == (K, top)
    assert np.array_equal(got.rank, ref.idx)
    nan = np.isnan(ref.loss)
    for g, w in ((got.loss_us, ref.loss), (got.score, ref.score)):
        assert np.array_equal(np.isnan(g), nan) and np.array_equal(bits(g[~nan]), bits(w[~nan]))
    assert np.array_equal(got.taken, ref.taken) and np.array_equal(got.positive, ref.positive)
    assert got.err == ref.err == 0
    return ref


def test_the_fixture_on_the_cpu():
    ns = durations()
    num = np.full((R, K), CALLS, np.int32)
    med = (np.median(ns, axis=2) / 1000.0).astype(np.float32)
    avg = (ns.mean(axis=2) / 1000.0).astype(np.float32)
    loss, s, err = histograms.score_losses(num, med, avg, "relative", ref=reference(num, med))
    w = num.astype(np.float64) * avg.astype(np.float64)
    score = (s * w).sum(1) / w.sum(1)
    assert err == 0 and [r for r in range(R) if score[r] < THR] == [SLOW]
    assert 0.75 < score[SLOW] < THR and (np.delete(score, SLOW) == 1.0).all()
    ranks = histograms.score_rank_attribution(num, med, avg, 3, "relative", ref=reference(num, med))
    assert ranks.idx[HOT, 0] == SLOW and ranks.positive[HOT] == 1 and ranks.taken[HOT] == R
    assert ranks.positive.sum() == 1 and abs(ranks.score[HOT, 0] - 1 / 1.5) < 1e-6


@pytest.mark.gpu
def test_relative_flagged_and_buffer_reuse():
    rep = batch.MatrixReporter(R, K, thr_rel=THR, thr_ind=THR)
    res = rep.report(torch.from_numpy(durations()).cuda(), CALLS)
    assert res.stragglers_relative.tolist() == [r == SLOW for r in range(R)]
    got = rep.score_kernel_ranks(top=3)
    same(got, rep, 3, "relative")
    assert got.rank[HOT, 0] == SLOW and got.positive[HOT] == 1 and got.loss_us[HOT, 0] > 0
    ptrs = {k: v.data_ptr() for k, v in rep._sranks[3].items() if v is not None}
    # restricted to the flagged ranks: a numpy mask, a device tensor, bool and uint8
    for flagged in (res.stragglers_relative, torch.from_numpy(res.stragglers_relative).cuda(),
                    res.stragglers_relative.astype(np.uint8)):
        only = rep.score_kernel_ranks(top=3, flagged=flagged)
        same(only, rep, 3, "relative", res.stragglers_relative)
        assert only.taken.tolist() == [1] * K and only.rank[:, 0].tolist() == [SLOW] * K
        assert (only.rank[:, 1:] == -1).all()
    # the second call reused the buffers, another top has its own
    assert {k: v.data_ptr() for k, v in rep._sranks[3].items() if v is not None} == ptrs
    same(rep.score_kernel_ranks(top=16), rep, 16, "relative")
    assert sorted(rep._sranks) == [3, 16]
    # the default top and kind
    assert rep.score_kernel_ranks().rank.shape == (K, 8)


@pytest.mark.gpu
def test_individual_after_a_healthy_and_a_slow_report():
    rep = batch.MatrixReporter(R, K, thr_rel=THR, thr_ind=THR)
    rep.report(torch.from_numpy(durations(False)).cuda(), CALLS)
    first = rep.score_kernel_ranks(top=3, kind="individual")
    same(first, rep, 3, "individual")
    assert not first.positive.any()
    hist = rep.hist.clone()
    res = rep.report(torch.from_numpy(durations()).cuda(), CALLS)
    assert res.stragglers_individual.tolist() == [r == SLOW for r in range(R)]
    got = rep.score_kernel_ranks(top=3, kind="individual")
    same(got, rep, 3, "individual")
    assert got.rank[HOT, 0] == SLOW and got.positive.tolist() == [int(k == HOT) for k in range(K)]
    assert torch.equal(rep.hist, hist)  # read only: the healthy report's minima stand


@pytest.mark.gpu
def test_the_report_is_unchanged_by_the_call():
    ns1 = torch.from_numpy(durations()).cuda()
    ns2 = torch.from_numpy((durations() * 1.1).astype(np.int32)).cuda()
    plain, probed = batch.MatrixReporter(R, K), batch.MatrixReporter(R, K)
    plain.report(ns1, CALLS)
    probed.report(ns1, CALLS)
    probed.score_kernel_ranks(top=8)
    probed.score_kernel_ranks(top=8, kind="individual", flagged=np.arange(R) % 2 == 0)
    for f in ("num", "med", "avg"):
        assert torch.equal(getattr(plain.stats, f), getattr(probed.stats, f))
    a, b = plain.report(ns2, CALLS), probed.report(ns2, CALLS)
    for f in ("gpu_relative", "gpu_individual"):
        assert np.array_equal(bits(getattr(a, f)), bits(getattr(b, f)))
    assert np.array_equal(a.stragglers_relative, b.stragglers_relative) and a.err == b.err == 0
    assert torch.equal(plain.hist, probed.hist)


@pytest.mark.gpu
def test_refusals_allocate_and_launch_nothing():
    rep = batch.MatrixReporter(R, K)
    bad = [(dict(flagged=np.ones(R + 1, bool)), "flagged"), (dict(flagged=np.ones(R, np.int32)), "flagged"),
           (dict(flagged=torch.ones(R, dtype=torch.float32, device="cuda")), "flagged"),
           (dict(top=0), "top"), (dict(top=17), "top"), (dict(kind="sections"), "kind")]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            rep.score_kernel_ranks(**kw)
    for kind in ("relative", "individual"):
        off = batch.MatrixReporter.__new__(batch.MatrixReporter)  # a shell: the refusal comes first
        off.exchange, off.relative, off.individual = False, kind != "relative", kind != "individual"
        with pytest.raises(RuntimeError, match=kind):
            off.score_kernel_ranks(top=2, kind=kind)
    rep.exchange = True
    with pytest.raises(NotImplementedError, match="exchange"):
        rep.score_kernel_ranks(top=2)
    rep.exchange = False
    assert rep._sranks == {} and torch.cuda.memory_allocated() == before


@pytest.mark.gpu
def test_a_reporter_built_without_the_kind():
    with pytest.raises(RuntimeError, match="relative"):
        batch.MatrixReporter(2, 3, relative=False).score_kernel_ranks(top=2, kind="relative")
    with pytest.raises(RuntimeError, match="individual"):
        batch.MatrixReporter(2, 3, individual=False).score_kernel_ranks(top=2, kind="individual")
